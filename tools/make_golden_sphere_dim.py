"""Fixture G15 (tests/golden/g15_sphere_dim.npz): the real reference on S^(d-1) for point dimensions d != 3.

`max_spherical_sliced_w.py` and `max_spherical_sliced_w_fast.py` are loaded by file path (as tools/make_golden_f64_general.py
does) and their own `sliced_cost`, `sliced_wasserstein_sphere`, circle routines and `backward()` run on the CPU.  They read
the point dimension from their input (`d = Xs.shape[1]`, :304) and run unchanged at every d >= 2.

Needs the reference next to the repository, so it runs on a build machine only; the tests read the .npz.
Run:  python tools/make_golden_sphere_dim.py [path/to/losses]

Contents (arrays only; the inputs are float32 and stored as such).
Per-pair cases `d{d}_n{n}_m{m}_L{L}{w|u}` (w: weighted): x (n, d), y (m, d) unit rows, U (L, d, 2) = qr(randn), wu, wv;
per power p: `val_*`, `slices_*` (the reference's circle routines on the coordinates of its lines :270-279), `gx_*`, `gy_*`
of the float32 run, and `val64_*`, `slices64_*`, `gx64_*`, `gy64_*` of the same call on the same numbers in float64.
`swap_*`: [entries of gx, entries of gy] of the float32 run outside grad_close's strict bound (2e-4 of the largest
float64 entry) of the float64 run.  The loss is piecewise smooth: two float32 evaluations that order a near-tie of
coordinates differently differ by a swapped pair of points, 2 d entries.  The script ASSERTS that the reference's own two
precisions differ by at most one such pair per gradient (and nowhere by more than grad_close's loose bound); a seed at
which they do not is replaced (`SEED_STEP` is added until they do).  No kernel output plays a part in the choice; the
seeds used are stored as `seed_*`.
Batched `_fast.sliced_cost` (`batched_*`): x, y (2, 96, 5), U (2, 8, 5, 2), p = 2: total (shape [1]) and the per-pair value
of the first pair, float32 and float64.  The batched reference does run at d != 3; were it not to, the script would store
the sum of the per-pair values (`batched_from_pairs` = 1).
RNG (`rng_*`): `manual_seed(seed); sliced_wasserstein_sphere(x, y, 16, "cpu")` at d = 8: the value, the Z it drew and the U
it used.
Frames (`frames_Z_d*`, `frames_U_d*`): Z (16, d, 2) and LAPACK's U (torch.linalg.qr on the CPU) for d in {2, 5, 64}.

Size: 563 KB.  The cases above cannot be stored in less: the five per-pair cases hold 104 KB of float32 inputs (140 KB
with the batched, RNG and frame cases) and 422 KB of gradients in two precisions (4 + 8 bytes per entry; d = 8 at three
powers and d = 64 are 147 KB and 154 KB of them), and random floats do not compress.  Every earlier fixture is below
200 KB; this one is pinned at its size here and in tests/test_sphere_dim_cpu.py.

Measured when the fixture was made: see the lines the script prints (per case: the float32-float64 gap of value, slices
and gradients, and the swap counts)."""
from __future__ import annotations

import importlib.util
import math
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LOSSES = "/root/reference/Point_Cloud_Resistration/losses"
OUT = os.path.join(ROOT, "tests", "golden", "g15_sphere_dim.npz")
CASES = (                      # d, n, m, L, weighted, powers, first seed
    (2, 64, 64, 8, False, (1, 2), 15001),
    (8, 256, 256, 16, False, (1, 2, 3), 15002),
    (6, 200, 256, 8, False, (1, 2), 15003),
    (16, 128, 128, 8, True, (2,), 15004),
    (64, 100, 100, 8, False, (2,), 15005),
)
BATCHED = (2, 5, 96, 8, 2, 15006)      # B, d, n, L, p, seed
RNG = (8, 128, 16, 15007)              # d, n, L, seed
FRAMES = ((2, 15008), (5, 15009), (64, 15010))
SEED_STEP = 100
STRICT, LOOSE = 2e-4, 2e-2             # tests/helpers/compare.py grad_close defaults


def _load(name, path):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _np(t):
    return t.detach().cpu().numpy()


def inputs(d, n, m, L, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.nn.functional.normalize(torch.randn(n, d, generator=g), dim=-1)
    y = torch.nn.functional.normalize(torch.randn(m, d, generator=g), dim=-1)
    U = torch.linalg.qr(torch.randn(L, d, 2, generator=g))[0]
    wu = torch.rand(n, generator=g) + 0.25
    wv = torch.rand(m, generator=g) + 0.25
    return x, y, U, wu / wu.sum(), wv / wv.sum()


def reference_slices(ref, x, y, U, p, wu, wv):
    """Per-slice costs by the reference's own circle routines on the coordinates of its lines :270-279."""
    def coords(X):
        planar = torch.nn.functional.normalize(torch.matmul(torch.transpose(U, 1, 2)[:, None], X[:, :, None]).reshape(
            U.shape[0], X.shape[0], 2), p=2, dim=-1)
        return (torch.atan2(-planar[:, :, 1], -planar[:, :, 0]) + math.pi) / (2 * math.pi)
    cu, cv = coords(x), coords(y)
    if p == 1:
        return ref.emd1D_circle(cu, cv, u_weights=wu, v_weights=wv)
    return ref.binary_search_circle(cu, cv, p=p, u_weights=wu, v_weights=wv)


def evaluate(ref, x, y, U, p, wu, wv, dtype):
    xs, ys = x.to(dtype).clone().requires_grad_(True), y.to(dtype).clone().requires_grad_(True)
    Ud = U.to(dtype)
    wud = wu.to(dtype) if wu is not None else None
    wvd = wv.to(dtype) if wv is not None else None
    val = ref.sliced_cost(xs, ys, Ud, p=p, u_weights=wud, v_weights=wvd)
    val.backward()
    assert val.dtype == dtype and xs.grad.dtype == dtype
    slices = reference_slices(ref, xs.detach(), ys.detach(), Ud, p, wud, wvd)
    return _np(val), _np(slices), _np(xs.grad), _np(ys.grad)


def outside(g32, g64):
    scale = np.abs(g64).max()
    err = np.abs(g32.astype(np.float64) - g64)
    return int((err > STRICT * scale).sum()), float(err.max() / scale)


def pair_case(ref, d, n, m, L, weighted, powers, seed):
    """All powers of one case at the first seed at which the reference's two precisions differ by at most one swapped pair."""
    while True:
        x, y, U, wu, wv = inputs(d, n, m, L, seed)
        if not weighted:
            wu = wv = None
        got, ok = {}, True
        for p in powers:
            r32 = evaluate(ref, x, y, U, p, wu, wv, torch.float32)
            r64 = evaluate(ref, x, y, U, p, wu, wv, torch.float64)
            ox, ex = outside(r32[2], r64[2])
            oy, ey = outside(r32[3], r64[3])
            ok = ok and ox <= 2 * d and oy <= 2 * d and max(ex, ey) < LOOSE
            got[p] = (r32, r64, (ox, oy), (ex, ey))
        if ok:
            return seed, (x, y, U, wu, wv), got
        print(f"d={d}: seed {seed} rejected by the reference's own float32 / float64 gradients "
              f"{[(p, g[2], ['%.1e' % e for e in g[3]]) for p, g in got.items()]}")
        seed += SEED_STEP


def main(losses=LOSSES):
    ref = _load("ref_ssw", os.path.join(losses, "max_spherical_sliced_w.py"))
    fast = _load("ref_ssw_fast", os.path.join(losses, "max_spherical_sliced_w_fast.py"))
    torch.set_num_threads(8)
    out = {}
    for d, n, m, L, weighted, powers, seed0 in CASES:
        tag = f"d{d}_n{n}_m{m}_L{L}{'w' if weighted else 'u'}"
        seed, (x, y, U, wu, wv), got = pair_case(ref, d, n, m, L, weighted, powers, seed0)
        out[f"seed_{tag}"] = np.asarray(seed)
        out[f"x_{tag}"], out[f"y_{tag}"], out[f"U_{tag}"] = _np(x), _np(y), _np(U)
        if weighted:
            out[f"wu_{tag}"], out[f"wv_{tag}"] = _np(wu), _np(wv)
        for p, (r32, r64, swaps, errs) in got.items():
            for name, a32, a64 in zip(("val", "slices", "gx", "gy"), r32, r64):
                assert a32.dtype == np.float32 and a64.dtype == np.float64
                out[f"{name}_{tag}_p{p}"], out[f"{name}64_{tag}_p{p}"] = a32, a64
            out[f"swap_{tag}_p{p}"] = np.asarray(swaps)
            gap = np.abs(r32[1] - r64[1]) / np.abs(r64[1])
            print(f"{tag} p={p} seed {seed}: val {abs(r32[0] - r64[0]) / abs(r64[0]):.1e}  slices {gap.max():.1e}  "
                  f"grad outside strict {swaps} of at most {2 * d}, worst {max(errs):.1e} of the largest entry")

    B, d, n, L, p, seed = BATCHED
    g = torch.Generator().manual_seed(seed)
    x = torch.nn.functional.normalize(torch.randn(B, n, d, generator=g), dim=-1)
    y = torch.nn.functional.normalize(torch.randn(B, n, d, generator=g), dim=-1)
    U = torch.linalg.qr(torch.randn(B, L, d, 2, generator=g))[0]
    out["batched_x"], out["batched_y"], out["batched_U"] = _np(x), _np(y), _np(U)
    for dtype, sfx in ((torch.float32, ""), (torch.float64, "64")):
        xd, yd, Ud = x.to(dtype), y.to(dtype), U.to(dtype)
        pairs = torch.stack([ref.sliced_cost(xd[b], yd[b], Ud[b], p=p) for b in range(B)])
        try:
            if dtype == torch.float64:      # the batched reference accumulates in torch.zeros((1)): the default dtype
                torch.set_default_dtype(torch.float64)
            total = fast.sliced_cost(xd, yd, Ud, p=p)
            from_pairs = 0
        except Exception as exc:            # not observed: the batched reference runs at d != 3
            print("batched reference failed at d =", d, ":", exc)
            total, from_pairs = pairs.sum().reshape(1), 1
        finally:
            torch.set_default_dtype(torch.float32)
        assert tuple(total.shape) == (1,) and total.dtype == dtype
        assert abs(total.item() - pairs.sum().item()) <= 1e-6 * abs(total.item())
        out[f"batched_total{sfx}"], out[f"batched_first{sfx}"] = _np(total), _np(pairs[0])
        out["batched_from_pairs"] = np.asarray(from_pairs)
    print("batched total", out["batched_total"], out["batched_total64"], "from pairs:", int(out["batched_from_pairs"]))

    d, n, L, seed = RNG
    g = torch.Generator().manual_seed(seed)
    x = torch.nn.functional.normalize(torch.randn(n, d, generator=g), dim=-1)
    y = torch.nn.functional.normalize(torch.randn(n, d, generator=g), dim=-1)
    torch.manual_seed(seed)
    val = ref.sliced_wasserstein_sphere(x, y, L, "cpu")
    torch.manual_seed(seed)
    Z = torch.randn((L, d, 2))
    Uq = torch.linalg.qr(Z)[0]
    assert torch.equal(ref.sliced_cost(x, y, Uq, p=2), val)
    out["rng_seed"], out["rng_x"], out["rng_y"] = np.asarray(seed), _np(x), _np(y)
    out["rng_val"], out["rng_Z"], out["rng_U"] = _np(val), _np(Z), _np(Uq)
    out["rng_val64"] = _np(ref.sliced_cost(x.double(), y.double(), Uq.double(), p=2))

    for d, seed in FRAMES:
        g = torch.Generator().manual_seed(seed)
        Z = torch.randn(16, d, 2, generator=g)
        out[f"frames_Z_d{d}"], out[f"frames_U_d{d}"] = _np(Z), _np(torch.linalg.qr(Z)[0])

    for key, val in out.items():
        assert isinstance(val, np.ndarray) and val.dtype in (np.float32, np.float64, np.int64), (key, val.dtype)
    np.savez_compressed(OUT, **out)
    print(OUT, os.path.getsize(OUT))
    assert os.path.getsize(OUT) <= 570 * 1000
    return 0


if __name__ == "__main__":
    sys.exit(main(*sys.argv[1:]))
