"""Fixture G14 (tests/golden/g14_f64_general.npz): the real reference in DOUBLE on unequal-size and weighted clouds.

`max_spherical_sliced_w.py` is loaded by file path (as tools/make_golden_f64.py does) and its own `sliced_cost`,
`binary_search_circle`, `emd1D_circle` and `backward()` run on the CPU on double inputs that are NOT representable in
float32 (seeded double randn / rand, asserted), so the fixture pins what a caller of the reference gets who passes
double clouds of two sizes, with or without weights.

Needs the reference next to the repository, so it runs on a build machine only; the tests read the .npz.
Run:  python tools/make_golden_f64_general.py [path/to/max_spherical_sliced_w.py]

Contents.  Sliced cases `n{n}_m{m}_L{L}{w|u}` (w: weighted, u: uniform): x (n, 3), y (m, 3), U (L, 3, 2), wu (n), wv (m);
per p: `val_*` the reference's value, `slices_*` its per-slice costs (its own circle routines on the coordinates of its
lines :270-279), `gx_*` and, where stored, `gy_*` its gradients.  Circle rows `rows_{w|u}`: u (8, 128), v (8, 100), wu,
wv; `bsc_p{p}_*`, `emd1_*`.
`slice_gap_*`: [min, max] of reference - definition per case with p != 1, the definition being the exact minimum over
the cut of tests/helpers/circle_general_exact.py.  `grad_gap_*`: largest entry of |definition gradient - reference
gradient| over the largest reference entry: the reference's bisection ends off the kink (its stopping rule, :191-200)
and mixes the two linear pieces next to it; the kernels implement the minimum.  The GPU test's bound on the G14
gradients for p != 1 is ten times the worst of these figures, which are measured here on the CPU and never on a kernel's
output.

Measured when the fixture was made (this file's cases and seeds; every slice has an isolated minimiser):
    n256_m200_L16w  p=2: gx 8.3e-07 gy 2.2e-07   slice gap [1.6e-15, 1.2e-11]
                    p=3: gx 5.4e-07 gy 7.1e-07   slice gap [7.9e-16, 6.3e-13]
    n256_m200_L8u   p=2: gx 1.4e-06               slice gap [8.0e-14, 5.2e-12]
    n1200_m1000_L4w p=2: gx 5.7e-07               slice gap [2.7e-15, 8.7e-14]
    rows_w  bsc p=1: [-2.1e-17, 6.9e-18]   p=2: [-4.3e-19, 1.6e-11]   p=3: [2.5e-14, 2.9e-12]
    rows_u  bsc p=1: [-2.1e-17, 1.7e-17]   p=2: [-2.2e-19, 1.1e-11]   p=3: [2.5e-14, 2.3e-12]
    worst gradient gap 1.395e-06  ->  bound on the G14 gradients for p != 1: 1.396e-05 of the largest entry
The figures are stored in the fixture as `grad_gap_*`, `grad_gap_worst` and `slice_gap_*`;
tests/test_f64_general_cpu.py recomputes them.
"""
from __future__ import annotations

import importlib.util
import math
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from helpers import circle_general_exact as exact  # noqa: E402

REFERENCE = "/root/reference/Point_Cloud_Resistration/losses/max_spherical_sliced_w.py"
OUT = os.path.join(ROOT, "tests", "golden", "g14_f64_general.npz")
SLICED = (                     # n, m, L, weighted, powers, store gy, seed
    (256, 200, 16, True, (1, 2, 3), True, 14001),
    (256, 200, 8, False, (1, 2), False, 14002),
    (1200, 1000, 4, True, (2,), False, 14003),
)
ROWS = (8, 128, 100, 14004)    # rows, n, m, seed


def _load(name, path):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _np(t):
    return t.detach().cpu().numpy()


def not_float32(a):
    return not np.array_equal(_np(a), _np(a).astype(np.float32).astype(np.float64))


def weights(count, g):
    w = torch.rand(count, generator=g, dtype=torch.float64) + 0.25
    return w / w.sum()


def sliced_inputs(n, m, L, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.nn.functional.normalize(torch.randn(n, 3, generator=g, dtype=torch.float64), dim=-1)
    y = torch.nn.functional.normalize(torch.randn(m, 3, generator=g, dtype=torch.float64), dim=-1)
    U = torch.linalg.qr(torch.randn(L, 3, 2, generator=g, dtype=torch.float64))[0]
    return x, y, U, weights(n, g), weights(m, g)


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


def main(path=REFERENCE):
    ref = _load("ref_ssw", path)
    torch.set_num_threads(8)
    out = {}
    worst = 0.0
    for n, m, L, weighted, powers, with_gy, seed in SLICED:
        tag = f"n{n}_m{m}_L{L}{'w' if weighted else 'u'}"
        x, y, U, wu, wv = sliced_inputs(n, m, L, seed)
        assert all(not_float32(a) for a in (x, y, U, wu, wv))
        out[f"x_{tag}"], out[f"y_{tag}"], out[f"U_{tag}"] = _np(x), _np(y), _np(U)
        if weighted:
            out[f"wu_{tag}"], out[f"wv_{tag}"] = _np(wu), _np(wv)
        else:
            wu = wv = None
        for p in powers:
            xs, ys = x.clone().requires_grad_(True), y.clone().requires_grad_(True)
            val = ref.sliced_cost(xs, ys, U, p=p, u_weights=wu, v_weights=wv)
            val.backward()
            assert val.dtype == torch.float64 and xs.grad.dtype == torch.float64
            slices = reference_slices(ref, x, y, U, p, wu, wv)
            assert abs(slices.mean().item() - val.item()) <= 1e-15 + 1e-13 * abs(val.item()), (slices.mean(), val)
            out[f"val_{tag}_p{p}"] = _np(val)
            out[f"slices_{tag}_p{p}"] = _np(slices)
            out[f"gx_{tag}_p{p}"] = _np(xs.grad)
            if with_gy:
                out[f"gy_{tag}_p{p}"] = _np(ys.grad)
            if p != 1:
                xe, ye = x.clone().requires_grad_(True), y.clone().requires_grad_(True)
                cost, iso = exact.slice_costs(xe, ye, U, p, wu, wv)
                cost.mean().backward()
                gaps = [np.abs(_np(xe.grad) - _np(xs.grad)).max() / np.abs(_np(xs.grad)).max()]
                if with_gy:
                    gaps.append(np.abs(_np(ye.grad) - _np(ys.grad)).max() / np.abs(_np(ys.grad)).max())
                out[f"grad_gap_{tag}_p{p}"] = np.asarray(gaps)
                worst = max(worst, max(gaps))
                d = _np(slices) - _np(cost)
                out[f"slice_gap_{tag}_p{p}"] = np.asarray([d.min(), d.max()])
                print(tag, p, "grad gap", ["%.2e" % g for g in gaps], "slice gap [%.2e, %.2e]" % (d.min(), d.max()),
                      "isolated", int(iso.sum()), "of", L)
    rows, n, m, seed = ROWS
    g = torch.Generator().manual_seed(seed)
    u = torch.rand(rows, n, generator=g, dtype=torch.float64)
    v = torch.rand(rows, m, generator=g, dtype=torch.float64)
    wu, wv = weights(n, g), weights(m, g)
    assert all(not_float32(a) for a in (u, v, wu, wv))
    out["u_rows"], out["v_rows"], out["wu_rows"], out["wv_rows"] = _np(u), _np(v), _np(wu), _np(wv)
    for tag, a, b in (("rows_w", wu, wv), ("rows_u", None, None)):
        for p in (1, 2, 3):
            got = ref.binary_search_circle(u, v, u_weights=a, v_weights=b, p=p)
            out[f"bsc_p{p}_{tag}"] = _np(got)
            cost, _, _ = exact.circle_min(u, v, p, a, b)
            d = _np(got) - _np(cost)
            out[f"slice_gap_{tag}_p{p}"] = np.asarray([d.min(), d.max()])
            print(tag, p, "slice gap [%.2e, %.2e]" % (d.min(), d.max()))
        out[f"emd1_{tag}"] = _np(ref.emd1D_circle(u, v, u_weights=a, v_weights=b))
    out["grad_gap_worst"] = np.asarray(worst)
    print("worst gradient gap %.3e -> bound %.3e" % (worst, 10 * worst))
    for key, val in out.items():
        assert val.dtype == np.float64, key
    np.savez_compressed(OUT, **out)
    print(OUT, os.path.getsize(OUT))
    assert os.path.getsize(OUT) < 200 * 1000
    return 0


if __name__ == "__main__":
    sys.exit(main(*sys.argv[1:]))
