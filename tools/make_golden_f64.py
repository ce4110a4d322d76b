"""Fixture G12 (tests/golden/g12_f64.npz): the real reference in DOUBLE.

`max_spherical_sliced_w.py` is loaded by file path (as oracle.make_golden._load does) and its own `sliced_cost` and
`backward()` run on the CPU on double inputs that are NOT representable in float32 (seeded double randn, normalised in
double), so the fixture pins what a caller of the reference gets who passes double clouds and double directions
(`dtype = u_values.dtype`, :153-160).

Needs the reference next to the repository, so it runs on a build machine only; the tests read the .npz.
Run:  python tools/make_golden_f64.py [path/to/max_spherical_sliced_w.py]

Contents, per case `n{n}_L{L}`: x, y (n, 3), U (L, 3, 2); per p: `val_*` the reference's value, `slices_*` its per-slice
costs (binary_search_circle / emd1D_circle on the coordinates its own lines :270-279 produce), `gx_*` and (n = 256)
`gy_*` its gradients.  `grad_gap_*`: the largest entry of |exact_shift.ssw_pair_grad - reference gradient| over the
largest reference entry, per case with p != 1 -- the reference's bisection ends a hair off the kink and mixes two
neighbouring shifts, the kernels implement the minimum over shifts; the GPU test's bound on the G12 gradients is ten
times the worst of these figures, which are measured here on the CPU and never on a kernel's output.

Measured when the fixture was made (this file's CASES and seeds):
    n256_L32  p=2: gx 3.1e-15  gy 1.7e-14     p=3: gx 7.5e-15  gy 1.1e-14
    n1200_L8  p=2: gx 2.5e-14
    worst 2.54e-14  ->  bound on the G12 gradients for p != 1: 2.54e-13 of the largest entry
    slice costs, exhaustive minimum - reference: within [-7.2e-18, 3.3e-19]
On these cases the reference's bisection ends ON the kink (on other seeds it mixes two shifts and the gap reaches 4e-6,
DESIGN 5), so the bound is at rounding level.  The figures are stored in the fixture as `grad_gap_*`, `grad_gap_worst`
and `slice_gap_*`; tests/test_f64_cpu.py recomputes them.
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
from oracle import exact_shift  # noqa: E402

REFERENCE = "/root/reference/Point_Cloud_Resistration/losses/max_spherical_sliced_w.py"
OUT = os.path.join(ROOT, "tests", "golden", "g12_f64.npz")
CASES = (                      # n, L, powers, store gy, seed
    (256, 32, (1, 2, 3), True, 12001),
    (1200, 8, (1, 2), False, 12002),
)


def _load(name, path):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _np(t):
    return t.detach().cpu().numpy()


def inputs(n, L, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.nn.functional.normalize(torch.randn(n, 3, generator=g, dtype=torch.float64), dim=-1)
    y = torch.nn.functional.normalize(torch.randn(n, 3, generator=g, dtype=torch.float64), dim=-1)
    U = torch.linalg.qr(torch.randn(L, 3, 2, generator=g, dtype=torch.float64))[0]
    return x, y, U


def reference_slices(ref, x, y, U, p):
    """Per-slice costs by the reference's own circle routines on the coordinates of its lines :270-279."""
    def coords(X):
        planar = torch.nn.functional.normalize(torch.matmul(torch.transpose(U, 1, 2)[:, None], X[:, :, None]).reshape(
            U.shape[0], X.shape[0], 2), p=2, dim=-1)
        return (torch.atan2(-planar[:, :, 1], -planar[:, :, 0]) + math.pi) / (2 * math.pi)
    cu, cv = coords(x), coords(y)
    if p == 1:
        return ref.emd1D_circle(cu, cv)
    return ref.binary_search_circle(cu, cv, p=p)


def main(path=REFERENCE):
    ref = _load("ref_ssw", path)
    torch.set_num_threads(8)
    out = {}
    worst = 0.0
    for n, L, powers, with_gy, seed in CASES:
        tag = f"n{n}_L{L}"
        x, y, U = inputs(n, L, seed)
        assert not np.array_equal(_np(x), _np(x).astype(np.float32).astype(np.float64))
        out[f"x_{tag}"], out[f"y_{tag}"], out[f"U_{tag}"] = _np(x), _np(y), _np(U)
        for p in powers:
            xs, ys = x.clone().requires_grad_(True), y.clone().requires_grad_(True)
            val = ref.sliced_cost(xs, ys, U, p=p)
            val.backward()
            assert val.dtype == torch.float64 and xs.grad.dtype == torch.float64
            slices = reference_slices(ref, x, y, U, p)
            assert abs(slices.mean().item() - val.item()) <= 1e-15 + 1e-13 * abs(val.item()), (slices.mean(), val)
            out[f"val_{tag}_p{p}"] = _np(val)
            out[f"slices_{tag}_p{p}"] = _np(slices)
            out[f"gx_{tag}_p{p}"] = _np(xs.grad)
            if with_gy:
                out[f"gy_{tag}_p{p}"] = _np(ys.grad)
            if p != 1:
                ex, ey = exact_shift.ssw_pair_grad(_np(x), _np(y), _np(U), p)
                gaps = [np.abs(ex - _np(xs.grad)).max() / np.abs(_np(xs.grad)).max()]
                if with_gy:
                    gaps.append(np.abs(ey - _np(ys.grad)).max() / np.abs(_np(ys.grad)).max())
                out[f"grad_gap_{tag}_p{p}"] = np.asarray(gaps)
                worst = max(worst, max(gaps))
                cu, cv = exact_shift.circle_coords(_np(x), _np(U)), exact_shift.circle_coords(_np(y), _np(U))
                cost, _ = exact_shift.circular_ot_equal(cu, cv, p)
                d = cost - _np(slices)
                out[f"slice_gap_{tag}_p{p}"] = np.asarray([d.min(), d.max()])
                print(tag, p, "grad gap", ["%.2e" % g for g in gaps], "slice gap [%.2e, %.2e]" % (d.min(), d.max()))
    out["grad_gap_worst"] = np.asarray(worst)
    print("worst gradient gap %.3e -> bound %.3e" % (worst, 10 * worst))
    np.savez_compressed(OUT, **out)
    print(OUT, os.path.getsize(OUT))
    return 0


if __name__ == "__main__":
    sys.exit(main(*sys.argv[1:]))
