"""Inputs and references of the frame-gradient tests (test_ssw_dirs_cpu.py, test_ssw_dirs_gpu.py).

Clouds are DISPLACED from each other, as in registration: x uniform on the sphere, y Gaussian with 1.5 added to its first
coordinate and then normalised.  For two samples of one distribution the frame gradient is a cancellation residue (the
mirror's own float32 run is then 1e-3 of the largest entry away from its float64 run at n = 1200); for displaced pairs it
stays within a few 1e-5, which is what makes a 1e-3 bound on the kernel meaningful (asserted per case in the CPU file).

The reference is float64 autograd through `oracle.ref_mirror`; `closed_form` restates the formula the kernels implement
    g[l,:,0] = sum_i coef[l,i] (-b_i) / (2 pi r2_i) x_i,   g[l,:,1] = sum_i coef[l,i] a_i / (2 pi r2_i) x_i
on the mirror's own coefficient rows and is compared with that autograd in the CPU file."""
import functools
import math
from collections import namedtuple

import torch
import torch.nn.functional as F

F64 = torch.float64
Case = namedtuple("Case", "name B n m d L p shared weighted seed")


def _cases():
    out = []

    def add(name, B, n, m, d, L, p, shared=False, weighted=False):
        out.append(Case(name, B, n, m, d, L, p, shared, weighted, 16000 + len(out)))
    # R^3: the sizes around the wave / tile edges, p, B, L, shared and per-pair frames
    add("n1", 1, 1, 1, 3, 3, 2)
    add("n7", 3, 7, 7, 3, 17, 2, shared=True)
    add("n63", 1, 63, 63, 3, 3, 1.5)
    add("n64", 3, 64, 64, 3, 1, 2)
    add("n65", 1, 65, 65, 3, 3, 3, shared=True)
    add("n255", 1, 255, 255, 3, 3, 1)
    add("n256", 3, 256, 256, 3, 3, 2)
    add("n257", 1, 257, 257, 3, 1, 2)
    add("n1000", 1, 1000, 1000, 3, 3, 2)
    add("n64_p1", 3, 64, 64, 3, 17, 1, shared=True)
    add("300x200", 3, 300, 200, 3, 3, 2)
    add("300x200_p1", 1, 300, 200, 3, 3, 1, shared=True)
    add("65x7", 1, 65, 7, 3, 17, 1.5, shared=True)
    add("65x7_p3", 3, 65, 7, 3, 1, 3)
    add("w200", 3, 200, 200, 3, 3, 2, weighted=True)
    add("w200_p1", 1, 200, 200, 3, 17, 1, shared=True, weighted=True)
    add("w200_p15", 1, 200, 200, 3, 3, 1.5, weighted=True)
    # the D-generic path
    for d in (2, 4, 8, 63, 64):
        add(f"d{d}_n65", 3, 65, 65, d, 3, 2)
        add(f"d{d}_300x200", 1, 300, 200, d, 17, 1.5, shared=True)
    for d in (2, 8, 64):
        add(f"d{d}_w200", 1, 200, 200, d, 3, 3, weighted=True)
        add(f"d{d}_n7_p1", 3, 7, 7, d, 1, 1)
        add(f"d{d}_n256", 1, 256, 256, d, 3, 2, shared=True)
    # many rows: the R^3 kernel then gives a wavefront four rows (16-byte loads at n = 8, scalar ones at n = 7); the
    # slice count is no multiple of four, so the last group of every pair is a partial one
    add("rows_n8", 3, 8, 8, 3, 2731, 2)
    add("rows_n7", 3, 7, 7, 3, 2731, 2)
    # the same for the D-generic kernel (four rows per wavefront from 4096 rows on; 1367 slices = 341 groups of 4 and 3)
    add("rows_d5", 3, 70, 7, 5, 1367, 2)
    add("rows_d64", 3, 7, 7, 64, 1367, 1.5)
    return out


CASES = _cases()
BY_NAME = {c.name: c for c in CASES}
# per-pair frames, 16 chosen slices against the mirror: the coefficient rows of the throughput kernels (2048 points, more
# slices than one pass of the grid) and of the cooperative kernels (3000 points)
LARGE = [Case("big2048", 2, 2048, 2048, 3, 520, 2, False, False, 16900),
         Case("big3000", 1, 3000, 3000, 3, 8, 2, False, False, 16901)]


def unit(t):
    return F.normalize(t, dim=-1)


def displaced_pair(g, B, n, m, d, dtype=F64):
    x = unit(torch.randn(B, n, d, generator=g, dtype=dtype))
    y = torch.randn(B, m, d, generator=g, dtype=dtype)
    y[..., 0] += 1.5
    return x, unit(y)


def frames(g, *lead, d=3, dtype=F64):
    return torch.linalg.qr(torch.randn(*lead, d, 2, generator=g, dtype=dtype))[0]


def weights(g, n, dtype=F64):
    w = torch.rand(n, generator=g, dtype=dtype) + 0.1
    return w / w.sum()


def inputs(case):
    """x (B,n,d), y (B,m,d), U (L,d,2) shared or (B,L,d,2), wu (n,) or None, wv (m,) or None -- float64, CPU."""
    g = torch.Generator().manual_seed(case.seed)
    x, y = displaced_pair(g, case.B, case.n, case.m, case.d)
    U = frames(g, case.L, d=case.d) if case.shared else frames(g, case.B, case.L, d=case.d)
    wu = weights(g, case.n) if case.weighted else None
    wv = weights(g, case.m) if case.weighted else None
    return x, y, U, wu, wv


def cast(t, dtype):
    return None if t is None else t.to(dtype)


def mirror_grad(x, y, U, p, wu=None, wv=None, pair_w=None):
    """d/dU of sum_b pair_w[b] * (mean over slices of pair b's costs) by autograd through oracle.ref_mirror, in the dtype
    of the inputs; U (L,d,2) shared or (B,L,d,2); returns the shape of U."""
    from oracle import ref_mirror
    Ug = U.detach().clone().requires_grad_(True)
    total = 0
    for b in range(x.shape[0]):
        Ub = Ug if Ug.dim() == 3 else Ug[b]
        w = 1.0 if pair_w is None else pair_w[b]
        total = total + w * ref_mirror.per_slice_costs(x[b], y[b], Ub, p, wu, wv).mean()
    return torch.autograd.grad(total, Ug)[0]


@functools.lru_cache(maxsize=None)
def reference(name):
    """float64 mirror gradient of the total (sum over pairs of the slice means) of a case of CASES."""
    case = BY_NAME[name]
    x, y, U, wu, wv = inputs(case)
    return mirror_grad(x, y, U, case.p, wu, wv)


def closed_form(x, y, U, p, wu=None, wv=None):
    """The kernels' formula in float64 on ONE pair: x (n,d), y (m,d), U (L,d,2) -> (L,d,2), the gradient of the mean over
    slices.  The coefficient rows are the mirror's d cost / d coordinate (autograd down to the coordinates only)."""
    from oracle import ref_mirror
    cs = ref_mirror.circle_coords(x, U).detach().requires_grad_(True)
    ct = ref_mirror.circle_coords(y, U).detach().requires_grad_(True)
    if p == 1:
        cost = ref_mirror.circular_w1_level_median(cs, ct, wu, wv)
    else:
        cost = ref_mirror.circular_ot_bisect(cs, ct, p=p, u_weights=wu, v_weights=wv)
    coef_s, coef_t = torch.autograd.grad(cost.mean(), (cs, ct))

    def fold(X, coef):
        ab = torch.einsum("ldk,nd->lnk", U, X)
        a, b = ab[..., 0], ab[..., 1]
        r2 = a * a + b * b
        w = torch.where(r2 > 0, coef / (2 * math.pi * r2), torch.zeros_like(r2))
        return torch.stack((torch.einsum("ln,nd->ld", -w * b, X), torch.einsum("ln,nd->ld", w * a, X)), dim=-1)
    return fold(x, coef_s) + fold(y, coef_t)


def closed_form_total(x, y, U, p, wu=None, wv=None):
    """`closed_form` over the pairs, in the shape of U (shared frames: summed over the pairs)."""
    rows = [closed_form(x[b], y[b], U if U.dim() == 3 else U[b], p, wu, wv) for b in range(x.shape[0])]
    return torch.stack(rows).sum(0) if U.dim() == 3 else torch.stack(rows)


# ---- gradcheck inputs (float64 paths): seeds for which a finite-difference step of 1e-6 stays on one smooth piece ----
GRADCHECK_EQUAL_SEED, GRADCHECK_GENERAL_SEED = 16801, 16802


def gradcheck_equal(seed=GRADCHECK_EQUAL_SEED):
    """x (2,12,3), y (2,12,3), U (2,2,3,2)."""
    g = torch.Generator().manual_seed(seed)
    x, y = displaced_pair(g, 2, 12, 12, 3)
    return x, y, frames(g, 2, 2)


def gradcheck_general(seed=GRADCHECK_GENERAL_SEED):
    """x (2,12,3), y (2,9,3), U (2,2,3,2), wu (12,), wv (9,)."""
    g = torch.Generator().manual_seed(seed)
    x, y = displaced_pair(g, 2, 12, 9, 3)
    return x, y, frames(g, 2, 2), weights(g, 12), weights(g, 9)


def gradcheck_margins_ok(x, y, U, wu, wv, p):
    """The margins test_f64_general_gpu.py asks of its own gradcheck inputs (coordinates apart, an isolated minimiser /
    the median threshold away), with uniform weights written out where the case has none."""
    from helpers import f64_general_cases
    wu = torch.full((x.shape[1],), 1.0 / x.shape[1], dtype=F64) if wu is None else wu
    wv = torch.full((y.shape[1],), 1.0 / y.shape[1], dtype=F64) if wv is None else wv
    return f64_general_cases.gradcheck_margins_ok(x, y, U, wu, wv, p)
