"""References and inputs for the tests of the line transport's gradients with respect to the weights
(test_line_weight_grad_cpu.py, test_line_weight_grad_gpu.py).

Two independent statements of d W_p^p / d weights:

    quantile_merge_w   `quantile_merge` of line_ot_cases.py with the weights left in the graph (any dtype): autograd gives
                       the gradient wherever the CDF ends of the two sides are distinct.  The `searchsorted` arguments
                       are detached: which atoms are active on an interval does not move with the weights.
    potentials_walk    numpy, one row: the Kantorovich potentials by the walk over the merged CDF ends that
                       include/shw.h describes -- on equal levels the u end comes first, segments of zero width count,
                       the jump at the end that closes segment k is c_k - c_(k+1) -- then
                       grad_a = (f - sum abar f) / T_a, grad_b = (g - sum bbar g) / T_b at the original indices.
                       `cost_dtype=np.float32` forms costs, jumps and their running sums in float32 (the CDF stays
                       float64): the float32 restatement that a float32 kernel is measured against.
"""
import functools

import numpy as np
import torch

from helpers.line_ot_cases import ROWS, rows

SIZES_CPU = [(1, 1), (2, 3), (48, 36), (130, 129), (100, 1), (257, 96)]
# one-atom sides; one atom per lane; mixed classes; dead lanes; one wave with 64 atoms per lane; and (1000, 513): the
# class of 16 atoms per lane, which no other size reaches and which asks for the most LDS (four waves, 130 KiB)
SIZES_GPU = [(1, 1), (100, 1), (4096, 1), (64, 64), (65, 64), (48, 36), (130, 129), (257, 96), (1000, 1536), (4096, 4095),
             (1000, 513)]
TIE_SIZES = [(48, 36), (65, 64), (257, 96)]
POWERS = [1, 2, 3, 1.5]
FLOOR = 1e-6


def _normalised_w(w, like, count, dtype):
    if w is None:
        w = torch.ones(count, dtype=dtype, device=like.device)
    w = w.to(dtype).expand(like.shape[:-1] + (count,))
    return w / w.sum(-1, keepdim=True)


def quantile_merge_w(u, v, p, a=None, b=None, dtype=torch.float64):
    """u (..., n), v (..., m), weights None / (n,) / (..., n) -> (...) in `dtype`; differentiable w.r.t. u, v, a and b."""
    u, v = u.to(dtype), v.to(dtype)
    n, m = u.shape[-1], v.shape[-1]
    a, b = _normalised_w(a, u, n, dtype), _normalised_w(b, v, m, dtype)
    us, iu = torch.sort(u, dim=-1, stable=True)
    vs, iv = torch.sort(v, dim=-1, stable=True)
    A = torch.cumsum(torch.gather(a, -1, iu), -1)
    B = torch.cumsum(torch.gather(b, -1, iv), -1)
    A = torch.cat([A[..., :-1], torch.ones_like(A[..., :1])], -1)
    B = torch.cat([B[..., :-1], torch.ones_like(B[..., :1])], -1)
    t = torch.sort(torch.cat([A, B], -1), dim=-1).values
    delta = torch.diff(t, dim=-1, prepend=torch.zeros_like(t[..., :1]))
    i = torch.searchsorted(A.detach().contiguous(), t.detach().contiguous(), right=False).clamp(max=n - 1)
    j = torch.searchsorted(B.detach().contiguous(), t.detach().contiguous(), right=False).clamp(max=m - 1)
    d = torch.gather(us, -1, i) - torch.gather(vs, -1, j)
    return (delta * d.abs() ** p).sum(-1)


def potentials_walk(u, v, p, a, b, cost_dtype=np.float64):
    """one row: u (n,), v (m,), raw weights a (n,), b (m,) -> (grad_a, grad_b, dual, c_last) in float64, where
    dual = sum abar f + sum bbar g (so dual + c_last = cost)"""
    u, v, a, b = [np.asarray(x, dtype=np.float64) for x in (u, v, a, b)]
    n, m = u.size, v.size
    iu, iv = np.argsort(u, kind="stable"), np.argsort(v, kind="stable")
    us, vs = u[iu].astype(cost_dtype), v[iv].astype(cost_dtype)
    Ta, Tb = a.sum(), b.sum()
    abar, bbar = a[iu] / Ta, b[iv] / Tb
    # (integer weights with equal totals: equal levels are equal doubles, k / T with the same T)
    A, B = np.cumsum(a[iu]) / Ta, np.cumsum(b[iv]) / Tb
    A[-1] = B[-1] = 1.0
    power = cost_dtype(p)

    def cost(i, j):
        return np.abs(us[i] - vs[j]) ** power

    i = j = 0
    phi, psi = np.zeros(n, dtype=cost_dtype), np.zeros(m, dtype=cost_dtype)
    c = cost(0, 0)
    while not (i == n - 1 and j == m - 1):
        if j == m - 1 or (i < n - 1 and A[i] <= B[j]):          # on equal levels the u end comes first
            nxt = cost(i + 1, j)
            phi[i] = c - nxt
            i += 1
        else:
            nxt = cost(i, j + 1)
            psi[j] = c - nxt
            j += 1
        c = nxt
    f = np.cumsum(phi[::-1], dtype=cost_dtype)[::-1].astype(np.float64)
    g = np.cumsum(psi[::-1], dtype=cost_dtype)[::-1].astype(np.float64)
    mean_f, mean_g = float((abar * f).sum()), float((bbar * g).sum())
    ga, gb = np.zeros(n), np.zeros(m)
    ga[iu] = (f - mean_f) / Ta
    gb[iv] = (g - mean_g) / Tb
    return ga, gb, mean_f + mean_g, float(c)


def walk_rows(u, v, p, a, b, cost_dtype=np.float64):
    """potentials_walk over the rows of u (R, n), v (R, m); weights (n,) / (R, n) -> two arrays (R, n), (R, m)"""
    u, v, a, b = [np.asarray(x, dtype=np.float64) for x in (u, v, a, b)]
    out = [potentials_walk(u[r], v[r], p, a if a.ndim == 1 else a[r], b if b.ndim == 1 else b[r], cost_dtype)[:2]
           for r in range(u.shape[0])]
    return np.stack([o[0] for o in out]), np.stack([o[1] for o in out])


def float_weights(n, m, seed, per_row, count=ROWS):
    g = torch.Generator().manual_seed(seed)
    shape = (count,) if per_row else ()
    return torch.rand(shape + (n,), generator=g) + 0.05, torch.rand(shape + (m,), generator=g) + 0.05


def tie_weights(n, m, seed, heavy=False):
    """integer weights (n,), (m,) as float64, drawn from 0..3 and topped up to equal totals (atoms of weight 0 stay at 0):
    exact ties between the two CDFs, and atoms of weight 0; `heavy`: one atom of v holds 90 % of its side's mass"""
    rng = np.random.default_rng(seed)
    ka, kb = rng.integers(0, 4, n), rng.integers(0, 4, m)
    ka[rng.integers(0, n)] += 1                                # neither side is empty
    kb[rng.integers(0, m)] += 1
    if heavy:
        kb[m // 3] += 9 * int(kb.sum() - kb[m // 3])
    diff = int(ka.sum() - kb.sum())                           # equal totals: top up atoms of the lighter side, zeros stay
    light = kb if diff > 0 else ka
    np.add.at(light, rng.choice(np.flatnonzero(light), abs(diff)), 1)
    assert ka.sum() == kb.sum()
    return ka.astype(np.float64), kb.astype(np.float64)


def autograd_weight_grads(u, v, p, a, b, dtype):
    """gradients of sum_rows quantile_merge_w w.r.t. a and b (float64 arrays of the weights' shapes)"""
    ar, br = a.clone().to(dtype).requires_grad_(), b.clone().to(dtype).requires_grad_()
    quantile_merge_w(u, v, p, ar, br, dtype=dtype).sum().backward()
    return ar.grad.double().numpy(), br.grad.double().numpy()


@functools.lru_cache(maxsize=None)
def row_case(n, m, p, per_row):
    """the shared case of the rows form: inputs, the float64 reference gradients and the bound per side -- 4 x the
    float32 restatement's own deviation from float64, floor 1e-6, on max |error| / max |entry|"""
    u, v = rows(n, m, seed=6000 + n + m)
    a, b = float_weights(n, m, 23, per_row)
    ref = autograd_weight_grads(u, v, p, a, b, torch.float64)
    f32 = autograd_weight_grads(u, v, p, a, b, torch.float32)
    bounds = tuple(max(4.0 * max_dev(f, r), FLOOR) for f, r in zip(f32, ref))
    return u, v, a, b, ref, bounds


def max_dev(got, ref):
    """max |error| / max |entry|; two all-zero arrays (a side of one atom) deviate by 0"""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    scale = np.abs(ref).max()
    err = np.abs(got - ref).max()
    return float(err / scale) if scale > 0 else float(err)
