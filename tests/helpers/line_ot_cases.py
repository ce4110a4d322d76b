"""References and inputs for the line-transport tests (test_line_ot_cpu.py, test_line_ot_gpu.py).

Two independent statements of W_p^p = int_0^1 |F_u^-1(t) - F_v^-1(t)|^p dt between weighted empirical measures:

    quantile_merge   torch, any dtype, differentiable w.r.t. the values: sort both sides, cumulative weights (last entry
                     forced to 1), merge the two sets of breakpoints, and on every merged interval (t_{k-1}, t_k] take the
                     atoms active there (first CDF end >= t_k, index clamped to n-1 / m-1).
    replication      numpy float64, integer weights k_i, k_j with equal totals: repeat every atom k times, sort, mean of
                     |U - V|^p.  Uniform n != m uses k = lcm/n and lcm/m.
"""
import math

import numpy as np
import torch

# (n, m): class edges of the 64 * {1, 2, 4, .., 64} size classes, mixed classes, one atom against many
SIZES = [(1, 1), (64, 64), (65, 64), (48, 36), (130, 129), (100, 1), (257, 96), (1000, 1536), (2048, 1536), (4096, 1),
         (4096, 4095)]
POWERS = [1, 2, 3, 1.5]
ROWS = 4


def _normalised(w, like, count, dtype):
    if w is None:
        w = torch.ones(count, dtype=dtype, device=like.device)
    w = w.detach().to(dtype)
    w = w.expand(like.shape[:-1] + (count,))
    return w / w.sum(-1, keepdim=True)


def quantile_merge(u, v, p, a=None, b=None, dtype=torch.float64):
    """u (..., n), v (..., m), weights None / (n,) / (..., n) -> (...) in `dtype`; differentiable w.r.t. u and v."""
    u, v = u.to(dtype), v.to(dtype)
    n, m = u.shape[-1], v.shape[-1]
    a, b = _normalised(a, u, n, dtype), _normalised(b, v, m, dtype)
    us, iu = torch.sort(u, dim=-1, stable=True)
    vs, iv = torch.sort(v, dim=-1, stable=True)
    A = torch.cumsum(torch.gather(a, -1, iu), -1)
    B = torch.cumsum(torch.gather(b, -1, iv), -1)
    A = torch.cat([A[..., :-1], torch.ones_like(A[..., :1])], -1)
    B = torch.cat([B[..., :-1], torch.ones_like(B[..., :1])], -1)
    t = torch.sort(torch.cat([A, B], -1), dim=-1).values
    delta = torch.diff(t, dim=-1, prepend=torch.zeros_like(t[..., :1]))
    i = torch.searchsorted(A.contiguous(), t.contiguous(), right=False).clamp(max=n - 1)
    j = torch.searchsorted(B.contiguous(), t.contiguous(), right=False).clamp(max=m - 1)
    d = torch.gather(us, -1, i) - torch.gather(vs, -1, j)
    return (delta * d.abs() ** p).sum(-1)


def replication(u, v, p, ku=None, kv=None):
    """u (n,), v (m,) numpy; integer weights ku, kv with equal totals (None, None: lcm/n and lcm/m) -> float64"""
    u, v = np.asarray(u, dtype=np.float64), np.asarray(v, dtype=np.float64)
    if ku is None and kv is None:
        lcm = math.lcm(u.size, v.size)
        ku, kv = np.full(u.size, lcm // u.size), np.full(v.size, lcm // v.size)
    ku, kv = np.asarray(ku, dtype=np.int64), np.asarray(kv, dtype=np.int64)
    assert ku.sum() == kv.sum()
    U, V = np.sort(np.repeat(u, ku)), np.sort(np.repeat(v, kv))
    return float(np.mean(np.abs(U - V) ** p))


def rows(n, m, seed, count=ROWS):
    """two float32 row blocks (count, n), (count, m); the second offset by 0.5 so that the cost is O(1)"""
    g = torch.Generator().manual_seed(seed)
    return torch.randn(count, n, generator=g), torch.randn(count, m, generator=g) + 0.5


def integer_weights(n, m, seed, heavy=False):
    """integer weights (n,), (m,) with equal totals; `heavy`: one atom of v holds 90 % of its mass"""
    rng = np.random.default_rng(seed)
    ku = rng.integers(1, 5, n)
    if heavy:
        kv = np.ones(m, dtype=np.int64)
        kv[m // 3] = 9 * (m - 1)                  # 90 % of the total 10 (m - 1)
    else:
        kv = rng.integers(1, 5, m)
    # equal totals: top up single atoms of the lighter side
    diff = int(ku.sum() - kv.sum())
    if diff > 0:
        np.add.at(kv, rng.integers(0, m, diff), 1)
    elif diff < 0:
        np.add.at(ku, rng.integers(0, n, -diff), 1)
    assert ku.sum() == kv.sum()
    return ku, kv


def rel_dev(got, ref):
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    return float(np.max(np.abs(got - ref) / np.abs(ref)))
