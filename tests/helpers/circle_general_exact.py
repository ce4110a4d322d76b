"""The definition of general circular OT (weights, n != m) on the CPU in double: min over the cut theta in [-1, 1] of
Cost(theta), the reference's quantile-merge integral.

Cost and its one-sided slopes are evaluated ONLY through `oracle.ref_mirror.cut_cost` / `cut_slopes` (code the kernels
share nothing with).  Cost is convex and piecewise linear in theta with kinks where a shifted target CDF level meets a
source CDF level, theta = v_cdf[j] - u_cdf[i] (mod 1), so the minimum sits on a kink.  Two minimisers:

  (a) `min_exhaustive`: Cost at every kink v_cdf[j] - u_cdf[i] + {-1, 0, 1} inside [-1, 1], the smallest wins
      (for n * m <= 3100);
  (b) `min_certificate`: bisection on the slope signs, then tangent intersection until Cost(t) exceeds the tangents'
      value at t -- a lower bound of the minimum over the bracket -- by no more than 1e-15 Cost, or the slopes at t
      straddle zero.

Gradients: autograd through `cut_cost` at the detached theta*, as the reference does (:207), composed with
`ref_mirror.circle_coords` at the sliced level.  p == 1 at the sliced level and emd1D_circle are
`ref_mirror.circular_w1_level_median`.
"""
import torch

from oracle import ref_mirror

EXHAUSTIVE_LIMIT = 3100
SLOPE_PROBE = 1e-9          # the one-sided slopes at theta* are read this far to either side of it
ISOLATED = 1e-6             # smaller slope / larger slope below this: the minimiser is not isolated


def sorted_cdfs(u, v, u_weights=None, v_weights=None, reverse_sum=False):
    """Rows u (R, n), v (R, m) -> sorted rows and CDFs as the reference builds them (:153-167).  reverse_sum: the CDFs
    as 1 - reversed cumsum of the same weights, a second summation order (for the rounding spread)."""
    R, n = u.shape
    m = v.shape[-1]
    wu = torch.full((n,), 1.0 / n, dtype=u.dtype) if u_weights is None else u_weights
    wv = torch.full((m,), 1.0 / m, dtype=u.dtype) if v_weights is None else v_weights
    us, iu = torch.sort(u, -1)
    vs, iv = torch.sort(v, -1)
    gu, gv = wu[..., iu].expand(R, n), wv[..., iv].expand(R, m)
    if reverse_sum:
        def back(g):
            tail = torch.flip(torch.cumsum(torch.flip(g, (-1,)), -1), (-1,))          # sum of the weights from i on
            return torch.cat([(1.0 - tail)[:, 1:], torch.ones_like(g[:, :1])], -1)
        return us, vs, back(gu), back(gv)
    return us, vs, torch.cumsum(gu, -1), torch.cumsum(gv, -1)


def _cost(theta, us, vs, cu, cv, p):
    return ref_mirror.cut_cost(theta, us, vs, cu, cv, p)


def min_exhaustive(us, vs, cu, cv, p):
    """Rows -> (minimum (R,), theta* (R,)): Cost at every kink inside [-1, 1]."""
    R, n = us.shape
    m = vs.shape[-1]
    assert n * m <= EXHAUSTIVE_LIMIT
    with torch.no_grad():
        base = (cv.unsqueeze(1) - cu.unsqueeze(2)).reshape(R, n * m)
        kinks = torch.cat([base - 1, base, base + 1, torch.full_like(base[:, :1], -1.0), torch.full_like(base[:, :1], 1.0)], -1)
        kinks = kinks.clamp(-1.0, 1.0)
        K = kinks.shape[1]
        rep = lambda a: a.unsqueeze(1).expand(R, K, a.shape[-1]).reshape(R * K, a.shape[-1])
        cost = _cost(kinks.reshape(R * K, 1), rep(us), rep(vs), rep(cu), rep(cv), p).reshape(R, K)
        best, at = cost.min(-1)
        return best, torch.gather(kinks, 1, at.unsqueeze(1)).squeeze(1)


def min_certificate(us, vs, cu, cv, p, bisections=6, max_rounds=200, rounds_out=None):
    """Rows -> (minimum (R,), theta* (R,)) by the certificate search; every row is followed until its own stop."""
    R = us.shape[0]
    args = (us, vs, cu, cv, p)
    with torch.no_grad():
        lo = torch.full((R, 1), -1.0, dtype=us.dtype)
        hi = torch.full((R, 1), 1.0, dtype=us.dtype)
        c_lo, c_hi = _cost(lo, *args).reshape(R, 1), _cost(hi, *args).reshape(R, 1)
        dp_lo, _ = ref_mirror.cut_slopes(lo, *args)
        _, dm_hi = ref_mirror.cut_slopes(hi, *args)
        best = torch.minimum(c_lo, c_hi)
        best_t = torch.where(c_hi < c_lo, hi, lo)
        active = (dp_lo < 0) & (dm_hi > 0)
        rounds = 0
        while bool(active.any()) and rounds < max_rounds:
            t = (lo + hi) / 2
            if rounds >= bisections:
                cross = (c_hi - c_lo + lo * dp_lo - hi * dm_hi) / (dp_lo - dm_hi)
                t = torch.where((cross > lo) & (cross < hi), cross, t)
            active = active & (t > lo) & (t < hi)
            c = _cost(t, *args).reshape(R, 1)
            dp, dm = ref_mirror.cut_slopes(t, *args)
            better = active & (c < best)
            best = torch.where(better, c, best)
            best_t = torch.where(better, t, best_t)
            done = (dp * dm) <= 0
            if rounds >= bisections:
                done = done | ((c - (c_lo + dp_lo * (t - lo))) <= 1e-15 * c)
            active = active & ~done
            right = active & (dp < 0)
            left = active & ~(dp < 0)
            lo, c_lo, dp_lo = torch.where(right, t, lo), torch.where(right, c, c_lo), torch.where(right, dp, dp_lo)
            hi, c_hi, dm_hi = torch.where(left, t, hi), torch.where(left, c, c_hi), torch.where(left, dm, dm_hi)
            rounds += 1
        assert not bool(active.any()), "certificate search did not stop"
        if rounds_out is not None:
            rounds_out.append(rounds)
        return best.squeeze(1), best_t.squeeze(1)


def minimise(us, vs, cu, cv, p):
    if us.shape[-1] * vs.shape[-1] <= EXHAUSTIVE_LIMIT:
        return min_exhaustive(us, vs, cu, cv, p)
    return min_certificate(us, vs, cu, cv, p)


def isolated(theta, us, vs, cu, cv, p):
    """(R,) bool: the slope of the piece left of theta* and of the piece right of it are both away from zero."""
    with torch.no_grad():
        t = theta.reshape(-1, 1)
        left, _ = ref_mirror.cut_slopes(t - SLOPE_PROBE, us, vs, cu, cv, p)
        _, right = ref_mirror.cut_slopes(t + SLOPE_PROBE, us, vs, cu, cv, p)
        a, b = left.abs().squeeze(1), right.abs().squeeze(1)
        small, large = torch.minimum(a, b), torch.maximum(a, b)
        return (large > 0) & (small >= ISOLATED * large)


def circle_min(u, v, p, u_weights=None, v_weights=None):
    """Rows of circle coordinates -> (cost (R,) attached to u and v through the final Cost evaluation, theta* (R,),
    isolated (R,)): the definition of binary_search_circle."""
    us, vs, cu, cv = sorted_cdfs(u, v, u_weights, v_weights)
    _, theta = minimise(us.detach(), vs.detach(), cu, cv, p)
    cost = _cost(theta.reshape(-1, 1), us, vs, cu, cv, p)
    return cost, theta, isolated(theta, us.detach(), vs.detach(), cu, cv, p)


def circle_level_median(u, v, u_weights=None, v_weights=None):
    return ref_mirror.circular_w1_level_median(u, v, u_weights, v_weights)


def slice_costs(Xs, Xt, Us, p, u_weights=None, v_weights=None):
    """One pair: Xs (n, 3), Xt (m, 3), Us (L, 3, 2) -> (per-slice costs (L,) attached to the clouds, isolated (L,))."""
    cs, ct = ref_mirror.circle_coords(Xs, Us), ref_mirror.circle_coords(Xt, Us)
    if p == 1:
        return circle_level_median(cs, ct, u_weights, v_weights), torch.ones(cs.shape[0], dtype=torch.bool)
    cost, _, iso = circle_min(cs, ct, p, u_weights, v_weights)
    return cost, iso


def batch_slice_costs(Xs, Xt, Us, p, u_weights=None, v_weights=None):
    """Batched: Xs (B, n, 3), Xt (B, m, 3), Us (L, 3, 2) or (B, L, 3, 2), weights shared or per pair ->
    (costs (B, L), isolated (B, L))."""
    costs, isos = [], []
    for b in range(Xs.shape[0]):
        U = Us if Us.dim() == 3 else Us[b]
        wu = None if u_weights is None else (u_weights if u_weights.dim() == 1 else u_weights[b])
        wv = None if v_weights is None else (v_weights if v_weights.dim() == 1 else v_weights[b])
        c, i = slice_costs(Xs[b], Xt[b], U, p, wu, wv)
        costs.append(c)
        isos.append(i)
    return torch.stack(costs), torch.stack(isos)


def rounding_spread(u, v, p, u_weights=None, v_weights=None):
    """Worst |value with CDFs from a forward cumsum - value with CDFs from 1 - reversed cumsum| over the rows: two
    summation orders of the same weights (rows of circle coordinates; p == 1 means the bisection form here)."""
    with torch.no_grad():
        a = sorted_cdfs(u, v, u_weights, v_weights)
        b = sorted_cdfs(u, v, u_weights, v_weights, reverse_sum=True)
        return float((minimise(*a, p)[0] - minimise(*b, p)[0]).abs().max())
