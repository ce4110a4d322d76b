"""References and inputs for the tests of the circle's gradients with respect to the weights
(test_circle_weight_grad_cpu.py, test_circle_weight_grad_gpu.py).

W(a, b) = min over the cut of Cost(cut; a, b) (oracle.ref_mirror.cut_cost).  Stated here, per row, in numpy:

    bisect_with_cut    the bisection of oracle.ref_mirror.circular_ot_bisect, step for step, returning the cut as well
    fixed_cut          the derivative of Cost at a FIXED cut: suffix sums of the jumps of the cost at the CDF ends, and the
                       slope in the cut, under one tie rule (source level first / target level first)
    closed_form        the gradient of W: the level pair (r, j) closest together at the cut, the side the comparisons put
                       it on, the slope s there, and  dW/da_i = ga_i - s [i <= r],  dW/db_k = gb_k + s [k <= j]
    lambda_mix         the same gradient as  lambda G+ + (1 - lambda) G-  of the fixed-cut derivatives at cut + eta under
                       the target-first rule and at cut - eta under the source-first rule (what the kernel computes)
    brute_min          the exact minimum over all n m kinks, for central differences
    level_median_grads autograd through oracle.ref_mirror.circular_w1_level_median

Every gradient is returned at the original indices and centred per side (sum_i a_i G_i = 0).  `dtype=np.float32` runs the
same code with float32 CDFs, costs and sums: the float32 restatement a float32 kernel is measured against.
"""
import functools

import numpy as np
import torch

from oracle import ref_mirror

ROWS = 3
FLOOR = 1e-6
POWERS = [1, 2, 3, 1.5]
SIZES_CPU = [(5, 7), (6, 6), (9, 4), (12, 12), (33, 20)]
POWERS_CPU = [1, 1.5, 2, 3]
# one-atom sides; few large kinks (the closing term decides); class edges and dead lanes; two waves' worth; four
SIZES_GPU = [(1, 1), (100, 1), (4096, 1), (5, 7), (64, 64), (65, 64), (48, 36), (130, 129), (257, 96), (513, 300),
             (1000, 1536), (4096, 4095)]
ETA = 3e-7          # the kernel's half-width around the cut (csrc/shw_ssw_weights.hip kEta)


def coords(n, m, seed, rows=ROWS):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(rows, n, generator=g), torch.rand(rows, m, generator=g)


def float_weights(n, m, seed, per_row, rows=ROWS):
    """rand + 0.2, normalised in float32 (what a caller passes)"""
    g = torch.Generator().manual_seed(seed)
    shape = (rows,) if per_row else ()
    a, b = torch.rand(shape + (n,), generator=g) + 0.2, torch.rand(shape + (m,), generator=g) + 0.2
    return a / a.sum(-1, keepdim=True), b / b.sum(-1, keepdim=True)


def dyadic_weights(n, m, seed, total=64, heavy=False):
    """integer weights over a power-of-two total (exact in float32, so equal levels are equal floats): zeros included,
    `heavy`: one atom of v holds 58 of the 64 units (about 90 %)"""
    rng = np.random.default_rng(seed)

    def draw(count, big):
        k = np.zeros(count, dtype=np.int64)
        left = total
        if big:
            k[count // 3] = (total * 29) // 32
            left -= k[count // 3]
        np.add.at(k, rng.integers(0, count, left), 1)
        return k
    ka, kb = draw(n, False), draw(m, heavy)
    return (ka / total).astype(np.float32), (kb / total).astype(np.float32)


def _pow(x, p, dt):
    return np.abs(x).astype(dt) ** dt(p)


def prepare(u, v, a, b, dtype=np.float64):
    """one row: sorted values, sort maps, sorted weights and CDFs in `dtype` (running sums in `dtype`)"""
    u, v, a, b = [np.asarray(x, dtype=np.float64) for x in (u, v, a, b)]
    iu, iv = np.argsort(u, kind="stable"), np.argsort(v, kind="stable")
    asort, bsort = a[iu].astype(dtype), b[iv].astype(dtype)
    return dict(us=u[iu].astype(dtype), vs=v[iv].astype(dtype), iu=iu, iv=iv, a=asort, b=bsort,
                A=np.cumsum(asort, dtype=dtype), B=np.cumsum(bsort, dtype=dtype))


def bisect_with_cut(u, v, a, b, p, dtype=torch.float64):
    """rows u (R,n), v (R,m), weights (n,) / (m,) -> (cost (R,), cut (R,)): oracle.ref_mirror.circular_ot_bisect with the
    cut returned"""
    u, v, a, b = [torch.as_tensor(x).to(dtype) for x in (u, v, a, b)]
    R = u.shape[0]
    us, iu = torch.sort(u, -1)
    vs, iv = torch.sort(v, -1)
    args = (us, vs, torch.cumsum(a[..., iu], -1), torch.cumsum(b[..., iv], -1), p)
    t_lo = torch.full((R, 1), -1.0, dtype=dtype)
    t_hi = torch.full((R, 1), 1.0, dtype=dtype)
    t_mid = (t_lo + t_hi) / 2
    while True:
        dp, dm = ref_mirror.cut_slopes(t_mid, *args)
        settled = (dp * dm) <= 0
        if bool(settled.all()):
            break
        tiny = ((t_hi - t_lo) < 1e-7) & ~settled
        if bool(tiny.any()):
            dp_lo, _ = ref_mirror.cut_slopes(t_lo, *args)
            _, dm_hi = ref_mirror.cut_slopes(t_hi, *args)
            c_lo = ref_mirror.cut_cost(t_lo, *args).reshape(-1, 1)
            c_hi = ref_mirror.cut_cost(t_hi, *args).reshape(-1, 1)
            usable = tiny & ((dp_lo - dm_hi).abs() > 1e-3)
            crossing = (c_hi - c_lo + t_lo * dp_lo - t_hi * dm_hi) / (dp_lo - dm_hi)
            t_mid = torch.where(usable, crossing, t_mid)
            break
        go_right = dp < 0
        t_lo = torch.where(go_right, t_mid, t_lo)
        t_hi = torch.where(~go_right, t_mid, t_hi)
        t_mid = torch.where(settled, t_mid, (t_lo + t_hi) / 2)
    return ref_mirror.cut_cost(t_mid, *args), t_mid[:, 0]


def fixed_cut(S, theta, p, target_first):
    """derivatives of Cost at the cut `theta` w.r.t. the sorted weights (suffix sums of the jumps), the slope in the cut,
    and the rotated levels by sorted target index.  Ties: source level first, or target level first."""
    dt = S["us"].dtype.type
    us, vs, A, B = S["us"], S["vs"], S["A"].copy(), S["B"]
    n, m = us.size, vs.size
    A[-1] = 1                                                   # the last level is 1 whatever its running sum says
    theta = dt(theta)
    turns = np.floor(theta)
    sh = B - (theta - turns)
    wrapped = sh < 0
    C = np.where(wrapped, sh + dt(1), sh)
    pos = vs + (turns + wrapped.astype(dt))
    start = int(wrapped.sum()) % m
    order = (np.arange(m) + start) % m
    pos_rot = np.concatenate([pos[order], pos[order[:1]] + dt(1)])
    rho = np.searchsorted(C[order], A[:-1], side="right" if target_first else "left")
    y = pos_rot[rho]
    ja = np.zeros(n, dtype=dt)
    ja[:-1] = _pow(us[:-1] - y, p, dt) - _pow(us[1:] - y, p, dt)
    i = np.minimum(np.searchsorted(A, C, side="left" if target_first else "right"), n - 1)
    nxt = (np.arange(m) + 1) % m
    posn = pos[nxt] + (nxt == start).astype(dt)
    jb = _pow(us[i] - pos, p, dt) - _pow(us[i] - posn, p, dt)
    ga = np.cumsum(ja[::-1], dtype=dt)[::-1]
    gb = np.cumsum(jb[::-1], dtype=dt)[::-1]
    return ga.astype(np.float64), gb.astype(np.float64), float(-jb.sum(dtype=dt)), C.astype(np.float64)


def _centred(S, ga, gb):
    """sorted-order gradients -> original indices, centred against the (normalised) weights"""
    a, b = S["a"].astype(np.float64), S["b"].astype(np.float64)
    out_a, out_b = np.zeros(a.size), np.zeros(b.size)
    out_a[S["iu"]] = ga - (a * ga).sum() / a.sum()
    out_b[S["iv"]] = gb - (b * gb).sum() / b.sum()
    return out_a, out_b


def closed_form(S, theta, p):
    """the gradient of W at the minimising cut: nearest level pair, its side, the slope there, the closing term"""
    ga, gb, s, C = fixed_cut(S, theta, p, target_first=False)   # (no exact ties at a generic cut: either rule)
    A = S["A"].astype(np.float64).copy()
    A[-1] = 1.0
    n, m = A.size, C.size
    by_level = np.argsort(C, kind="stable")                     # every source level against its two neighbours
    at = np.searchsorted(C[by_level], A)
    cand = np.stack([by_level[(at - 1) % m], by_level[at % m]], 1)
    diff = C[cand] - A[:, None]
    diff -= np.round(diff)                                      # levels live on a circle: 1 is 0
    r, c = np.unravel_index(np.argmin(np.abs(diff)), diff.shape)
    j = cand[r, c]
    ga = ga - s * (np.arange(n) <= r)
    gb = gb + s * (np.arange(m) <= j)
    return _centred(S, ga, gb)


def lambda_mix(S, theta, p, eta=ETA):
    lo = fixed_cut(S, theta - eta, p, target_first=False)
    hi = fixed_cut(S, theta + eta, p, target_first=True)
    s_lo, s_hi = lo[2], hi[2]
    if s_lo == 0 and s_hi == 0:
        lam = 0.5
    elif s_lo >= 0:
        lam = 0.0
    elif s_hi <= 0:
        lam = 1.0
    else:
        lam = -s_lo / (s_hi - s_lo)
    return _centred(S, lo[0] + lam * (hi[0] - lo[0]), lo[1] + lam * (hi[1] - lo[1]))


def brute_min(u, v, a, b, p):
    """one row, float64: the minimum of Cost over all n m kinks cut = B_j - A_r (and one turn either way: Cost is not
    periodic in the cut, a whole turn moves every target atom by 1) in [-1, 1], and the minimising cut"""
    S = prepare(u, v, a, b)
    base = (S["B"][None, :] - S["A"][:, None]).ravel()
    kinks = np.concatenate([base - 1.0, base, base + 1.0])
    kinks = kinks[np.abs(kinks) <= 1.0]
    t = torch.from_numpy(kinks).unsqueeze(1)
    rep = lambda x: torch.from_numpy(x).unsqueeze(0).expand(kinks.size, -1).contiguous()
    costs = ref_mirror.cut_cost(t, rep(S["us"]), rep(S["vs"]), rep(S["A"]), rep(S["B"]), p)
    k = int(torch.argmin(costs))
    return float(costs[k]), float(kinks[k])


def weight_grad_rows(u, v, a, b, p, dtype=np.float64, form="closed"):
    """rows u (R,n), v (R,m), weights (n,) / (R,n): the gradient rows of the bisection's value -> (R,n), (R,m)"""
    u, v, a, b = [np.asarray(x) for x in (u, v, a, b)]
    tdt = torch.float64 if dtype == np.float64 else torch.float32
    ga, gb = [], []
    for r in range(u.shape[0]):
        ar, br = (a if a.ndim == 1 else a[r]), (b if b.ndim == 1 else b[r])
        _, cut = bisect_with_cut(u[r:r + 1], v[r:r + 1], ar, br, p, tdt)
        S = prepare(u[r], v[r], ar, br, dtype)
        g = (closed_form if form == "closed" else lambda_mix)(S, float(cut[0]), p)
        ga.append(g[0])
        gb.append(g[1])
    return np.stack(ga), np.stack(gb)


def level_median_grads(u, v, a, b, dtype=torch.float64):
    """autograd through the level-median formula, rows as weight_grad_rows, centred per side"""
    u, v, a, b = [torch.as_tensor(np.asarray(x)) for x in (u, v, a, b)]
    ga, gb = [], []
    for r in range(u.shape[0]):
        ar = (a if a.dim() == 1 else a[r]).to(dtype).clone().requires_grad_()
        br = (b if b.dim() == 1 else b[r]).to(dtype).clone().requires_grad_()
        ref_mirror.circular_w1_level_median(u[r:r + 1].to(dtype), v[r:r + 1].to(dtype), ar, br).sum().backward()
        an, bn = ar.detach().double(), br.detach().double()
        ga.append((ar.grad.double() - (an * ar.grad.double()).sum() / an.sum()).numpy())
        gb.append((br.grad.double() - (bn * br.grad.double()).sum() / bn.sum()).numpy())
    return np.stack(ga), np.stack(gb)


def max_dev(got, ref):
    """max |error| / max |entry|; two all-zero arrays (a side of one atom) deviate by 0"""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    scale = np.abs(ref).max()
    err = np.abs(got - ref).max()
    return float(err / scale) if scale > 0 else float(err)


def dense(n, m):
    """The size class in which the rule "4 x the float32 restatement's deviation on the same inputs" cannot hold for the
    cut search: the n m kinks of cut -> Cost lie closer together (under 1e-6) than a float32 running sum of the weights
    resolves its levels.  A float32 computation then minimises over slightly different kinks and ends on a NEIGHBOUR of
    the float64 minimiser: the gradient of a neighbouring piece.  Whether that happens on given inputs is chance -- the
    restatement's own deviation at (1000, 1536) is 4e-7 on one seed and 1e-3 on the next -- so a bound taken from one
    draw says nothing about another float32 computation on that draw."""
    return n * m > (1 << 20)


@functools.lru_cache(maxsize=None)
def dense_class_bound(n, m, p, per_row, seeds=4):
    """the bound of a dense class: 4 x the float32 restatement's WORST deviation from float64 over `seeds` draws of the
    inputs (the first one is row_case's own), floor 1e-6, per side"""
    worst = [0.0, 0.0]
    for k in range(seeds):
        u, v = coords(n, m, seed=9000 + n + m + 1000 * k)
        a, b = float_weights(n, m, 31 + 1000 * k, per_row)
        ref = weight_grad_rows(u.numpy(), v.numpy(), a.numpy(), b.numpy(), p)
        f32 = weight_grad_rows(u.numpy(), v.numpy(), a.numpy(), b.numpy(), p, np.float32)
        if not per_row:
            ref, f32 = tuple(r.sum(0) for r in ref), tuple(f.sum(0) for f in f32)
        worst = [max(w, max_dev(f, r)) for w, f, r in zip(worst, f32, ref)]
    return tuple(max(4.0 * w, FLOOR) for w in worst)


@functools.lru_cache(maxsize=None)
def row_case(n, m, p, per_row, median=False):
    """the shared case of the circle level: inputs, the float64 reference for the gradient of the SUM of the rows' costs
    and the bound per side -- 4 x the float32 restatement's own deviation from float64, floor 1e-6, on
    max |error| / max |entry|"""
    u, v = coords(n, m, seed=9000 + n + m)
    a, b = float_weights(n, m, 31, per_row)
    if median:
        ref = level_median_grads(u, v, a, b)
        f32 = level_median_grads(u, v, a, b, torch.float32)
    else:
        ref = weight_grad_rows(u.numpy(), v.numpy(), a.numpy(), b.numpy(), p)
        f32 = weight_grad_rows(u.numpy(), v.numpy(), a.numpy(), b.numpy(), p, np.float32)
    if not per_row:                                             # shared weights receive the sum over the rows
        ref, f32 = tuple(r.sum(0) for r in ref), tuple(f.sum(0) for f in f32)
    bounds = tuple(max(4.0 * max_dev(f, r), FLOOR) for f, r in zip(f32, ref))
    if dense(n, m) and not median:
        bounds = dense_class_bound(n, m, p, per_row)
    return u, v, a, b, ref, bounds
