"""Cases, a NumPy restatement of the auction rule of csrc/shw_emd.hip, and the independent exact optimum
(scipy.optimize.linear_sum_assignment, float64) shared by tests/test_emd_cpu.py and tests/test_emd_gpu.py.

The rule restated ("Exact W for equal-size clouds"):
  * costs C(i, j) evaluated in float32, K = a power of two above the largest possible cost (bounding boxes for the
    L_p^p cost, pi^p for the angle cost), integer costs c = floor(C 2^s) with 2^s K = 2^26;
  * Jacobi rounds: every unassigned source bids for the target of least c + price (ties: lowest target), raising its
    price by (second least - least) + eps; a target takes its highest bid (ties: lowest bidder);
  * eps = 2^24, 2^21, ..., 1 (9 phases); prices are kept from phase to phase, the assignment starts empty in each.

How the value bound is set.  eps-complementary slackness at eps = 1 puts the integer cost of the returned permutation
within n of the integer optimum, and flooring loses less than 1 per entry: the mean of C along it is within
2^(1-s) = K 2^-25 of the optimum OF THE FLOAT32 COSTS.  The float64 optimum differs from that by the float32
evaluation error of a mean of n costs, which is measured, not guessed: g = |mean32 - mean64| of one and the same
assignment (the one under test), both evaluated with NumPy, and the allowance is max(16 g, FLOOR K),
FLOOR = 4 * 2^-24 -- 16 as everywhere in this suite (the kernel uses FMAs and the hardware atan2 / pow where NumPy
rounds each operation), a few float32 ulps of K where the two evaluations agree exactly.

How the bound on the returned cost is set (the float32 `cost` output against the float64 mean along the returned
assignment): max(16 g_abs, 16 * 2^-24 * mean), g_abs = mean_i |C32_i - C64_i| the per-couple float32 evaluation error
of NumPy along that assignment (no cancellation between couples, unlike g), the relative floor for the kernel's
summation: at most 4 sequential + 6 butterfly + 8 sequential roundings and one division."""
import functools

import numpy as np

FRAC_BITS = 26
EPS_FIRST = 1 << 24
EPS_DIV = 8
LIMIT = 2048                      # shw_max_points_emd()
GAP_K = 16
GAP_FLOOR = 4 * 2.0 ** -24


def round_cap(n):
    """shw_emd.hip emd_round_cap: a pair that needs more rounds than this is given up (cost NaN)"""
    return 1024 * n + 4096


# ------------------------------------------------------------------------------------------------------------ costs
def costs(a, b, kind, p, dtype=np.float64):
    """C of broadcastable arrays of points (..., 3): kind "lp" sum_d |a_d - b_d|^p, kind "geodesic" angle(a, b)^p
    with atan2(|a cross b|, a . b) and pi / 2 for a zero-length point"""
    a = np.asarray(a, dtype=dtype)
    b = np.asarray(b, dtype=dtype)
    p = dtype(p)
    if kind == "lp":
        d = np.abs(a - b)
        if p == 2:
            d = d * d
        elif p != 1:
            d = d ** p
        return (d[..., 0] + d[..., 1]) + d[..., 2]
    cx = a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1]
    cy = a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2]
    cz = a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]
    cross = np.sqrt((cx * cx + cy * cy) + cz * cz)
    dot = (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]
    theta = np.arctan2(cross, dot).astype(dtype)
    zero = ((a * a).sum(-1) == 0) | ((b * b).sum(-1) == 0)
    theta = np.where(zero, dtype(np.pi / 2), theta)
    if p == 1:
        return theta
    return theta * theta if p == 2 else theta ** p


def cost_matrix(x, y, kind, p, dtype=np.float64):
    """C (n, n) of two clouds (n, 3)"""
    return costs(np.asarray(x)[:, None, :], np.asarray(y)[None, :, :], kind, p, dtype)


def cost_bound(x, y, kind, p):
    """K of the kernel: 0 when every cost is 0, else the power of two 2^e with 1.001 B <= 2^e, B the float32 bound"""
    f = np.float32
    x, y = np.asarray(x, dtype=f), np.asarray(y, dtype=f)
    if kind == "lp":
        span = np.maximum(x.max(0) - y.min(0), y.max(0) - x.min(0))
        t = span * span if p == 2 else (span if p == 1 else span ** f(p))
        B = f((t[0] + t[1]) + t[2])
    else:
        B = f(np.pi) if p == 1 else f(np.pi) ** f(p)
    if not B > 0:
        return 0.0
    _, e = np.frexp(f(B * f(1.001)))
    return float(2.0 ** max(int(e), -100))


def integer_costs(x, y, kind, p):
    """(c (n, n) int64, K): what the kernel's cost function returns, from float32 costs"""
    K = cost_bound(x, y, kind, p)
    C = cost_matrix(x, y, kind, p, np.float32)
    if K == 0:
        return np.zeros(C.shape, dtype=np.int64), K
    scale = np.float32(2.0 ** FRAC_BITS / K)
    return np.clip(np.floor(C * scale), 0, 2.0 ** FRAC_BITS).astype(np.int64), K


# ------------------------------------------------------------------------------------------------------ restatement
def auction(c):
    """The rule on integer costs c (n, n).  Returns (assign (n,) target of each source, rounds, bids) or
    (None, cap, bids) when the round cap is reached."""
    n = c.shape[0]
    cap = round_cap(n)
    price = np.zeros(n, dtype=np.int64)
    rounds = bids = 0
    eps = EPS_FIRST
    while True:
        owner = np.full(n, -1, dtype=np.int64)
        free = np.arange(n)
        while free.size:
            if rounds == cap:
                return None, cap, bids
            rounds += 1
            bids += free.size
            w = c[free] + price[None, :]
            rows = np.arange(free.size)
            best = w.argmin(1)                                   # first minimum: the lowest target among equals
            w1 = w[rows, best]
            w[rows, best] = np.iinfo(np.int64).max
            w2 = w.min(1) if n > 1 else w1
            offer = price[best] + (w2 - w1) + eps
            order = np.lexsort((free, -offer, best))            # by target, then highest offer, then lowest bidder
            first = np.ones(free.size, dtype=bool)
            first[1:] = best[order][1:] != best[order][:-1]
            win = order[first]
            tgt, src = best[win], free[win]
            old = owner[tgt]
            price[tgt] = offer[win]
            owner[tgt] = src
            lost = np.ones(free.size, dtype=bool)
            lost[win] = False
            free = np.sort(np.concatenate([free[lost], old[old >= 0]]))
        if eps == 1:
            break
        eps //= EPS_DIV
    assign = np.empty(n, dtype=np.int64)
    assign[owner] = np.arange(n)
    return assign, rounds, bids


def mean_along(x, y, kind, p, assign, dtype=np.float64):
    """mean_i C(i, assign[i]) evaluated in dtype"""
    c = costs(x, np.asarray(y)[np.asarray(assign)], kind, p, dtype)
    return float(c.mean(dtype=dtype))


def eval_gap(x, y, kind, p, assign):
    """g of the module docstring: |mean32 - mean64| along one assignment"""
    return abs(mean_along(x, y, kind, p, assign, np.float32) - mean_along(x, y, kind, p, assign, np.float64))


def cost_bound_along(x, y, kind, p, assign):
    """allowance on |returned cost - float64 mean along the returned assignment| (module docstring)"""
    ya = np.asarray(y)[np.asarray(assign)]
    c64 = costs(x, ya, kind, p, np.float64)
    g_abs = float(np.abs(costs(x, ya, kind, p, np.float32).astype(np.float64) - c64).mean())
    return max(GAP_K * g_abs, 16 * 2.0 ** -24 * float(c64.mean()))


def of_largest(a, b):
    """max |a - b| in units of the largest |b|"""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300))


GRAD_FLOOR = 8 * 2.0 ** -24          # as tests/helpers/sinkhorn_chamfer_cases.py: where the two torch runs agree exactly
GRAD_CEILING = 1e-4                  # as the Chamfer gradient test


def grad_bound(g):
    return min(max(GAP_K * g, GRAD_FLOOR), GRAD_CEILING)


def value_bound(K, g):
    """allowance on (mean cost along the returned permutation) - (float64 optimum): the solver's K 2^-25 plus the
    float32 evaluation term max(16 g, FLOOR K) (module docstring)"""
    return K * 2.0 ** -25 + max(GAP_K * g, GAP_FLOOR * K)


# ------------------------------------------------------------------------------------------------------------ clouds
def _rng(*key):
    return np.random.default_rng([20260, *key])


def _sphere(rng, n):
    v = rng.standard_normal((n, 3))
    return (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(np.float32)


def _rotation(rng):
    q, r = np.linalg.qr(rng.standard_normal((3, 3)))
    q = q * np.sign(np.diag(r))
    if np.linalg.det(q) < 0:
        q[:, 0] = -q[:, 0]
    return q


def build(cloud, n, seed=0):
    """(x, y, extra) float32 clouds (n, 3); extra holds what a case-specific assertion needs"""
    rng = _rng(n, seed, sum(map(ord, cloud)))
    extra = {}
    if cloud == "sphere":
        x, y = _sphere(rng, n), _sphere(rng, n)
    elif cloud == "registration":                     # the trainers' situation: a rotated, noisy copy
        x = _sphere(rng, n)
        y = x.astype(np.float64) @ _rotation(rng).T + 0.02 * rng.standard_normal((n, 3))
        y = (y / np.linalg.norm(y, axis=1, keepdims=True)).astype(np.float32)
    elif cloud == "permuted":                         # y is x reordered: cost exactly 0, one optimal assignment
        x = _sphere(rng, n)
        perm = rng.permutation(n)
        y = x[perm].copy()                            # y[j] = x[perm[j]]: source perm[j] goes to target j
        extra["inverse"] = np.argsort(perm)           # assign[i] = the j with perm[j] = i
    elif cloud == "lattice":                          # 8 x 8 x k lattice against itself shifted by one cell: ties
        k = n // 64
        assert 64 * k == n
        g = np.stack(np.meshgrid(np.arange(8), np.arange(8), np.arange(k), indexing="ij"), -1).reshape(-1, 3)
        x = (g / 8.0).astype(np.float32)
        y = x + np.array([0.125, 0, 0], dtype=np.float32)
    elif cloud == "clusters":                         # 16 points, each repeated n / 16 times, in both clouds
        cx, cy = _sphere(rng, 16), _sphere(rng, 16)
        x, y = np.repeat(cx, n // 16, axis=0), np.repeat(cy, n // 16, axis=0)
        assert x.shape[0] == n
    elif cloud == "zeros":
        x, y = np.zeros((n, 3), np.float32), np.zeros((n, 3), np.float32)
    elif cloud in ("times1000", "times0.001", "plus100"):
        x, y = _sphere(rng, n), _sphere(rng, n)
        if cloud == "plus100":
            x, y = x + np.float32(100), y + np.float32(100)
        else:
            s = np.float32(1000 if cloud == "times1000" else 1e-3)
            x, y = x * s, y * s
    elif cloud == "cube":                             # the notebooks' shape: points on the surface of [-1, 1]^3
        def surface():
            pts = rng.uniform(-1, 1, (n, 3))
            face = rng.integers(0, 6, n)
            pts[np.arange(n), face % 3] = np.where(face < 3, -1.0, 1.0)
            return pts.astype(np.float32)
        x, y = surface(), (0.5 * _sphere(rng, n)).astype(np.float32)
    else:
        raise ValueError(cloud)
    return np.ascontiguousarray(x), np.ascontiguousarray(y), extra


# (cloud, n, kind, p)
CASES = (
    [("sphere", n, "lp", 2.0) for n in (1, 2, 63, 64, 65, 257, 1000, LIMIT)]
    + [("sphere", 63, "lp", 3.0), ("sphere", 65, "lp", 1.0), ("sphere", 257, "lp", 1.0), ("sphere", 257, "lp", 3.0),
       ("sphere", 2, "geodesic", 1.0), ("sphere", 65, "geodesic", 2.0), ("sphere", 257, "geodesic", 1.0),
       ("registration", 257, "lp", 2.0), ("registration", LIMIT, "lp", 2.0), ("registration", 1000, "geodesic", 2.0),
       ("registration", 257, "geodesic", 1.0),
       ("permuted", 65, "lp", 2.0), ("permuted", 1000, "lp", 2.0), ("permuted", 257, "geodesic", 1.0),
       ("lattice", 64, "lp", 2.0), ("lattice", 256, "lp", 1.0), ("lattice", 256, "geodesic", 2.0),
       ("clusters", 512, "lp", 2.0), ("clusters", 512, "geodesic", 1.0),
       ("zeros", 64, "lp", 2.0), ("zeros", LIMIT, "lp", 1.0), ("zeros", 64, "geodesic", 2.0),
       ("times1000", 257, "lp", 2.0), ("times0.001", 257, "lp", 3.0), ("plus100", 257, "lp", 1.0),
       ("plus100", 65, "geodesic", 2.0),
       ("cube", 1200, "lp", 2.0), ("cube", 1200, "geodesic", 2.0)])


def case_id(case):
    cloud, n, kind, p = case
    return f"{cloud}-{n}-{kind}-p{p:g}"


@functools.lru_cache(maxsize=None)
def reference(case):
    """Inputs and the independent float64 optimum of a case (computed once per session, never modified):
    x, y, extra, K, opt (float64 optimum of the mean cost), sigma (scipy's assignment)"""
    from scipy.optimize import linear_sum_assignment
    cloud, n, kind, p = case
    x, y, extra = build(cloud, n)
    C = cost_matrix(x, y, kind, p, np.float64)
    rows, sigma = linear_sum_assignment(C)
    opt = float(C[rows, sigma].mean())
    K = cost_bound(x, y, kind, p)
    for a in (x, y, sigma):
        a.setflags(write=False)
    return {"x": x, "y": y, "extra": extra, "K": K, "opt": opt, "sigma": sigma}


@functools.lru_cache(maxsize=None)
def restated(case):
    """the restatement's run of a case: assign, rounds, bids, K"""
    cloud, n, kind, p = case
    x, y, _ = build(cloud, n)
    c, K = integer_costs(x, y, kind, p)
    if K == 0:
        return {"assign": np.arange(n), "rounds": 0, "bids": 0, "K": K, "c": c}
    assign, rounds, bids = auction(c)
    return {"assign": assign, "rounds": rounds, "bids": bids, "K": K, "c": c}


# --------------------------------------------------------------------------------------------------------- gradients
GRAD_W = (1.0, -0.5)
GRAD_CASES = [(65, "lp", 2.0), (257, "lp", 3.0), (257, "lp", 1.0), (65, "geodesic", 1.0), (257, "geodesic", 2.0)]


def grad_inputs(n):
    """two registration-like pairs (B = 2)"""
    xs, ys = zip(*(build("registration", n, seed=7 + b)[:2] for b in range(2)))
    return np.stack(xs), np.stack(ys)


def torch_cost_along(x, y, assign, kind, p):
    """(B,) mean_i C(x_i, y_assign[i]) in torch (any dtype): what autograd differentiates"""
    import torch
    ya = torch.gather(y, 1, assign[..., None].expand(-1, -1, 3))
    if kind == "lp":
        return (x - ya).abs().pow(p).sum(-1).mean(1)
    theta = torch.atan2(torch.linalg.cross(x, ya, dim=-1).norm(dim=-1), (x * ya).sum(-1))
    return theta.pow(p).mean(1)


def torch_grads(x, y, assign, kind, p, dtype):
    import torch
    xd = torch.as_tensor(x).to(dtype).requires_grad_(True)
    yd = torch.as_tensor(y).to(dtype).requires_grad_(True)
    cost = torch_cost_along(xd, yd, torch.as_tensor(assign).long(), kind, p)
    (cost * torch.as_tensor(GRAD_W, dtype=dtype)).sum().backward()
    return xd.grad.numpy(), yd.grad.numpy()
