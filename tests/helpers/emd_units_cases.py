"""Cases, the restatement and the independent exact optimum for the exact-W path of clouds of DIFFERENT sizes
(csrc/shw_emd_units.hip, emd.transport_pair_costs), shared by tests/test_emd_units_cpu.py and tests/test_emd_units_gpu.py.
Everything numeric comes from tests/helpers/emd_cases.py: the cost functions, K, the integer costs, the auction rule and
the bounds (its docstring derives them; they are used here with n -> U).

The formulation ("Exact W for clouds of different sizes").  g = gcd(n, m), ks = m / g, kt = n / g,
U = lcm(n, m) = n ks = m kt.  Source i carries the units i ks .. i ks + ks - 1 of mass 1 / U, target j has the slots
j kt .. j kt + kt - 1.  The transport optimum between the uniform clouds equals the optimum of the U x U assignment problem
with c(unit q, slot r) = C(x[q // ks], y[r // kt]): `expand` writes that matrix out, `restated` runs emd_cases.auction on
it (the rule the kernel applies without expanding anything), `reference` gives scipy's optimum of it in float64.

Sizes the kernel serves: 1 <= n, m <= 2048, U <= 4096 (12 id bits in a bid word) and 40 U + 12 (n + m) bytes of LDS (each
count rounded up to 4) within 160 KB - 1 KB: `units` restates that rule."""
import functools
import math

import numpy as np

from helpers import emd_cases

UNITS_LIMIT = 4096
LDS_LIMIT = 160 * 1024 - 1024


def lds_bytes(n, m):
    up4 = lambda v: (v + 3) // 4 * 4
    return 40 * up4(math.lcm(n, m)) + 12 * (up4(n) + up4(m))


def units(n, m):
    """(U, ks, kt) of a pair the kernel serves, None otherwise"""
    if not (1 <= n <= emd_cases.LIMIT and 1 <= m <= emd_cases.LIMIT):
        return None
    U = math.lcm(n, m)
    if U > UNITS_LIMIT or lds_bytes(n, m) > LDS_LIMIT:
        return None
    return U, U // n, U // m


def expand(c, ks, kt):
    """(n, m) costs of points -> (U, U) costs of (unit, slot)"""
    return np.repeat(np.repeat(c, ks, axis=0), kt, axis=1)


# ------------------------------------------------------------------------------------------------------------ clouds
def build(cloud, n, m, seed=0):
    """(x (n, 3), y (m, 3)) float32, drawn with the generators of emd_cases.build"""
    rng = emd_cases._rng(n, m, seed, sum(map(ord, cloud)))
    if cloud == "sphere":
        x, y = emd_cases._sphere(rng, n), emd_cases._sphere(rng, m)
    elif cloud == "registration":     # the trainers' situation at two densities: both clouds sample one shape, y rotated, noisy
        base = emd_cases._sphere(rng, max(n, m))
        x = base[:n].copy()
        y = base[:m].astype(np.float64) @ emd_cases._rotation(rng).T + 0.02 * rng.standard_normal((m, 3))
        y = (y / np.linalg.norm(y, axis=1, keepdims=True)).astype(np.float32)
    elif cloud == "zeros":
        x, y = np.zeros((n, 3), np.float32), np.zeros((m, 3), np.float32)
    elif cloud == "doubled":          # every source point twice in the target: one plan of cost exactly 0
        assert m == 2 * n
        x = emd_cases._sphere(rng, n)
        y = np.repeat(x, 2, axis=0)
    else:
        raise ValueError(cloud)
    return np.ascontiguousarray(x), np.ascontiguousarray(y)


# (cloud, n, m, kind, p): each the smallest place where something can go wrong
CASES = (
    ("sphere", 1, 2, "lp", 2.0), ("sphere", 1, 7, "lp", 2.0), ("sphere", 7, 1, "lp", 2.0),   # one point carries everything
    ("sphere", 2, 3, "lp", 2.0), ("sphere", 3, 2, "lp", 2.0),               # both multiplicities > 1 at the smallest size
    ("sphere", 8, 12, "lp", 2.0), ("sphere", 12, 8, "lp", 2.0),             # ks, kt = 3, 2; several lanes per bidder
    ("sphere", 65, 13, "lp", 1.0),                                          # m divides n: ks = 1, kt = 5
    ("sphere", 64, 96, "geodesic", 2.0), ("sphere", 96, 64, "geodesic", 2.0),
    ("sphere", 100, 75, "lp", 3.0),                                         # odd sizes, U = 300
    ("registration", 128, 256, "lp", 2.0), ("registration", 128, 512, "lp", 2.0),   # the runner's shapes; U > 512 threads
    ("sphere", 65, 65, "lp", 2.0),                                          # ks = kt = 1 through the new entry
    ("zeros", 32, 48, "geodesic", 2.0),                                     # every cost equal: the price war
    ("zeros", 32, 48, "lp", 2.0),                                           # K = 0: the identity without a round
    ("doubled", 33, 66, "lp", 2.0),                                         # one plan of integer cost 0
    ("registration", 768, 1024, "lp", 2.0),                                 # U = 3072: the layout's limit
)


def case_id(case):
    cloud, n, m, kind, p = case
    return f"{cloud}-{n}x{m}-{kind}-p{p:g}"


@functools.lru_cache(maxsize=None)
def reference(case):
    """Inputs and the independent float64 optimum of a case (computed once per session, never modified):
    x, y, U, ks, kt, K, opt (float64 optimum of the mean cost over units), targets (scipy's plan: target of each unit)"""
    from scipy.optimize import linear_sum_assignment
    cloud, n, m, kind, p = case
    U, ks, kt = units(n, m)
    x, y = build(cloud, n, m)
    C = expand(emd_cases.cost_matrix(x, y, kind, p, np.float64), ks, kt)
    rows, slots = linear_sum_assignment(C)
    opt = float(C[rows, slots].mean())
    targets = slots // kt
    K = emd_cases.cost_bound(x, y, kind, p)
    for a in (x, y, targets):
        a.setflags(write=False)
    return {"x": x, "y": y, "U": U, "ks": ks, "kt": kt, "K": K, "opt": opt, "targets": targets}


@functools.lru_cache(maxsize=None)
def restated(case):
    """the restatement's run of a case: targets (target point of each unit), rounds, bids, K, c (n, m) integer costs"""
    cloud, n, m, kind, p = case
    U, ks, kt = units(n, m)
    x, y = build(cloud, n, m)
    c, K = emd_cases.integer_costs(x, y, kind, p)
    if K == 0:
        return {"targets": np.arange(U) // kt, "rounds": 0, "bids": 0, "K": K, "c": c}
    slot, rounds, bids = emd_cases.auction(expand(c, ks, kt))
    return {"targets": None if slot is None else slot // kt, "rounds": rounds, "bids": bids, "K": K, "c": c}


# ------------------------------------------------------------------------------------------------- along a unit plan
def feasible(targets, m, kt):
    """every target is held by exactly kt units"""
    t = np.asarray(targets)
    return t.min() >= 0 and t.max() < m and np.array_equal(np.bincount(t, minlength=m), np.full(m, kt))


def mean_along(x, y, kind, p, targets, ks, dtype=np.float64):
    """(1/U) sum_q C(x[q // ks], y[targets[q]]) evaluated in dtype"""
    return emd_cases.mean_along(np.repeat(x, ks, axis=0), y, kind, p, targets, dtype)


def eval_gap(x, y, kind, p, targets, ks):
    return emd_cases.eval_gap(np.repeat(x, ks, axis=0), y, kind, p, targets)


def cost_bound_along(x, y, kind, p, targets, ks):
    return emd_cases.cost_bound_along(np.repeat(x, ks, axis=0), y, kind, p, targets)


# --------------------------------------------------------------------------------------------------------- gradients
GRAD_W = emd_cases.GRAD_W
GRAD_CASES = [(8, 12, "lp", 2.0), (65, 13, "lp", 1.0), (100, 75, "lp", 3.0), (96, 64, "geodesic", 2.0)]


def grad_inputs(n, m):
    """two registration-like pairs (B = 2)"""
    xs, ys = zip(*(build("registration", n, m, seed=7 + b) for b in range(len(GRAD_W))))
    return np.stack(xs), np.stack(ys)


def torch_grads(x, y, targets, ks, kind, p, dtype):
    """d/dx, d/dy of sum_b GRAD_W[b] (1/U) sum_q C(x[b, q // ks], y[b, targets[b, q]]) by torch autograd: a source row
    receives the sum over its ks units"""
    import torch
    xd = torch.as_tensor(x).to(dtype).requires_grad_(True)
    yd = torch.as_tensor(y).to(dtype).requires_grad_(True)
    cost = emd_cases.torch_cost_along(xd.repeat_interleave(ks, dim=1), yd, torch.as_tensor(targets).long(), kind, p)
    (cost * torch.as_tensor(GRAD_W, dtype=dtype)).sum().backward()
    return xd.grad.numpy(), yd.grad.numpy()
