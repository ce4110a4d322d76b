"""Exact Wasserstein loss between two uniform clouds, with the call shapes of the reference's live
loss (losses/s2_wasserstein.py:13-66 `Cos_disimilarity_W`, :73-126 `Geodesic_distance_W`; Flow_cube.ipynb cell 5
`wasserstein_distance`, `wasserstein_distance_geo`), which go through POT's `ot.emd2` on the CPU, pair by pair.

With n = m and uniform weights optimal transport is a linear assignment problem; csrc/shw_emd.hip solves it with an
eps-scaling auction on fixed-point costs, one workgroup per pair.  "Exact" means: the mean cost along the
returned permutation is within K 2^-25 of the optimum, K the power of two the kernel finds above the largest cost of
the pair -- below the float32 resolution of the costs themselves.  POT is not installed: parity with `ot.emd2` itself
is unpinned; the tests compare with scipy.optimize.linear_sum_assignment.

Clouds of different sizes (the trainers' --source_p_n / --target_p_n, train_W_COS.py:292-293; the runner's 128 against
256 and 512 points) go through `transport_pair_costs`: with U = lcm(n, m) every source carries U / n units of mass 1 / U
and every target has U / m slots, the transport optimum is the optimum of the assignment problem between units and
slots, and csrc/shw_emd_units.hip runs the same auction on it without expanding the clouds.  It serves the pairs
`transport_units(n, m)` accepts: U <= 4096 and an LDS footprint within the CU -- every lcm(n, m) <= 2048, and e.g.
(768, 1024); a pair such as (1000, 1024), U = 128 000, is refused.  The modules and the notebook functions send n != m
there and n = m to `emd_pair_costs`.

Deviation from the reference, geodesic cost only: the angle is atan2(|x cross y|, x . y), not acos of the cosine
similarity, and where sin(angle) = 0 (a point matched to itself or to its antipode) or a point has zero length the
gradient written is 0 -- the reference's acos has an infinite derivative there and returns inf / NaN."""
from __future__ import annotations

import math

import torch
from torch import nn

from . import _lib
from .ssw import _check_cloud, _stream_ptr

_KINDS = {"lp": 0, "geodesic": 1}
_UNITS_LIMIT = 4096                   # shw_emd_units.hip kEmdUnitsMax: a bid word names its bidder in 12 bits
_UNITS_LDS_LIMIT = 160 * 1024 - 1024  # ... kEmdUnitsLdsMax


def max_points_emd() -> int:
    """Largest point count per cloud of the exact solver (`shw_max_points_emd`)."""
    return int(_lib.load().shw_max_points_emd())


class _EmdPairs(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, y, p, kind):
        lib = _lib.load()
        B, n, _ = x.shape
        dev = x.device
        xc, yc = x.contiguous(), y.contiguous()
        ws = torch.empty(max(int(lib.shw_emd_workspace_bytes(B, n)), 4) // 4, dtype=torch.int32, device=dev)
        cost = torch.empty(B, dtype=torch.float32, device=dev)
        assign = torch.empty(B, n, dtype=torch.int32, device=dev)
        rounds = torch.empty(B, dtype=torch.int32, device=dev)
        with torch.cuda.device(dev):
            _lib.check(lib.shw_emd_forward(xc.data_ptr(), yc.data_ptr(), B, n, n, kind, p, ws.data_ptr(),
                                           cost.data_ptr(), assign.data_ptr(), rounds.data_ptr(), _stream_ptr(dev)),
                       "shw_emd_forward")
        ctx.save_for_backward(xc, yc, ws)
        ctx.p, ctx.kind = p, kind
        ctx.mark_non_differentiable(assign, rounds)
        return cost, assign, rounds

    @staticmethod
    def backward(ctx, g_cost, _g_assign, _g_rounds):
        lib = _lib.load()
        xc, yc, ws = ctx.saved_tensors
        B, n, _ = xc.shape
        dev = xc.device
        gx = torch.empty_like(xc)
        gy = torch.empty_like(yc)
        w = g_cost.to(torch.float32).contiguous()
        with torch.cuda.device(dev):
            _lib.check(lib.shw_emd_backward(xc.data_ptr(), yc.data_ptr(), ws.data_ptr(), w.data_ptr(), B, n, ctx.kind,
                                            ctx.p, gx.data_ptr(), gy.data_ptr(), _stream_ptr(dev)), "shw_emd_backward")
        return gx, gy, None, None


class _EmdUnitPairs(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, y, p, kind, U):
        lib = _lib.load()
        B, n, _ = x.shape
        m = y.shape[1]
        dev = x.device
        xc, yc = x.contiguous(), y.contiguous()
        ws = torch.empty(max(int(lib.shw_emd_units_workspace_bytes(B, n, m)), 4) // 4, dtype=torch.int32, device=dev)
        cost = torch.empty(B, dtype=torch.float32, device=dev)
        targets = torch.empty(B, U, dtype=torch.int32, device=dev)
        rounds = torch.empty(B, dtype=torch.int32, device=dev)
        with torch.cuda.device(dev):
            _lib.check(lib.shw_emd_units_forward(xc.data_ptr(), yc.data_ptr(), B, n, m, kind, p, ws.data_ptr(),
                                                 cost.data_ptr(), targets.data_ptr(), rounds.data_ptr(),
                                                 _stream_ptr(dev)), "shw_emd_units_forward")
        ctx.save_for_backward(xc, yc, ws)
        ctx.p, ctx.kind = p, kind
        ctx.mark_non_differentiable(targets, rounds)
        return cost, targets, rounds

    @staticmethod
    def backward(ctx, g_cost, _g_targets, _g_rounds):
        lib = _lib.load()
        xc, yc, ws = ctx.saved_tensors
        B, n, _ = xc.shape
        m = yc.shape[1]
        dev = xc.device
        gx = torch.empty_like(xc)
        gy = torch.empty_like(yc)
        w = g_cost.to(torch.float32).contiguous()
        with torch.cuda.device(dev):
            _lib.check(lib.shw_emd_units_backward(xc.data_ptr(), yc.data_ptr(), ws.data_ptr(), w.data_ptr(), B, n, m,
                                                  ctx.kind, ctx.p, gx.data_ptr(), gy.data_ptr(), _stream_ptr(dev)),
                       "shw_emd_units_backward")
        return gx, gy, None, None, None


def transport_units(n, m):
    """(U, ks, kt) of a pair of sizes the unit solver serves: U = lcm(n, m) units of mass 1 / U, ks = U / n per source,
    kt = U / m slots per target.  Raises ValueError for a pair it does not serve (no HIP call is made)."""
    n, m = int(n), int(m)
    most = max_points_emd()
    if not (1 <= n <= most and 1 <= m <= most):
        raise ValueError(f"the exact solver takes 1..{most} points per cloud (its limit), got n = {n} and m = {m}")
    U = int(_lib.load().shw_emd_units_supported(n, m))
    if U == 0:
        lcm = n // math.gcd(n, m) * m
        why = (f"above its limit of {_UNITS_LIMIT} units" if lcm > _UNITS_LIMIT else
               f"whose 40 lcm(n, m) + 12 (n + m) = {40 * lcm + 12 * (n + m)} bytes of LDS are above its limit of "
               f"{_UNITS_LDS_LIMIT}")
        raise ValueError(f"the exact solver works on lcm(n, m) units of mass: n = {n}, m = {m} have lcm(n, m) = {lcm}, "
                         f"{why}; every pair with lcm(n, m) <= {most} is served (sinkhorn_pair_costs and the sliced "
                         "losses take any sizes)")
    return U, U // n, U // m


def transport_pair_costs(x, y, p=2, cost="lp", return_plan=False):
    """(B,n,3), (B,m,3) -> (B,) exact optimal-transport costs between uniform clouds of n and m points: the minimum over
    transport plans with marginals 1/n and 1/m of sum_ij P_ij C(x_i, y_j), C as in `emd_pair_costs` -- what `ot.emd2`
    returns for such a pair.  Solved as the assignment problem between the U = lcm(n, m) units of mass 1 / U of the
    sources and the slots of the targets (`transport_units`; pairs outside its size rule raise ValueError; n = m is
    accepted).  Differentiable in x and y (the plan is locally constant); gradients are bit-identical from run to run.
    `return_plan=True` also returns `targets` (B,U) int32, the target point of each unit -- units i U/n .. (i + 1) U/n - 1
    belong to source i, so P_ij = #{units of i with target j} / U -- and `rounds` (B,) int32.
    Uniform weights only.  A pair the solver gives up on (its round cap; never observed) has cost NaN and zero gradients."""
    for name, t in (("x", x), ("y", y)):
        if isinstance(t, torch.Tensor) and t.dtype != torch.float32:      # float64 stays refused after enable_float64()
            raise TypeError(f"{name} must be float32, got {t.dtype}: the exact solver is float32")
        _check_cloud(name, t)
    if cost not in _KINDS:
        raise ValueError(f"cost must be 'lp' or 'geodesic', got {cost!r}")
    if x.dim() != 3 or y.dim() != 3 or x.shape[0] != y.shape[0]:
        raise ValueError("x and y must be (B,n,3) and (B,m,3) with the same B")
    U, _, _ = transport_units(x.shape[1], y.shape[1])
    if not float(p) >= 1:
        raise ValueError(f"p must be >= 1, got {p}")
    out, targets, rounds = _EmdUnitPairs.apply(x, y, float(p), _KINDS[cost], U)
    return (out, targets, rounds) if return_plan else out


def _pair_costs(x, y, p, cost):
    """n = m: the assignment solver; n != m: the unit solver"""
    if x.dim() == 3 and y.dim() == 3 and x.shape[1] != y.shape[1]:
        return transport_pair_costs(x, y, p, cost)
    return emd_pair_costs(x, y, p, cost)


def emd_pair_costs(x, y, p=2, cost="lp", return_assignment=False):
    """(B,n,3), (B,n,3) -> (B,) exact optimal-transport costs between uniform clouds of equal size:
    min over permutations sigma of mean_i C(x_i, y_sigma(i)), C = sum_d |x_d - y_d|^p (`cost="lp"`, the reference's
    cos_cost_matrix) or angle(x, y)^p (`cost="geodesic"`), any float p >= 1.  Differentiable in x and y (the plan is
    locally constant, as for `ot.emd2`); gradients are bit-identical from run to run.  `return_assignment=True` also
    returns `assign` (B,n) int32, the target index of each source point, and `rounds` (B,) int32.
    A pair the solver gives up on (its round cap; never observed) has cost NaN and zero gradients."""
    for name, t in (("x", x), ("y", y)):
        if isinstance(t, torch.Tensor) and t.dtype != torch.float32:      # float64 stays refused after enable_float64()
            raise TypeError(f"{name} must be float32, got {t.dtype}: the exact solver is float32")
        _check_cloud(name, t)
    if cost not in _KINDS:
        raise ValueError(f"cost must be 'lp' or 'geodesic', got {cost!r}")
    if x.dim() != 3 or y.dim() != 3 or x.shape[0] != y.shape[0]:
        raise ValueError("x and y must be (B,n,3) and (B,n,3) with the same B")
    if x.shape[1] != y.shape[1]:
        raise ValueError(f"the exact solver needs clouds of equal sizes, got {x.shape[1]} and {y.shape[1]} points "
                         "(unequal sizes are a transport problem: sinkhorn_pair_costs, or the sliced losses)")
    most = max_points_emd()
    if not 1 <= x.shape[1] <= most:
        raise ValueError(f"the exact solver takes 1..{most} points per cloud (its limit), got {x.shape[1]}")
    if not float(p) >= 1:
        raise ValueError(f"p must be >= 1, got {p}")
    out, assign, rounds = _EmdPairs.apply(x, y, float(p), _KINDS[cost])
    return (out, assign, rounds) if return_assignment else out


def _reference_reduction(x, y, p, cost):
    """s2_wasserstein.py:25-50: batch mean of cost_b^(1/p) for (B,n,3), cost^(1/p) for (n,3); the root is torch.pow,
    so its gradient at cost = 0 behaves as the reference's does"""
    if x.dim() == 2 and y.dim() == 2:
        return torch.pow(_pair_costs(x.unsqueeze(0), y.unsqueeze(0), p, cost)[0], 1.0 / p)
    return torch.pow(_pair_costs(x, y, p, cost), 1.0 / p).mean()


class Cos_disimilarity_W(nn.Module):
    """`Cos_disimilarity_W(device, p)(x, y)` (s2_wasserstein.py:13-66; the CSW train_W_COS.py:393 builds with p = 2):
    exact W_p with the cost sum_d |x_d - y_d|^p.  Clouds of different sizes (--source_p_n / --target_p_n) are served
    within `transport_units`' size rule."""

    def __init__(self, device, p=1):
        super().__init__()
        self.device, self.p = device, p

    def forward(self, x, y):
        return _reference_reduction(x, y, self.p, "lp")


class Geodesic_distance_W(nn.Module):
    """`Geodesic_distance_W(device, p)(x, y)` (s2_wasserstein.py:73-126): exact W_p with the cost angle(x, y)^p
    (module docstring: atan2 form, zero gradient where the reference's acos gives inf / NaN)."""

    def __init__(self, device, p=1):
        super().__init__()
        self.device, self.p = device, p

    def forward(self, x, y):
        return _reference_reduction(x, y, self.p, "geodesic")


def wasserstein_distance(x, y, device, p=2):
    """Flow_cube.ipynb cell 5: one pair (n,3), (m,3) (or (1,n,3), (1,m,3)) -> emd2(C)^(1/p), C = sum_d |x_d - y_d|^p."""
    return _single_pair(x, y, p, "lp")


def wasserstein_distance_geo(x, y, device, p=2):
    """Flow_cube.ipynb cell 5: the same with C = angle(x, y)^p."""
    return _single_pair(x, y, p, "geodesic")


def _single_pair(x, y, p, cost):
    if x.dim() == 3 and x.shape[0] != 1:
        raise ValueError("the notebooks' function takes one pair; use the module or emd_pair_costs for a batch")
    xb = x if x.dim() == 3 else x.unsqueeze(0)
    yb = y if y.dim() == 3 else y.unsqueeze(0)
    return torch.pow(_pair_costs(xb, yb, p, cost)[0], 1.0 / p)


__all__ = ["emd_pair_costs", "transport_pair_costs", "transport_units", "max_points_emd", "Cos_disimilarity_W", "Geodesic_distance_W", "wasserstein_distance",
           "wasserstein_distance_geo"]
