"""Seeded inputs and cached mirror runs (float64 = the reference value, float32 = its own rounding noise g) for the
gradients through the Sinkhorn plan P and cost matrix C and for the barycentric map, shared by
tests/test_sinkhorn_plan_gpu.py and tests/test_sinkhorn_plan_cpu.py.

The bound is the rule of tests/helpers/sinkhorn_chamfer_cases.py, imported unchanged: a kernel result lies within
bound(g) = max(16 g, FLOOR) of the float64 autograd through oracle/sinkhorn_mirror.py, g the float32 mirror's gap on the
same inputs (gradients in units of the largest entry).  The reasoning in that module's header applies as it stands: the
new seed kernels sum a row sequentially (y side, map) or per lane and then across the wave (dense x side, which is closer to
torch's pairwise sums) over at most 1025 candidates.

The two losses:  plan:  L = sum_b w_b cost_b + <WP, P> + <WC, C>   (linear in everything the call returns)
                 map :  L = sum ||T - x||^2 + sum_b w_b cost_b,  T = P @ y / P.sum(-1)."""
import functools

import numpy as np
import torch

from helpers import sinkhorn_chamfer_cases as cases
from oracle import sinkhorn_mirror

# the ragged shapes of the existing forward tests, plus one either side of what the dense x-side layout introduces: 16 rows
# per block (four waves of four rows) and 64 lanes along the candidates
SEED_EDGE_SHAPES = [(15, 65), (17, 63)]
PLAN_CASES = cases.FORWARD_CASES[:5] + [(n, m, 0.05, 30) for n, m in SEED_EDGE_SHAPES] + cases.FORWARD_CASES[5:]
B = 2
W = (1.0, -0.7)


def case_id(c):
    return "%dx%d_eps%g" % (c[0], c[1], c[2])


def plan_inputs(n, m, batch=B):
    """clouds of the forward tests and seeded cotangents: WP ~ N(0, 1), WC ~ N(0, 1) / (n m) so that the three terms of the
    loss contribute gradients of the same order"""
    x, y = cases.forward_inputs(n, m, B=batch)
    g = torch.Generator().manual_seed(1600 + 3 * n + m)
    WP = torch.randn(batch, n, m, generator=g)
    WC = torch.randn(batch, n, m, generator=g) / (n * m)
    return x, y, WP, WC


def plan_mirror(x, y, eps, iters, w, WP, WC, dtype, norm_p=2, cost_pow=1, thresh=1e-9, use=("cost", "P", "C")):
    """autograd through the mirror of L restricted to the outputs in `use`; cost is cost^(1/N) and C is C^N as the classes
    return them"""
    xd, yd = x.detach().clone().to(dtype).requires_grad_(True), y.detach().clone().to(dtype).requires_grad_(True)
    cost, P, C, its = sinkhorn_mirror.sinkhorn_costs(xd, yd, eps, iters, norm_p=norm_p, cost_pow=cost_pow, thresh=thresh)
    if cost_pow != 1:
        cost = cost.pow(1.0 / cost_pow)
    loss = 0
    if "cost" in use:
        loss = loss + (cost * torch.as_tensor(w, dtype=dtype)).sum()
    if "P" in use:
        loss = loss + (WP.to(dtype) * P).sum()
    if "C" in use:
        loss = loss + (WC.to(dtype) * C).sum()
    loss.backward()
    return {"cost": cost.detach().numpy(), "gx": xd.grad.numpy(), "gy": yd.grad.numpy(), "its": its}


def plan_reference(x, y, eps, iters, w, WP, WC, **kw):
    ref = plan_mirror(x, y, eps, iters, w, WP, WC, torch.float64, **kw)
    f32 = plan_mirror(x, y, eps, iters, w, WP, WC, torch.float32, **kw)
    g = cases.grad_gaps(f32["cost"], f32["gx"], f32["gy"], ref)
    g["its32"] = f32["its"]
    return ref, g


@functools.lru_cache(maxsize=None)
def plan_case(n, m, eps, iters, use=("cost", "P", "C")):
    """inputs, the float64 run and the float32 run's gaps (computed once per session, never modified)"""
    x, y, WP, WC = plan_inputs(n, m)
    return (x, y, WP, WC) + plan_reference(x, y, eps, iters, W, WP, WC, use=use)


def map_mirror(x, y, eps, iters, w, dtype, thresh=1e-9):
    xd, yd = x.detach().clone().to(dtype).requires_grad_(True), y.detach().clone().to(dtype).requires_grad_(True)
    cost, P, _, its = sinkhorn_mirror.sinkhorn_costs(xd, yd, eps, iters, thresh=thresh)
    r = P.sum(-1)
    T = P @ yd / r.unsqueeze(-1)
    (((T - xd) ** 2).sum() + (cost * torch.as_tensor(w, dtype=dtype)).sum()).backward()
    return {"T": T.detach().numpy(), "r": r.detach().numpy(), "cost": cost.detach().numpy(), "gx": xd.grad.numpy(),
            "gy": yd.grad.numpy(), "its": its}


def map_gaps(got, ref):
    return {"T": cases.of_largest(got["T"], ref["T"]), "r": cases.relmax(got["r"], ref["r"]),
            "cost": cases.relmax(got["cost"], ref["cost"]), "gx": cases.of_largest(got["gx"], ref["gx"]),
            "gy": cases.of_largest(got["gy"], ref["gy"])}


@functools.lru_cache(maxsize=None)
def map_case(n, m, eps, iters):
    x, y = cases.forward_inputs(n, m, B=B)
    ref = map_mirror(x, y, eps, iters, W, torch.float64)
    f32 = map_mirror(x, y, eps, iters, W, torch.float32)
    g = map_gaps(f32, ref)
    g["its32"] = f32["its"]
    return x, y, ref, g


@functools.lru_cache(maxsize=None)
def stop_plan_case():
    """cases.STOP_CASES[0]: its inputs, weights and threshold (the stop at sweep cases.STOP_T of 40), with the plan loss"""
    Bs, n, m, own = cases.STOP_CASES[0]
    x, y, w, thresh = cases.stop_case(Bs, n, m, own)[:4]
    g = torch.Generator().manual_seed(1600 + 3 * n + m)
    WP = torch.randn(Bs, n, m, generator=g)
    WC = torch.randn(Bs, n, m, generator=g) / (n * m)
    return (x, y, w, thresh, WP, WC) + plan_reference(x, y, 0.5, 40, w, WP, WC, thresh=thresh)


@functools.lru_cache(maxsize=None)
def no_sweep_plan_case():
    """max_iter = 0 at (257, 513): duals zero, P = exp(-C / eps)"""
    n, m = cases.VARIANT_SHAPE
    x, y = cases.variant_inputs()
    g = torch.Generator().manual_seed(1600 + 3 * n + m)
    WP = torch.randn(2, n, m, generator=g)
    WC = torch.randn(2, n, m, generator=g) / (n * m)
    return (x, y, WP, WC) + plan_reference(x, y, 0.05, 0, cases.VARIANT_W, WP, WC)


G17 = {"L2": dict(eps=0.05, max_iter=60, norm_p=2, cost_pow=1), "L1": dict(eps=0.05, max_iter=30, norm_p=1, cost_pow=1),
       "N2": dict(eps=0.05, max_iter=30, norm_p=2, cost_pow=2)}
