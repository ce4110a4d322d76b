"""Log-domain Sinkhorn distance with the reference's class interface
(/root/reference/Comparison_Wasserstein_with_Chamfer_distance/losses/sinkhorn.py:3-87 and :92-186; used at
main_rotation.py:207-211):

    criteria = log_Sinkhorn_Distance_Loss(eps, max_iter, batch_reduction='sum', type_of_cost_norm='L2')
    loss, P, C = criteria(template, source, device)

Differentiable like the reference (its forward is autograd-visible through the unrolled iterations, :35-49): when a
cloud requires grad the iterations keep the trajectory of the duals and `backward` walks it (shw_sinkhorn_backward;
round 2).  The dense plan P and cost matrix C the
reference returns are produced on request by the SAME solve (`return_plan=True`, the default, keeps the call a drop-in;
`return_plan=False` returns (cost, None, None) and never allocates the two (B, n, m) tensors).

Gradients through P and C are an opt-in.  By default a training call returns P and C as plain values (marked
non-differentiable) and the gradient is that of the cost.  With `plan_grad=True` P and C are outputs of the autograd
node, as the reference's are (:46-60): a loss built on them (soft correspondences `P @ y`, a residual on C, ...) reaches
both clouds.  Their cotangents seed the same adjoint recursion (shw_sinkhorn_backward_plan): the walk over the iterations
is the one of the cost gradient, and when only the cost is consumed the cost-only entry runs, with the same bits.  The
training workspace, (max_iter + 2) B (n + m) floats, then lives as long as P or C does (they hold the graph node).

`sinkhorn_barycentric_map` is the memory-free form of the main use of the plan: T_i = sum_j P_ij y_j / sum_j P_ij from the
same single solve as the cost, differentiable w.r.t. both clouds, with nothing of size (B, n, m) read or written in
either direction."""
from __future__ import annotations

import torch

from . import _lib
from .ssw import _check_cloud, _stream_ptr


class _SinkhornCosts(torch.autograd.Function):
    """(B,n,3), (B,m,3) -> (B,) costs with the gradient through the unrolled iterations."""

    @staticmethod
    def forward(ctx, x, y, eps, max_iter, norm_p, cost_pow, thresh, return_plan, plan=False):
        """plan=True (only from _SinkhornPlan): P and C are allocated and stay differentiable outputs"""
        return_plan = return_plan or plan
        lib = _lib.load()
        B, n, _ = x.shape
        m = y.shape[1]
        dev = x.device
        xc, yc = x.contiguous(), y.contiguous()
        ws = torch.empty(lib.shw_sinkhorn_train_workspace_bytes(B, n, m, max_iter), dtype=torch.uint8, device=dev)
        cost = torch.empty(B, dtype=torch.float32, device=dev)
        # the dense outputs of the reference, from the SAME solve (a second solve doubled the step)
        P = torch.empty(B, n, m, dtype=torch.float32, device=dev) if return_plan else None
        C = torch.empty(B, n, m, dtype=torch.float32, device=dev) if return_plan else None
        with torch.cuda.device(dev):
            _lib.check(lib.shw_sinkhorn_forward_train(xc.data_ptr(), yc.data_ptr(), B, n, m, eps, max_iter, norm_p,
                                                      cost_pow, thresh, ws.data_ptr(), cost.data_ptr(),
                                                      P.data_ptr() if return_plan else None,
                                                      C.data_ptr() if return_plan else None, _stream_ptr(dev)),
                       "shw_sinkhorn_forward_train")
        ctx.save_for_backward(xc, yc, ws)
        ctx.cfg = (B, n, m, eps, max_iter, norm_p, cost_pow)
        if return_plan and not plan:
            ctx.mark_non_differentiable(P, C)
        return cost, P, C

    @staticmethod
    def backward(ctx, g, _gP=None, _gC=None):
        lib = _lib.load()
        xc, yc, ws = ctx.saved_tensors
        B, n, m, eps, max_iter, norm_p, cost_pow = ctx.cfg
        dev = xc.device
        gx, gy = torch.empty_like(xc), torch.empty_like(yc)
        gc = g.to(torch.float32).contiguous()
        with torch.cuda.device(dev):
            _lib.check(lib.shw_sinkhorn_backward(xc.data_ptr(), yc.data_ptr(), B, n, m, eps, max_iter, norm_p, cost_pow,
                                                 ws.data_ptr(), gc.data_ptr(), gx.data_ptr(), gy.data_ptr(),
                                                 _stream_ptr(dev)), "shw_sinkhorn_backward")
        return gx, gy, None, None, None, None, None, None


class _SinkhornPlan(torch.autograd.Function):
    """_SinkhornCosts with P and C as differentiable outputs (`plan_grad=True`): their cotangents reach backward."""

    @staticmethod
    def forward(ctx, x, y, eps, max_iter, norm_p, cost_pow, thresh):
        ctx.set_materialize_grads(False)          # an unused output arrives as None and travels as a null pointer
        cost, P, C = _SinkhornCosts.forward(ctx, x, y, eps, max_iter, norm_p, cost_pow, thresh, False, plan=True)
        return cost, P, C

    @staticmethod
    def backward(ctx, g, gP, gC):
        if gP is None and gC is None:
            return _SinkhornCosts.backward(ctx, g)[:2] + (None,) * 5         # cost only: the cost-only entry, same bits
        lib = _lib.load()
        xc, yc, ws = ctx.saved_tensors
        B, n, m, eps, max_iter, norm_p, cost_pow = ctx.cfg
        dev = xc.device
        gx, gy = torch.empty_like(xc), torch.empty_like(yc)
        gc, gPc, gCc = (None if t is None else t.to(torch.float32).contiguous() for t in (g, gP, gC))
        with torch.cuda.device(dev):
            _lib.check(lib.shw_sinkhorn_backward_plan(xc.data_ptr(), yc.data_ptr(), B, n, m, eps, max_iter, norm_p, cost_pow,
                                                      ws.data_ptr(), *(None if t is None else t.data_ptr()
                                                                       for t in (gc, gPc, gCc)),
                                                      gx.data_ptr(), gy.data_ptr(), _stream_ptr(dev)),
                       "shw_sinkhorn_backward_plan")
        return gx, gy, None, None, None, None, None


class _SinkhornMap(torch.autograd.Function):
    """(B,n,3), (B,m,3) -> map T (B,n,3), cost (B,), row sums r (B,n); gradients of T and cost w.r.t. both clouds."""

    @staticmethod
    def forward(ctx, x, y, eps, max_iter, norm_p, cost_pow, thresh):
        ctx.set_materialize_grads(False)
        lib = _lib.load()
        B, n, _ = x.shape
        m = y.shape[1]
        dev = x.device
        xc, yc = x.contiguous(), y.contiguous()
        ws = torch.empty(lib.shw_sinkhorn_train_workspace_bytes(B, n, m, max_iter), dtype=torch.uint8, device=dev)
        cost = torch.empty(B, dtype=torch.float32, device=dev)
        T = torch.empty(B, n, 3, dtype=torch.float32, device=dev)
        r = torch.empty(B, n, dtype=torch.float32, device=dev)
        with torch.cuda.device(dev):
            _lib.check(lib.shw_sinkhorn_map_forward(xc.data_ptr(), yc.data_ptr(), B, n, m, eps, max_iter, norm_p, cost_pow,
                                                    thresh, ws.data_ptr(), cost.data_ptr(), T.data_ptr(), r.data_ptr(),
                                                    _stream_ptr(dev)), "shw_sinkhorn_map_forward")
        ctx.save_for_backward(xc, yc, ws, T, r)
        ctx.cfg = (B, n, m, eps, max_iter, norm_p, cost_pow)
        ctx.mark_non_differentiable(r)
        return T, cost, r

    @staticmethod
    def backward(ctx, gT, g, _gr=None):
        lib = _lib.load()
        xc, yc, ws, T, r = ctx.saved_tensors
        B, n, m, eps, max_iter, norm_p, cost_pow = ctx.cfg
        dev = xc.device
        gx, gy = torch.empty_like(xc), torch.empty_like(yc)
        gc = None if g is None else g.to(torch.float32).contiguous()
        with torch.cuda.device(dev):
            if gT is None:                        # only the cost is consumed: the cost-only entry, same bits
                _lib.check(lib.shw_sinkhorn_backward(xc.data_ptr(), yc.data_ptr(), B, n, m, eps, max_iter, norm_p, cost_pow,
                                                     ws.data_ptr(), gc.data_ptr(), gx.data_ptr(), gy.data_ptr(),
                                                     _stream_ptr(dev)), "shw_sinkhorn_backward")
            else:
                gTc = gT.to(torch.float32).contiguous()
                _lib.check(lib.shw_sinkhorn_map_backward(xc.data_ptr(), yc.data_ptr(), B, n, m, eps, max_iter, norm_p,
                                                         cost_pow, ws.data_ptr(), T.data_ptr(), r.data_ptr(),
                                                         gTc.data_ptr(), None if gc is None else gc.data_ptr(),
                                                         gx.data_ptr(), gy.data_ptr(), _stream_ptr(dev)),
                           "shw_sinkhorn_map_backward")
        return gx, gy, None, None, None, None, None


def sinkhorn_barycentric_map(x, y, eps, max_iter, norm_p=2, cost_pow=1, thresh=1e-9, return_cost=False):
    """(B,n,3), (B,m,3) -> T (B,n,3) [, cost (B,)]: the soft correspondences T_i = sum_j P_ij y_j / r_i, r_i = sum_j P_ij,
    of the plan of sinkhorn_pair_costs, from the same single solve as the cost (`return_cost=True` returns the bits of
    sinkhorn_pair_costs) and without the dense (B, n, m) tensors, forward or backward.  Differentiable w.r.t. both clouds
    through the unrolled iterations.  A row whose whole sum underflowed (r_i = 0, far outside the other cloud at a small
    eps) gives T_i = 0 and passes no gradient.  The solve always keeps the trajectory of the duals (the training
    workspace, (max_iter + 2) B (n + m) floats), also under no_grad."""
    _check_cloud("x", x)
    _check_cloud("y", y)
    if x.dim() != 3 or y.dim() != 3 or x.shape[0] != y.shape[0]:
        raise ValueError("x and y must be (B,n,3) and (B,m,3) with the same B")
    T, cost, _ = _SinkhornMap.apply(x, y, float(eps), int(max_iter), int(norm_p), int(cost_pow), float(thresh))
    return (T, cost) if return_cost else T


def sinkhorn_pair_costs(x, y, eps, max_iter, norm_p=2, cost_pow=1, thresh=1e-9, return_plan=False, plan_grad=False):
    """(B,n,3), (B,m,3) -> (B,) transport costs sum_ij P_ij C_ij [, P, C].  plan_grad=True (needs return_plan=True): P and
    C carry the gradient to both clouds, see the module docstring; under no_grad or with no cloud requiring grad it
    changes nothing."""
    _check_cloud("x", x)
    _check_cloud("y", y)
    if x.dim() != 3 or y.dim() != 3 or x.shape[0] != y.shape[0]:
        raise ValueError("x and y must be (B,n,3) and (B,m,3) with the same B")
    if plan_grad and not return_plan:
        raise ValueError("plan_grad=True needs return_plan=True: there is no plan to differentiate through")
    if torch.is_grad_enabled() and (x.requires_grad or y.requires_grad):
        if plan_grad:
            return _SinkhornPlan.apply(x, y, float(eps), int(max_iter), int(norm_p), int(cost_pow), float(thresh))
        # P and C come out of the same solve; without plan_grad they are plain values, marked non-differentiable, and the
        # gradient is that of the cost (plan_grad=True makes them outputs of the node, as the reference's are)
        return _SinkhornCosts.apply(x, y, float(eps), int(max_iter), int(norm_p), int(cost_pow), float(thresh),
                                    bool(return_plan))
    lib = _lib.load()
    B, n, _ = x.shape
    m = y.shape[1]
    dev = x.device
    xc, yc = x.contiguous(), y.contiguous()
    ws = torch.empty(lib.shw_sinkhorn_workspace_bytes(B, n, m), dtype=torch.uint8, device=dev)
    cost = torch.empty(B, dtype=torch.float32, device=dev)
    P = C = None
    if return_plan:
        P = torch.empty(B, n, m, dtype=torch.float32, device=dev)
        C = torch.empty(B, n, m, dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        _lib.check(lib.shw_sinkhorn_forward(xc.data_ptr(), yc.data_ptr(), B, n, m, float(eps), int(max_iter),
                                            int(norm_p), int(cost_pow), float(thresh), ws.data_ptr(), cost.data_ptr(),
                                            P.data_ptr() if return_plan else None,
                                            C.data_ptr() if return_plan else None, _stream_ptr(dev)),
                   "shw_sinkhorn_forward")
    return cost, P, C


class log_Sinkhorn_Distance_Loss(torch.nn.Module):
    """Reference signature (sinkhorn.py:7, :14)."""

    cost_pow = 1

    def __init__(self, eps, max_iter, batch_reduction="none", type_of_cost_norm="L2", return_plan=True, plan_grad=False):
        super().__init__()
        if plan_grad and not return_plan:
            raise ValueError("plan_grad=True needs return_plan=True: there is no plan to differentiate through")
        self.plan_grad = plan_grad
        self.eps = eps
        self.max_iter = max_iter
        self.batch_reduction = batch_reduction
        self.p = int(type_of_cost_norm[-1])
        self.return_plan = return_plan

    def forward(self, x, y, device=None):
        single = x.dim() == 2
        if single:
            x, y = x.unsqueeze(0), y.unsqueeze(0)
        cost, P, C = sinkhorn_pair_costs(x, y, self.eps, self.max_iter, self.p, self.cost_pow, 1e-9, self.return_plan,
                                         self.plan_grad)
        if self.cost_pow != 1:
            cost = torch.pow(cost, 1.0 / self.cost_pow)
        if single:
            cost = cost[0]
            P = None if P is None else P[0]
            C = None if C is None else C[0]
        if self.batch_reduction == "mean":
            cost = cost.mean()
        elif self.batch_reduction == "sum":
            cost = cost.sum()
        return cost, P, C


class log_N_Sinkhorn_Distance_Loss(log_Sinkhorn_Distance_Loss):
    """Reference signature (sinkhorn.py:96): cost matrix raised to the power N, result to the power 1/N."""

    def __init__(self, eps, max_iter, batch_reduction="none", type_of_cost_norm="L2", type_of_Wasserstein_N="2",
                 return_plan=True, plan_grad=False):
        super().__init__(eps, max_iter, batch_reduction, type_of_cost_norm, return_plan, plan_grad)
        self.N = int(type_of_Wasserstein_N)
        self.cost_pow = self.N
