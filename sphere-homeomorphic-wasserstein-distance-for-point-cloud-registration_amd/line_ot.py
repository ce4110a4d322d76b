"""Exact 1-D optimal transport between two weighted empirical measures on the line, on the HIP path
(csrc/shw_line_ot.hip, include/shw.h shw_line_*): the Euclidean sliced family for clouds of different size and for
weighted clouds -- what `sliced_cost` / `binary_search_circle` already do on the sphere.

    line_ot_rows(u_rows, v_rows, p, u_weights, v_weights, weight_grad)      rows of keys the caller computed
    esw_slice_costs(Xs, Xt, thetas, p, u_weights, v_weights, weight_grad)   keys x . theta formed inside the kernel
    weighted_sliced_wasserstein_distance(first, second, ...)                the notebook's SWD call shape on top

A row has values u_1..u_n with weights a_i >= 0 and values v_1..v_m with weights b_j >= 0; the kernel divides the weights
by their sums, `None` means uniform.  The cost is W_p^p = int_0^1 |F_u^-1(t) - F_v^-1(t)|^p dt (the quantile merge) for
any real p >= 1.  It is MASS-NORMALISED: for n == m and no weights it equals `sorted_row_sums / n` (`esw_slice_sums / n`),
which sum over points.  An atom of weight 0 contributes nothing and receives gradient 0, so a padded batch is evaluated
with zero-weight padding.  Gradients are with respect to the values (both sides, and the directions of the fused op).
Gradients with respect to the weights are opt-in: by default a weight tensor that requires grad is refused, with
`weight_grad=True` it receives a gradient of its own shape (values, directions and weights in any combination; without
a weight that requires grad the keyword does nothing).  That gradient is the Kantorovich potential at the atom, centred
and divided by the row's weight sum (include/shw.h has the definition): the cost does not change when a side's weights
are scaled, so sum_i a_i * grad_i = 0; a side of one atom gets exactly 0; an atom of weight 0 gets the rate at which the
cost changes when it gains mass (its value gradient stays 0); where CDF ends of the two sides coincide the cost has a kink
in the weights and the result is one subgradient (on equal levels the first side's end comes first).  Weights must be
finite and non-negative with a positive sum per row: that is NOT checked (it would cost a device synchronisation); a
row whose weights sum to zero or less comes back, in bounded time, as a value that means nothing.  A weighted CDF lives
on a grid of 2^30 steps: an atom lighter than 2^-31 of its row's total is rounded away.  Cost and gradients are the same
bits on every run."""
from __future__ import annotations

import torch

from . import _lib
from .esw import MAX_POINTS, _check_esw_cloud, rand_projections
from .gsw import _check_rows
from .ssw import _stream_ptr

MAX_PAIRS = 65535      # include/shw.h shw_line_esw_*


def _check_weights(name, w, count, lead, lead_name, weight_grad=False):
    """None, (count,) shared, or lead + (count,) -> (contiguous tensor or None, stride in floats); with `weight_grad` the
    tensor stays in the graph"""
    if w is None:
        return None, 0
    if not isinstance(w, torch.Tensor):
        raise TypeError(f"{name} must be a torch.Tensor or None")
    if w.requires_grad and not weight_grad:
        raise ValueError(f"{name} requires grad: the line transport has no gradient with respect to the weights "
                         "(detach them) unless it is asked for with weight_grad=True")
    if not w.is_cuda:
        raise RuntimeError(f"{name} is on {w.device}: the MI355X HIP path needs device tensors (no CPU fallback)")
    if w.dtype != torch.float32:
        raise TypeError(f"{name} must be float32, got {w.dtype}")
    if tuple(w.shape) == (count,):
        return w.contiguous(), 0
    if tuple(w.shape) == tuple(lead) + (count,):
        return w.reshape(-1, count).contiguous(), count
    raise ValueError(f"{name} must have shape ({count},) or {lead_name}, got {tuple(w.shape)}")


def _ptr(t):
    return None if t is None else t.data_ptr()


class _LineRows(torch.autograd.Function):
    @staticmethod
    def forward(ctx, u, v, p, wu, wv, su, sv, need_grad):
        lib = _lib.load()
        rows, n = u.shape
        m = v.shape[1]
        dev = u.device
        cost = torch.empty(rows, dtype=torch.float32, device=dev)
        cu = cv = None
        if need_grad:
            cu = torch.empty(rows, n, dtype=torch.float32, device=dev)
            cv = torch.empty(rows, m, dtype=torch.float32, device=dev)
        with torch.cuda.device(dev):
            _lib.check(lib.shw_line_rows_forward(u.data_ptr(), v.data_ptr(), rows, n, m, float(p), _ptr(wu), _ptr(wv), su,
                                                 sv, cost.data_ptr(), _ptr(cu), _ptr(cv), _stream_ptr(dev)),
                       "shw_line_rows_forward")
        if need_grad:
            ctx.save_for_backward(cu, cv)
        return cost

    @staticmethod
    def backward(ctx, g):
        cu, cv = ctx.saved_tensors
        w = g.to(torch.float32).unsqueeze(-1)
        return ((cu * w if ctx.needs_input_grad[0] else None), (cv * w if ctx.needs_input_grad[1] else None),
                None, None, None, None, None, None)


def _wants_grad(t):
    return t is not None and t.requires_grad


def _weight_grads(pot, slice_w, pairs, slices, count, shared):
    """shw_line_weight_grads: (pairs*slices, count) potentials, (pairs*slices,) upstream -> (pairs, count), or (count,)"""
    lib = _lib.load()
    dev = pot.device
    if shared and pairs * slices > MAX_PAIRS * 64:
        raise ValueError(f"weights shared by more than {MAX_PAIRS * 64} rows: split the call")
    grad = torch.empty((count,) if shared else (pairs, count), dtype=torch.float32, device=dev)
    nbytes = lib.shw_line_weight_grads_workspace_bytes(pairs, slices, count, int(shared))
    work = torch.empty(nbytes // 4, dtype=torch.float32, device=dev) if nbytes else None
    with torch.cuda.device(dev):
        _lib.check(lib.shw_line_weight_grads(pot.data_ptr(), slice_w.data_ptr(), pairs, slices, count, int(shared),
                                             _ptr(work), grad.data_ptr(), _stream_ptr(dev)), "shw_line_weight_grads")
    return grad


class _LineRowsWeighted(torch.autograd.Function):
    """_LineRows with the weights in the graph (weight_grad=True and a weight that requires grad)"""

    @staticmethod
    def forward(ctx, u, v, wu, wv, p, su, sv):
        lib = _lib.load()
        rows, n = u.shape
        m = v.shape[1]
        dev = u.device
        need = ctx.needs_input_grad
        cost = torch.empty(rows, dtype=torch.float32, device=dev)
        cu = cv = pu = pv = None
        if need[0] or need[1]:
            cu = torch.empty(rows, n, dtype=torch.float32, device=dev)
            cv = torch.empty(rows, m, dtype=torch.float32, device=dev)
        if need[2]:
            pu = torch.empty(rows, n, dtype=torch.float32, device=dev)
        if need[3]:
            pv = torch.empty(rows, m, dtype=torch.float32, device=dev)
        with torch.cuda.device(dev):
            _lib.check(lib.shw_line_rows_forward_pot(u.data_ptr(), v.data_ptr(), rows, n, m, float(p), _ptr(wu), _ptr(wv),
                                                     su, sv, cost.data_ptr(), _ptr(cu), _ptr(cv), _ptr(pu), _ptr(pv),
                                                     _stream_ptr(dev)), "shw_line_rows_forward_pot")
        ctx.held = (cu, cv, pu, pv)
        ctx.dims = (rows, n, m, su, sv)
        return cost

    @staticmethod
    def backward(ctx, g):
        cu, cv, pu, pv = ctx.held
        rows, n, m, su, sv = ctx.dims
        g = g.to(torch.float32).contiguous()
        w = g.unsqueeze(-1)
        need = ctx.needs_input_grad
        gwu = gwv = None
        if need[2]:          # shared (n,): the reduction over the rows; per row: pot * g
            gwu = _weight_grads(pu, g, 1, rows, n, True) if su == 0 else pu * w
        if need[3]:
            gwv = _weight_grads(pv, g, 1, rows, m, True) if sv == 0 else pv * w
        return (cu * w if need[0] else None), (cv * w if need[1] else None), gwu, gwv, None, None, None


def line_ot_rows(u_rows, v_rows, p=2, u_weights=None, v_weights=None, weight_grad=False):
    """(..., n), (..., m) -> (...): W_p^p between the two weighted empirical measures of every row pair, 1 <= n, m <= 4096,
    mass-normalised (n == m, no weights: `sorted_row_sums / n`).  The keys are the caller's -- a circular or polynomial
    defining function, a network's output -- so this carries the generalised sliced family at n != m.  Weights are
    (n,) / (m,) shared by all rows, or the rows' own shape; None is uniform.  Differentiable w.r.t. both row tensors and,
    with `weight_grad=True`, w.r.t. the weights (the module docstring says what that gradient is)."""
    _check_rows("u_rows", u_rows)
    _check_rows("v_rows", v_rows)
    if u_rows.shape[:-1] != v_rows.shape[:-1]:
        raise ValueError(f"the line transport pairs rows: leading shapes must agree, got {tuple(u_rows.shape)} and "
                         f"{tuple(v_rows.shape)}")
    if not float(p) >= 1:
        raise ValueError(f"p must be at least 1, got {p}")
    lead, n, m = u_rows.shape[:-1], u_rows.shape[-1], v_rows.shape[-1]
    wu, su = _check_weights("u_weights", u_weights, n, lead, f"u_rows' shape {tuple(u_rows.shape)}", weight_grad)
    wv, sv = _check_weights("v_weights", v_weights, m, lead, f"v_rows' shape {tuple(v_rows.shape)}", weight_grad)
    u = u_rows.reshape(-1, n).contiguous()
    v = v_rows.reshape(-1, m).contiguous()
    if torch.is_grad_enabled() and (_wants_grad(wu) or _wants_grad(wv)):
        return _LineRowsWeighted.apply(u, v, wu, wv, float(p), su, sv).reshape(lead)
    need = torch.is_grad_enabled() and (u_rows.requires_grad or v_rows.requires_grad)
    return _LineRows.apply(u, v, float(p), wu, wv, su, sv, need).reshape(lead)


class _LineSliceCosts(torch.autograd.Function):
    @staticmethod
    def forward(ctx, Xs, Xt, thetas, p, wu, wv, su, sv, need_grad):
        lib = _lib.load()
        B, n, D = Xs.shape
        m = Xt.shape[1]
        L = thetas.shape[-2]
        dev = Xs.device
        xs, xt, th = Xs.contiguous(), Xt.contiguous(), thetas.contiguous()
        stride = 0 if th.dim() == 2 else L * D
        cost = torch.empty(B * L, dtype=torch.float32, device=dev)
        cs = ct = None
        if need_grad:
            cs = torch.empty(B * L * n, dtype=torch.float32, device=dev)
            ct = torch.empty(B * L * m, dtype=torch.float32, device=dev)
        with torch.cuda.device(dev):
            _lib.check(lib.shw_line_esw_forward(xs.data_ptr(), xt.data_ptr(), th.data_ptr(), B, n, m, D, L, stride,
                                                float(p), _ptr(wu), _ptr(wv), su, sv, cost.data_ptr(), _ptr(cs), _ptr(ct),
                                                _stream_ptr(dev)), "shw_line_esw_forward")
        if need_grad:
            ctx.save_for_backward(th, cs, ct, xs, xt)
            ctx.dims = (B, n, m, D, L, stride)
            ctx.theta_shape = tuple(thetas.shape)
        return cost.view(B, L)

    @staticmethod
    def backward(ctx, g):
        lib = _lib.load()
        th, cs, ct, xs, xt = ctx.saved_tensors
        B, n, m, D, L, stride = ctx.dims
        dev = th.device
        gxs = gxt = gth = None
        w = g.to(torch.float32).contiguous()
        with torch.cuda.device(dev):
            if ctx.needs_input_grad[0] or ctx.needs_input_grad[1]:
                gxs = torch.empty(B, n, D, dtype=torch.float32, device=dev)
                gxt = torch.empty(B, m, D, dtype=torch.float32, device=dev)
                _lib.check(lib.shw_line_esw_backward_points(th.data_ptr(), cs.data_ptr(), ct.data_ptr(), w.data_ptr(), B, n,
                                                            m, D, L, stride, gxs.data_ptr(), gxt.data_ptr(),
                                                            _stream_ptr(dev)), "shw_line_esw_backward_points")
            if ctx.needs_input_grad[2]:
                gth = torch.empty(B, L, D, dtype=torch.float32, device=dev)
                _lib.check(lib.shw_line_esw_backward_dirs(xs.data_ptr(), xt.data_ptr(), cs.data_ptr(), ct.data_ptr(),
                                                          w.data_ptr(), B, n, m, D, L, gth.data_ptr(), _stream_ptr(dev)),
                           "shw_line_esw_backward_dirs")
                if len(ctx.theta_shape) == 2:          # directions shared by the pairs
                    gth = gth.sum(0)
        return gxs, gxt, gth, None, None, None, None, None, None


class _LineSliceCostsWeighted(torch.autograd.Function):
    """_LineSliceCosts with the weights in the graph (weight_grad=True and a weight that requires grad)"""

    @staticmethod
    def forward(ctx, Xs, Xt, thetas, wu, wv, p, su, sv):
        lib = _lib.load()
        B, n, D = Xs.shape
        m = Xt.shape[1]
        L = thetas.shape[-2]
        dev = Xs.device
        need = ctx.needs_input_grad
        xs, xt, th = Xs.contiguous(), Xt.contiguous(), thetas.contiguous()
        stride = 0 if th.dim() == 2 else L * D
        cost = torch.empty(B * L, dtype=torch.float32, device=dev)
        cs = ct = pu = pv = None
        if need[0] or need[1] or need[2]:
            cs = torch.empty(B * L * n, dtype=torch.float32, device=dev)
            ct = torch.empty(B * L * m, dtype=torch.float32, device=dev)
        if need[3]:
            pu = torch.empty(B * L, n, dtype=torch.float32, device=dev)
        if need[4]:
            pv = torch.empty(B * L, m, dtype=torch.float32, device=dev)
        with torch.cuda.device(dev):
            _lib.check(lib.shw_line_esw_forward_pot(xs.data_ptr(), xt.data_ptr(), th.data_ptr(), B, n, m, D, L, stride,
                                                    float(p), _ptr(wu), _ptr(wv), su, sv, cost.data_ptr(), _ptr(cs),
                                                    _ptr(ct), _ptr(pu), _ptr(pv), _stream_ptr(dev)),
                       "shw_line_esw_forward_pot")
        ctx.held = (th, cs, ct, xs, xt, pu, pv)
        ctx.dims = (B, n, m, D, L, stride, su, sv)
        ctx.theta_shape = tuple(thetas.shape)
        return cost.view(B, L)

    @staticmethod
    def backward(ctx, g):
        lib = _lib.load()
        th, cs, ct, xs, xt, pu, pv = ctx.held
        B, n, m, D, L, stride, su, sv = ctx.dims
        dev = th.device
        need = ctx.needs_input_grad
        gxs = gxt = gth = gwu = gwv = None
        w = g.to(torch.float32).contiguous()
        with torch.cuda.device(dev):
            if need[0] or need[1]:
                gxs = torch.empty(B, n, D, dtype=torch.float32, device=dev)
                gxt = torch.empty(B, m, D, dtype=torch.float32, device=dev)
                _lib.check(lib.shw_line_esw_backward_points(th.data_ptr(), cs.data_ptr(), ct.data_ptr(), w.data_ptr(), B, n,
                                                            m, D, L, stride, gxs.data_ptr(), gxt.data_ptr(),
                                                            _stream_ptr(dev)), "shw_line_esw_backward_points")
            if need[2]:
                gth = torch.empty(B, L, D, dtype=torch.float32, device=dev)
                _lib.check(lib.shw_line_esw_backward_dirs(xs.data_ptr(), xt.data_ptr(), cs.data_ptr(), ct.data_ptr(),
                                                          w.data_ptr(), B, n, m, D, L, gth.data_ptr(), _stream_ptr(dev)),
                           "shw_line_esw_backward_dirs")
                if len(ctx.theta_shape) == 2:          # directions shared by the pairs
                    gth = gth.sum(0)
        if need[3]:
            gwu = _weight_grads(pu, w, B, L, n, su == 0)
        if need[4]:
            gwv = _weight_grads(pv, w, B, L, m, sv == 0)
        return (gxs if need[0] else None), (gxt if need[1] else None), gth, gwu, gwv, None, None, None


def esw_slice_costs(Xs, Xt, thetas, p=2, u_weights=None, v_weights=None, weight_grad=False):
    """(B,n,D), (B,m,D), directions (L,D) or (B,L,D) -> (B,L): W_p^p per slice between the projected clouds, 1 <= D <= 64,
    1 <= n, m <= 4096, B <= 65535, mass-normalised (n == m, no weights: `esw_slice_sums / n`).  One fused kernel: no
    (B,L,n) key matrix.  Weights are (n,) / (m,) shared by the pairs, or (B,n) / (B,m); None is uniform.
    Differentiable w.r.t. both clouds and thetas and, with `weight_grad=True`, w.r.t. the weights (the module docstring
    says what that gradient is)."""
    _check_esw_cloud("Xs", Xs)
    _check_esw_cloud("Xt", Xt)
    if Xs.dim() != 3 or Xt.dim() != 3 or Xs.shape[0] != Xt.shape[0] or Xs.shape[2] != Xt.shape[2]:
        raise ValueError(f"the line transport needs clouds (B,n,D) and (B,m,D), got {tuple(Xs.shape)} and "
                         f"{tuple(Xt.shape)}")
    B, n, D = Xs.shape
    m = Xt.shape[1]
    for name, count in (("Xs", n), ("Xt", m)):
        if not 1 <= count <= MAX_POINTS:
            raise ValueError(f"the line transport takes 1 to {MAX_POINTS} points per cloud, {name} has {count}")
    if B > MAX_PAIRS:
        raise ValueError(f"the line transport takes at most {MAX_PAIRS} pairs per call, got {B}")
    if (not isinstance(thetas, torch.Tensor) or not thetas.is_cuda or thetas.dtype != torch.float32
            or thetas.dim() not in (2, 3) or thetas.shape[-1] != D or (thetas.dim() == 3 and thetas.shape[0] != B)):
        raise TypeError(f"thetas must be a float32 device tensor (L,{D}) or ({B},L,{D})")
    if not float(p) >= 1:
        raise ValueError(f"p must be at least 1, got {p}")
    wu, su = _check_weights("u_weights", u_weights, n, (B,), f"({B},{n})", weight_grad)
    wv, sv = _check_weights("v_weights", v_weights, m, (B,), f"({B},{m})", weight_grad)
    if torch.is_grad_enabled() and (_wants_grad(wu) or _wants_grad(wv)):
        return _LineSliceCostsWeighted.apply(Xs, Xt, thetas, wu, wv, float(p), su, sv)
    need = torch.is_grad_enabled() and (Xs.requires_grad or Xt.requires_grad or thetas.requires_grad)
    return _LineSliceCosts.apply(Xs, Xt, thetas, float(p), wu, wv, su, sv, need)


def weighted_sliced_wasserstein_distance(first_samples, second_samples, num_projection=100, p=2, device="cuda",
                                         u_weights=None, v_weights=None, weight_grad=False):
    """(n,D), (m,D) -> (mean_l W_p^p)^(1/p): `sliced_wasserstein_distance` for clouds of different size and / or with
    weights (n,), (m,).  The directions are drawn exactly as there: `rand_projections(D, num_projection)` on the CPU
    generator, then moved to `device`.  The notebook's cell sums over points; this one is mass-normalised: for n == m and
    no weights it equals `sliced_wasserstein_distance / n^(1/p)`.  `weight_grad=True`: weights that require grad receive
    gradients (`esw_slice_costs`); the direction draw itself is not differentiated."""
    dim = second_samples.size(1)
    projections = rand_projections(dim, num_projection).to(device)
    costs = esw_slice_costs(first_samples.unsqueeze(0), second_samples.unsqueeze(0), projections, p, u_weights, v_weights,
                            weight_grad)
    return torch.pow(costs.mean(), 1.0 / p)
