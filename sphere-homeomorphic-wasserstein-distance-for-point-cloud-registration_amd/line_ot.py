"""Exact 1-D optimal transport between two weighted empirical measures on the line, on the HIP path
(csrc/shw_line_ot.hip, include/shw.h shw_line_*): the Euclidean sliced family for clouds of different size and for
weighted clouds -- what `sliced_cost` / `binary_search_circle` already do on the sphere.

    line_ot_rows(u_rows, v_rows, p, u_weights, v_weights)           rows of keys the caller computed (any defining function)
    esw_slice_costs(Xs, Xt, thetas, p, u_weights, v_weights)        keys x . theta formed inside the kernel
    weighted_sliced_wasserstein_distance(first, second, ...)        the notebook's SWD call shape on top

A row has values u_1..u_n with weights a_i >= 0 and values v_1..v_m with weights b_j >= 0; the kernel divides the weights
by their sums, `None` means uniform.  The cost is W_p^p = int_0^1 |F_u^-1(t) - F_v^-1(t)|^p dt (the quantile merge) for
any real p >= 1.  It is MASS-NORMALISED: for n == m and no weights it equals `sorted_row_sums / n` (`esw_slice_sums / n`),
which sum over points.  An atom of weight 0 contributes nothing and receives gradient 0, so a padded batch is evaluated
with zero-weight padding.  Gradients are with respect to the values (both sides, and the directions of the fused op);
there is no gradient with respect to the weights, and a weight tensor that requires grad is refused.  Weights must be
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


def _check_weights(name, w, count, lead, lead_name):
    """None, (count,) shared, or lead + (count,) -> (contiguous tensor or None, stride in floats)"""
    if w is None:
        return None, 0
    if not isinstance(w, torch.Tensor):
        raise TypeError(f"{name} must be a torch.Tensor or None")
    if not w.is_cuda:
        raise RuntimeError(f"{name} is on {w.device}: the MI355X HIP path needs device tensors (no CPU fallback)")
    if w.dtype != torch.float32:
        raise TypeError(f"{name} must be float32, got {w.dtype}")
    if w.requires_grad:
        raise ValueError(f"{name} requires grad: the line transport has no gradient with respect to the weights "
                         "(detach them)")
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


def line_ot_rows(u_rows, v_rows, p=2, u_weights=None, v_weights=None):
    """(..., n), (..., m) -> (...): W_p^p between the two weighted empirical measures of every row pair, 1 <= n, m <= 4096,
    mass-normalised (n == m, no weights: `sorted_row_sums / n`).  The keys are the caller's -- a circular or polynomial
    defining function, a network's output -- so this carries the generalised sliced family at n != m.  Weights are
    (n,) / (m,) shared by all rows, or the rows' own shape; None is uniform.  Differentiable w.r.t. both row tensors."""
    _check_rows("u_rows", u_rows)
    _check_rows("v_rows", v_rows)
    if u_rows.shape[:-1] != v_rows.shape[:-1]:
        raise ValueError(f"the line transport pairs rows: leading shapes must agree, got {tuple(u_rows.shape)} and "
                         f"{tuple(v_rows.shape)}")
    if not float(p) >= 1:
        raise ValueError(f"p must be at least 1, got {p}")
    lead, n, m = u_rows.shape[:-1], u_rows.shape[-1], v_rows.shape[-1]
    wu, su = _check_weights("u_weights", u_weights, n, lead, f"u_rows' shape {tuple(u_rows.shape)}")
    wv, sv = _check_weights("v_weights", v_weights, m, lead, f"v_rows' shape {tuple(v_rows.shape)}")
    need = torch.is_grad_enabled() and (u_rows.requires_grad or v_rows.requires_grad)
    u = u_rows.reshape(-1, n).contiguous()
    v = v_rows.reshape(-1, m).contiguous()
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


def esw_slice_costs(Xs, Xt, thetas, p=2, u_weights=None, v_weights=None):
    """(B,n,D), (B,m,D), directions (L,D) or (B,L,D) -> (B,L): W_p^p per slice between the projected clouds, 1 <= D <= 64,
    1 <= n, m <= 4096, B <= 65535, mass-normalised (n == m, no weights: `esw_slice_sums / n`).  One fused kernel: no
    (B,L,n) key matrix.  Weights are (n,) / (m,) shared by the pairs, or (B,n) / (B,m); None is uniform.
    Differentiable w.r.t. both clouds and thetas."""
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
    wu, su = _check_weights("u_weights", u_weights, n, (B,), f"({B},{n})")
    wv, sv = _check_weights("v_weights", v_weights, m, (B,), f"({B},{m})")
    need = torch.is_grad_enabled() and (Xs.requires_grad or Xt.requires_grad or thetas.requires_grad)
    return _LineSliceCosts.apply(Xs, Xt, thetas, float(p), wu, wv, su, sv, need)


def weighted_sliced_wasserstein_distance(first_samples, second_samples, num_projection=100, p=2, device="cuda",
                                         u_weights=None, v_weights=None):
    """(n,D), (m,D) -> (mean_l W_p^p)^(1/p): `sliced_wasserstein_distance` for clouds of different size and / or with
    weights (n,), (m,).  The directions are drawn exactly as there: `rand_projections(D, num_projection)` on the CPU
    generator, then moved to `device`.  The notebook's cell sums over points; this one is mass-normalised: for n == m and
    no weights it equals `sliced_wasserstein_distance / n^(1/p)`."""
    dim = second_samples.size(1)
    projections = rand_projections(dim, num_projection).to(device)
    costs = esw_slice_costs(first_samples.unsqueeze(0), second_samples.unsqueeze(0), projections, p, u_weights, v_weights)
    return torch.pow(costs.mean(), 1.0 / p)
