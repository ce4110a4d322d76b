"""Generalised sliced-Wasserstein: the rest of the notebooks' sliced family (Wasserstein_flow_problem/Flow_cube.ipynb,
the cell that starts with `def rand_projections`) on the HIP path -- GSWD with the circular and the polynomial defining
function, their max- variants, the network-defined gsw_nn / max_gsw_nn, and the distributional DSWD.

Every member maps a point and a parameter to a scalar key, sorts both clouds' keys per slice and sums
|sorted difference|^p.  Three lower-level ops carry that (csrc/shw_gsw.hip, include/shw.h shw_gsw_*):

    sorted_row_sums(u_rows, v_rows, p)                   rows of keys the caller computed (any defining function)
    gsw_circular_slice_sums(Xs, Xt, thetas, r, p)        g(x, theta) = |x - r theta|, keys formed inside the kernel
    gsw_polynomial_slice_sums(Xs, Xt, coefficient, degree, p)   monomial features in torch, then esw_slice_sums

and the cell's call shapes sit on top with the cell's names, argument order and defaults.  Every function returns
(mean_l S_l)^(1/p), S_l a SUM over points.  Where the cell draws from the CPU generator (GSWD_circular,
max_GSWD_circular, DSWD) so does the mirror, draw for draw; the three polynomial functions draw on `device`, and take a
keyword-only `coefficient=` (the raw draw, before the cell's normalisation) so that a CPU-made fixture can drive them.
One deliberate deviation: a point exactly at r theta has a zero circular key, where the cell's sqrt yields a NaN
gradient; here it contributes gradient 0.  The cell's TransformNet, MLP and Mapping are the caller's modules and are not
shipped."""
from __future__ import annotations

from itertools import combinations

import torch

from . import _lib
from .esw import MAX_DIM, MAX_POINTS, _check_esw_cloud, _directions_on, esw_slice_sums, rand_projections
from .ssw import _stream_ptr


# ----------------------------------------------------------------------------------------------- rows of keys
class _RowSums(torch.autograd.Function):
    @staticmethod
    def forward(ctx, u, v, p, need_grad):
        lib = _lib.load()
        rows, n = u.shape
        dev = u.device
        sums = torch.empty(rows, dtype=torch.float32, device=dev)
        cu = cv = None
        if need_grad:
            cu = torch.empty(rows, n, dtype=torch.float32, device=dev)
            cv = torch.empty(rows, n, dtype=torch.float32, device=dev)
        cu_p, cv_p = (cu.data_ptr(), cv.data_ptr()) if need_grad else (None, None)
        with torch.cuda.device(dev):
            _lib.check(lib.shw_gsw_rows_forward(u.data_ptr(), v.data_ptr(), rows, n, float(p), sums.data_ptr(), cu_p, cv_p,
                                                _stream_ptr(dev)), "shw_gsw_rows_forward")
        if need_grad:
            ctx.save_for_backward(cu, cv)
        return sums

    @staticmethod
    def backward(ctx, g):
        cu, cv = ctx.saved_tensors
        w = g.to(torch.float32).unsqueeze(-1)
        return (cu * w if ctx.needs_input_grad[0] else None), (cv * w if ctx.needs_input_grad[1] else None), None, None


def _check_rows(name, t):
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{name} must be a torch.Tensor")
    if not t.is_cuda:
        raise RuntimeError(f"{name} is on {t.device}: the MI355X HIP path needs device tensors (no CPU fallback)")
    if t.dtype != torch.float32:
        raise TypeError(f"{name} must be float32, got {t.dtype}")
    if t.dim() < 1 or not 1 <= t.shape[-1] <= MAX_POINTS:
        raise ValueError(f"{name} must hold 1 to {MAX_POINTS} keys per row, got shape {tuple(t.shape)}")


def sorted_row_sums(u_rows, v_rows, p=2):
    """(..., n), (..., n) -> (...): sum_i |u_(i) - v_(i)|^p of every row pair, u_(.) and v_(.) sorted ascending.
    The keys are the caller's (a network's transposed output, any defining function); non-contiguous rows are made
    contiguous, and the gradient comes back through autograd in the caller's layout."""
    _check_rows("u_rows", u_rows)
    _check_rows("v_rows", v_rows)
    if u_rows.shape != v_rows.shape:
        raise ValueError(f"the sorted difference needs rows of equal shape, got {tuple(u_rows.shape)} and "
                         f"{tuple(v_rows.shape)}")
    if not float(p) >= 1:
        raise ValueError(f"p must be at least 1, got {p}")
    lead, n = u_rows.shape[:-1], u_rows.shape[-1]
    need = torch.is_grad_enabled() and (u_rows.requires_grad or v_rows.requires_grad)
    u = u_rows.reshape(-1, n).contiguous()
    v = v_rows.reshape(-1, n).contiguous()
    return _RowSums.apply(u, v, float(p), need).reshape(lead)


# ----------------------------------------------------------------------------------------------- circular, fused
class _CircularSliceSums(torch.autograd.Function):
    @staticmethod
    def forward(ctx, Xs, Xt, thetas, r, p, need_grad):
        lib = _lib.load()
        B, n, D = Xs.shape
        L = thetas.shape[-2]
        dev = Xs.device
        xs, xt, th = Xs.contiguous(), Xt.contiguous(), thetas.contiguous()
        stride = 0 if th.dim() == 2 else L * D
        sums = torch.empty(B * L, dtype=torch.float32, device=dev)
        cs = ct = None
        if need_grad:
            cs = torch.empty(B * L * n, dtype=torch.float32, device=dev)
            ct = torch.empty(B * L * n, dtype=torch.float32, device=dev)
        cs_p, ct_p = (cs.data_ptr(), ct.data_ptr()) if need_grad else (None, None)
        with torch.cuda.device(dev):
            _lib.check(lib.shw_gsw_circular_forward(xs.data_ptr(), xt.data_ptr(), th.data_ptr(), B, n, D, L, stride,
                                                    float(r), float(p), sums.data_ptr(), cs_p, ct_p, _stream_ptr(dev)),
                       "shw_gsw_circular_forward")
        if need_grad:
            ctx.save_for_backward(th, cs, ct, xs, xt)
            ctx.dims = (B, n, D, L, stride, float(r))
            ctx.theta_shape = tuple(thetas.shape)
        return sums.view(B, L)

    @staticmethod
    def backward(ctx, g):
        lib = _lib.load()
        th, cs, ct, xs, xt = ctx.saved_tensors
        B, n, D, L, stride, r = ctx.dims
        dev = th.device
        gxs = gxt = gth = None
        w = g.to(torch.float32).contiguous()
        with torch.cuda.device(dev):
            if ctx.needs_input_grad[0] or ctx.needs_input_grad[1]:
                gxs = torch.empty(B, n, D, dtype=torch.float32, device=dev)
                gxt = torch.empty(B, n, D, dtype=torch.float32, device=dev)
                _lib.check(lib.shw_gsw_circular_backward_points(xs.data_ptr(), xt.data_ptr(), th.data_ptr(), cs.data_ptr(),
                                                                ct.data_ptr(), w.data_ptr(), B, n, D, L, stride, r,
                                                                gxs.data_ptr(), gxt.data_ptr(), _stream_ptr(dev)),
                           "shw_gsw_circular_backward_points")
            if ctx.needs_input_grad[2]:
                gth = torch.empty(B, L, D, dtype=torch.float32, device=dev)
                _lib.check(lib.shw_gsw_circular_backward_dirs(xs.data_ptr(), xt.data_ptr(), th.data_ptr(), cs.data_ptr(),
                                                              ct.data_ptr(), w.data_ptr(), B, n, D, L, stride, r,
                                                              gth.data_ptr(), _stream_ptr(dev)),
                           "shw_gsw_circular_backward_dirs")
                if len(ctx.theta_shape) == 2:          # directions shared by the pairs
                    gth = gth.sum(0)
        return gxs, gxt, gth, None, None, None


def gsw_circular_slice_sums(Xs, Xt, thetas, r=1.0, p=2):
    """(B,n,D), (B,n,D), thetas (L,D) or (B,L,D) -> (B,L) per-slice sums of |sorted key difference|^p with the circular
    defining function key = |x - r theta|_2, 1 <= D <= 64, n <= 4096.  One fused kernel: no (B,L,n) key matrix.
    Differentiable w.r.t. both clouds and thetas; a point exactly at r theta contributes gradient 0."""
    _check_esw_cloud("Xs", Xs)
    _check_esw_cloud("Xt", Xt)
    if Xs.shape != Xt.shape or Xs.dim() != 3:
        raise ValueError("the generalised sliced distance needs two (B,n,D) clouds of equal size")
    B, n, D = Xs.shape
    if not 1 <= n <= MAX_POINTS:
        raise ValueError(f"the generalised sliced distance takes 1 to {MAX_POINTS} points per cloud, got {n}")
    if B > 65535:
        raise ValueError(f"the generalised sliced distance takes at most 65535 pairs per call, got {B}")
    if (not isinstance(thetas, torch.Tensor) or not thetas.is_cuda or thetas.dtype != torch.float32
            or thetas.dim() not in (2, 3) or thetas.shape[-1] != D or (thetas.dim() == 3 and thetas.shape[0] != B)):
        raise TypeError(f"thetas must be a float32 device tensor (L,{D}) or ({B},L,{D})")
    if not float(p) >= 1:
        raise ValueError(f"p must be at least 1, got {p}")
    need = torch.is_grad_enabled() and (Xs.requires_grad or Xt.requires_grad or thetas.requires_grad)
    return _CircularSliceSums.apply(Xs, Xt, thetas, float(r), float(p), need)


# ----------------------------------------------------------------------------------------------- polynomial
def poly_degree(degree, dim):
    """Exponent rows of the homogeneous monomials of `degree` in `dim` variables, (count, dim) float32, in the cell's
    order: the dim - 1 bars among degree + dim - 1 slots in lexicographic order, an exponent = the gap between bars."""
    rows = []
    for bars in combinations(range(1, degree + dim), dim - 1):
        edges = (0,) + bars + (degree + dim,)
        rows.append([edges[j + 1] - edges[j] - 1 for j in range(dim)])
    return torch.tensor(rows, dtype=torch.float32)


def _monomials(X, exponents):
    """(..., n, D), (F, D) -> (..., n, F): prod_d x_d ^ e_d, as the cell's polynomial_function forms them"""
    return torch.prod(X.unsqueeze(-2) ** exponents, dim=-1)


def gsw_polynomial_slice_sums(Xs, Xt, coefficient, degree, p=2):
    """(B,n,D), (B,n,D), coefficient (F,L) in the cell's layout -> (B,L): the polynomial defining function
    key = sum_f coefficient[f,l] * monomial_f(x), F = the number of degree-`degree` monomials in D variables (10 for
    degree 3 in R^3, 21 for degree 5).  The monomials are torch; the keys, sorts and sums run on the Euclidean HIP
    kernels (esw_slice_sums), whose limit of 64 coordinates bounds F."""
    if Xs.dim() != 3 or Xs.shape != Xt.shape:
        raise ValueError("the generalised sliced distance needs two (B,n,D) clouds of equal size")
    exponents = poly_degree(degree, Xs.shape[-1])
    count = exponents.shape[0]
    if count > MAX_DIM:
        raise ValueError(f"degree {degree} in {Xs.shape[-1]} variables has {count} monomials: the polynomial defining "
                         f"function takes at most {MAX_DIM}")
    if coefficient.dim() != 2 or coefficient.shape[0] != count:
        raise ValueError(f"coefficient must be ({count}, L) for degree {degree} in {Xs.shape[-1]} variables, got "
                         f"{tuple(coefficient.shape)}")
    exponents = exponents.to(Xs.device)
    return esw_slice_sums(_monomials(Xs, exponents), _monomials(Xt, exponents), coefficient.transpose(0, 1), p)


def _outer(sums, p):
    return torch.pow(sums.mean(), 1.0 / p)


def _unit_columns(c):
    return c / torch.sqrt(torch.sum(c ** 2, dim=0))


def _drawn_coefficient(count, num_projection, device, coefficient):
    if coefficient is None:
        return torch.randn((count, num_projection), device=device)
    if tuple(coefficient.shape) != (count, num_projection):
        raise ValueError(f"coefficient must be ({count}, {num_projection}), got {tuple(coefficient.shape)}")
    return coefficient.detach().to(device=device, dtype=torch.float32).clone()


def GSWD_polynomial(encoded_samples, distribution_samples, p=2, num_projection=100, degree=5, device="cuda", *,
                    coefficient=None):
    count = poly_degree(degree, encoded_samples.shape[-1]).shape[0]
    coefficient_1 = _unit_columns(_drawn_coefficient(count, num_projection, device, coefficient))
    sums = gsw_polynomial_slice_sums(encoded_samples.unsqueeze(0), distribution_samples.unsqueeze(0), coefficient_1,
                                     degree, p)
    return _outer(sums, p)


def _max_GSWD_polynomial(encoded_samples, distribution_samples, p, degree, device, max_iter, coefficient):
    """one coefficient column, `max_iter` Adam ascent steps on it against the detached clouds (lr 0.005, betas
    (0.999, 0.999), columns re-normalised after every step), then the distance along the final coefficient"""
    count = poly_degree(degree, encoded_samples.shape[-1]).shape[0]
    coefficient_1 = _unit_columns(_drawn_coefficient(count, 1, device, coefficient))
    coefficient_1.requires_grad_()
    first_d, second_d = encoded_samples.detach().unsqueeze(0), distribution_samples.detach().unsqueeze(0)
    optimizer = torch.optim.Adam([coefficient_1], lr=0.005, betas=(0.999, 0.999))
    for _ in range(max_iter):
        dist = _outer(gsw_polynomial_slice_sums(first_d, second_d, coefficient_1, degree, p), p)
        optimizer.zero_grad()
        (-dist).backward()
        optimizer.step()
        coefficient_1.data = _unit_columns(coefficient_1.data)
    sums = gsw_polynomial_slice_sums(encoded_samples.unsqueeze(0), distribution_samples.unsqueeze(0),
                                     coefficient_1.detach(), degree, p)
    return _outer(sums, p), coefficient_1.detach()


def max_GSWD_polynomial_3(encoded_samples, distribution_samples, p=2, num_projection=100, degree=3, device="cuda",
                          max_iter=10, *, coefficient=None):
    """`num_projection` is accepted and forced to 1, as in the cell."""
    return _max_GSWD_polynomial(encoded_samples, distribution_samples, p, degree, device, max_iter, coefficient)[0]


def max_GSWD_polynomial_5(encoded_samples, distribution_samples, p=2, num_projection=100, degree=5, device="cuda",
                          max_iter=10, *, coefficient=None):
    """`num_projection` is accepted and forced to 1, as in the cell."""
    return _max_GSWD_polynomial(encoded_samples, distribution_samples, p, degree, device, max_iter, coefficient)[0]


# ----------------------------------------------------------------------------------------------- circular call shapes
def GSWD_circular(encoded_samples, distribution_samples, p=2, num_projection=100, r=1, device="cuda"):
    theta = _directions_on(encoded_samples.shape[1], num_projection, device)
    sums = gsw_circular_slice_sums(encoded_samples.unsqueeze(0), distribution_samples.unsqueeze(0), theta, r, p)
    return _outer(sums, p)


def _max_GSWD_circular(encoded_samples, distribution_samples, p, r, device, max_iter):
    theta = _directions_on(encoded_samples.shape[1], 1, device)
    theta.requires_grad_()
    first_d, second_d = encoded_samples.detach().unsqueeze(0), distribution_samples.detach().unsqueeze(0)
    optimizer = torch.optim.Adam([theta], lr=0.005, betas=(0.999, 0.999))
    for _ in range(max_iter):
        dist = _outer(gsw_circular_slice_sums(first_d, second_d, theta, r, p), p)     # r rides on theta: theta * r
        optimizer.zero_grad()
        (-dist).backward()
        optimizer.step()
        theta.data = theta.data / torch.sqrt(torch.sum(theta.data ** 2, dim=1))
    sums = gsw_circular_slice_sums(encoded_samples.unsqueeze(0), distribution_samples.unsqueeze(0), theta.detach(), r, p)
    return _outer(sums, p), theta.detach()


def max_GSWD_circular(encoded_samples, distribution_samples, p=2, num_projection=1, r=1, device="cuda", max_iter=10):
    """One theta from the CPU generator, `max_iter` Adam ascent steps on it (the gradient passes through theta * r, as
    in the cell), re-normalised after every step; `num_projection` is accepted and forced to 1."""
    return _max_GSWD_circular(encoded_samples, distribution_samples, p, r, device, max_iter)[0]


# ----------------------------------------------------------------------------------------------- network-defined
def _net_distance(first_samples, second_samples, net, p):
    return _outer(sorted_row_sums(net(first_samples).transpose(0, 1), net(second_samples).transpose(0, 1), p), p)


def gsw_nn_1(first_samples, second_samples, net, net_op, max_iter=10, p=2):
    """`net_op` and `max_iter` are accepted and unused, as in the cell."""
    return _net_distance(first_samples, second_samples, net, p)


def max_gsw_nn_1(first_samples, second_samples, net, net_op, max_iter=10, p=2):
    """`max_iter` ascent steps of `net_op` on the caller's `net` against the detached clouds, then the distance."""
    first_d, second_d = first_samples.detach(), second_samples.detach()
    for _ in range(max_iter):
        loss = -_net_distance(first_d, second_d, net, p)
        net_op.zero_grad()
        loss.backward()
        net_op.step()
    return _net_distance(first_samples, second_samples, net, p)


gsw_nn_3 = gsw_nn_1              # the cell defines both pairs with the same body
max_gsw_nn_3 = max_gsw_nn_1


# ----------------------------------------------------------------------------------------------- DSWD
def cosine_distance_torch(x1, x2=None, eps=1e-8):
    """mean_ij |cos(x1_i, x2_j)|; the product of the two norms is clamped from below at eps (x2 defaults to x1)"""
    other = x1 if x2 is None else x2
    norms = torch.linalg.vector_norm(x1, dim=1).unsqueeze(1) * torch.linalg.vector_norm(other, dim=1).unsqueeze(0)
    return (x1 @ other.transpose(0, 1)).div(norms.clamp_min(eps)).abs().mean()


def distributional_sliced_wasserstein_distance(first_samples, second_samples, num_projections, f, f_op, p=2, max_iter=10,
                                               lam=1, device="cuda"):
    """The notebooks' DSWD: directions f(pro), pro ~ rand_projections from the CPU generator, f the caller's module
    (the cell's TransformNet).  One draw is made and discarded before the loop (as in the cell), then one per ascent
    step and one for the final evaluation: max_iter + 2 draws.  Every ascent step of `f_op` minimises
    lam * cosine_distance_torch(f(pro), f(pro)) - (mean_l S_l)^(1/p) on the detached clouds; the slice sums and their
    gradient w.r.t. the directions run on the Euclidean HIP kernels."""
    dim = first_samples.size(1)
    rand_projections(dim, num_projections)          # the cell's first draw, never used: only the generator moves
    first_d, second_d = first_samples.detach().unsqueeze(0), second_samples.detach().unsqueeze(0)
    for _ in range(max_iter):
        projections = f(_directions_on(dim, num_projections, device))
        reg = lam * cosine_distance_torch(projections, projections)
        loss = reg - _outer(esw_slice_sums(first_d, second_d, projections, p), p)
        f_op.zero_grad()
        loss.backward()
        f_op.step()
    projections = f(_directions_on(dim, num_projections, device))
    return _outer(esw_slice_sums(first_samples.unsqueeze(0), second_samples.unsqueeze(0), projections, p), p)
