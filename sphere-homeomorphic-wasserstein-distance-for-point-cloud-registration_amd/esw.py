"""Euclidean sliced-Wasserstein, the notebooks' SWD baseline
(/root/reference/Wasserstein_flow_problem/Flow_cube.ipynb:275-292: `rand_projections`,
`sliced_wasserstein_distance`), on the HIP path.  Same call shape:

    sliced_wasserstein_distance(first_samples (n,D), second_samples (n,D), num_projection=100, p=2, device='cuda')

for any point dimension 1 <= D <= 64 (D = 3 on the R^3 kernels, csrc/shw_esw.hip; every other D on
csrc/shw_esw_dim.hip), and the notebooks' ASWD baseline `augmented_sliced_wassersten_distance` on top of it.

Notes on the reference cell: it draws the directions on the CPU generator and moves them to `device`
(`torch.randn((L, dim))` then `.to(device)`), which this mirror does too; it reads a *global* `num_projections`
instead of its own `num_projection` argument (a notebook slip) -- here the argument is used.  The notebook cannot
be imported (its `datas` / `losses` modules are not shipped); the cell itself is self-contained torch code and fixture
G9 (tests/golden/g9_notebook_esw.npz, oracle/make_golden.py) holds its outputs -- values and gradients -- exec'd from
the .ipynb JSON: the family is pinned by the reference (round 2).
`max_sliced_wasserstein_distance` (:294-323: Adam ascent on ONE direction, then the distance along it) is mirrored
too; the op is differentiable w.r.t. the clouds and the directions."""
from __future__ import annotations

import torch

from . import _lib
from .ssw import _stream_ptr


def rand_projections(dim, num_projections=100):
    projections = torch.randn((num_projections, dim))
    return projections / torch.sqrt(torch.sum(projections ** 2, dim=1, keepdim=True))


class _SliceSums(torch.autograd.Function):
    @staticmethod
    def forward(ctx, Xs, Xt, thetas, p, need_grad=True):
        lib = _lib.load()
        B, n, D = Xs.shape
        L = thetas.shape[-2]
        dev = Xs.device
        xs, xt, th = Xs.contiguous(), Xt.contiguous(), thetas.contiguous()
        stride = 0 if th.dim() == 2 else L * D
        sums = torch.empty(B * L, dtype=torch.float32, device=dev)
        need = need_grad
        cs = ct = None
        if need:
            cs = torch.empty(B * L * n, dtype=torch.float32, device=dev)
            ct = torch.empty(B * L * n, dtype=torch.float32, device=dev)
        cs_p, ct_p = (cs.data_ptr(), ct.data_ptr()) if need else (None, None)
        with torch.cuda.device(dev):
            if D == 3:      # the R^3 kernels, unchanged
                _lib.check(lib.shw_esw_forward(xs.data_ptr(), xt.data_ptr(), th.data_ptr(), B, n, L, stride, float(p),
                                               sums.data_ptr(), cs_p, ct_p, _stream_ptr(dev)), "shw_esw_forward")
            else:
                _lib.check(lib.shw_esw_forward_dim(xs.data_ptr(), xt.data_ptr(), th.data_ptr(), B, n, D, L, stride,
                                                   float(p), sums.data_ptr(), cs_p, ct_p, _stream_ptr(dev)),
                           "shw_esw_forward_dim")
        if need:
            ctx.save_for_backward(th, cs, ct, xs, xt)
            ctx.dims = (B, n, D, L, stride)
            ctx.theta_shape = tuple(thetas.shape)
        return sums.view(B, L)

    @staticmethod
    def backward(ctx, g):
        lib = _lib.load()
        th, cs, ct, xs, xt = ctx.saved_tensors
        B, n, D, L, stride = ctx.dims
        dev = th.device
        gxs = gxt = gth = None
        w = g.to(torch.float32).contiguous()
        with torch.cuda.device(dev):
            if ctx.needs_input_grad[0] or ctx.needs_input_grad[1]:
                gxs = torch.empty(B, n, D, dtype=torch.float32, device=dev)
                gxt = torch.empty(B, n, D, dtype=torch.float32, device=dev)
                if D == 3:
                    _lib.check(lib.shw_esw_backward_points(th.data_ptr(), cs.data_ptr(), ct.data_ptr(), w.data_ptr(), B,
                                                           n, L, stride, gxs.data_ptr(), gxt.data_ptr(),
                                                           _stream_ptr(dev)), "shw_esw_backward_points")
                else:
                    _lib.check(lib.shw_esw_backward_points_dim(th.data_ptr(), cs.data_ptr(), ct.data_ptr(), w.data_ptr(),
                                                               B, n, D, L, stride, gxs.data_ptr(), gxt.data_ptr(),
                                                               _stream_ptr(dev)), "shw_esw_backward_points_dim")
            if ctx.needs_input_grad[2]:
                gth = torch.empty(B, L, D, dtype=torch.float32, device=dev)
                if D == 3:
                    _lib.check(lib.shw_esw_backward_dirs(xs.data_ptr(), xt.data_ptr(), cs.data_ptr(), ct.data_ptr(),
                                                         w.data_ptr(), B, n, L, gth.data_ptr(), _stream_ptr(dev)),
                               "shw_esw_backward_dirs")
                else:
                    _lib.check(lib.shw_esw_backward_dirs_dim(xs.data_ptr(), xt.data_ptr(), cs.data_ptr(), ct.data_ptr(),
                                                             w.data_ptr(), B, n, D, L, gth.data_ptr(), _stream_ptr(dev)),
                               "shw_esw_backward_dirs_dim")
                if len(ctx.theta_shape) == 2:          # directions shared by the pairs
                    gth = gth.sum(0)
        return gxs, gxt, gth, None, None


MAX_DIM = 64          # include/shw.h shw_esw_*_dim
MAX_POINTS = 4096


def _check_esw_cloud(name, t):
    """ESW's own check: any point dimension 1..MAX_DIM (the spherical path's _check_cloud stays R^3 only)."""
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{name} must be a torch.Tensor")
    if not t.is_cuda:
        raise RuntimeError(f"{name} is on {t.device}: the MI355X HIP path needs device tensors (no CPU fallback)")
    if t.dtype != torch.float32:
        raise TypeError(f"{name} must be float32, got {t.dtype}")
    if t.dim() >= 1 and not 1 <= t.shape[-1] <= MAX_DIM:
        raise ValueError(f"{name} must have 1 to {MAX_DIM} coordinates per point, got shape {tuple(t.shape)}")


def esw_slice_sums(Xs, Xt, thetas, p=2):
    """(B,n,D), (B,n,D), directions (L,D) or (B,L,D) -> (B,L) per-slice sums of |sorted difference|^p.
    1 <= D <= 64; D = 3 runs the R^3 kernels, every other D the D-generic ones (include/shw.h shw_esw_*_dim)."""
    _check_esw_cloud("Xs", Xs)
    _check_esw_cloud("Xt", Xt)
    if Xs.shape != Xt.shape or Xs.dim() != 3:
        raise ValueError("the Euclidean sliced distance needs two (B,n,D) clouds of equal size")
    D = Xs.shape[-1]
    if D != 3 and Xs.shape[1] > MAX_POINTS:
        raise ValueError(f"the Euclidean sliced distance takes at most {MAX_POINTS} points per cloud, got {Xs.shape[1]}")
    if not thetas.is_cuda or thetas.dtype != torch.float32 or thetas.shape[-1] != D:
        raise TypeError(f"thetas must be a float32 device tensor (L,{D}) or (B,L,{D})")
    need = torch.is_grad_enabled() and (Xs.requires_grad or Xt.requires_grad or thetas.requires_grad)
    return _SliceSums.apply(Xs, Xt, thetas, float(p), need)


def sliced_wasserstein_distance(first_samples, second_samples, num_projection=100, p=2, device="cuda"):
    dim = second_samples.size(1)
    projections = rand_projections(dim, num_projection).to(device)
    sums = esw_slice_sums(first_samples.unsqueeze(0), second_samples.unsqueeze(0), projections, p)
    return torch.pow(sums.mean(), 1.0 / p)


def max_sliced_wasserstein_distance(first_samples, second_samples, num_projection=100, p=2, max_iter=10, device="cuda"):
    """Flow_cube.ipynb:294-323: one direction, `max_iter` Adam ascent steps on it (lr 0.005, betas (0.999, 0.999),
    re-normalised after every step) against the detached clouds, then the distance along the final direction."""
    dim = second_samples.size(1)
    first_d, second_d = first_samples.detach().unsqueeze(0), second_samples.detach().unsqueeze(0)
    projections = rand_projections(dim, 1).to(device)
    projections.requires_grad_()
    optimizer = torch.optim.Adam([projections], lr=0.005, betas=(0.999, 0.999))
    for _ in range(max_iter):
        dist_l = torch.pow(esw_slice_sums(first_d, second_d, projections, p).mean(), 1.0 / p)
        optimizer.zero_grad()
        (-dist_l).backward()
        optimizer.step()
        projections.data = projections.data / torch.sqrt(torch.sum(projections.data ** 2, dim=1))
    sums = esw_slice_sums(first_samples.unsqueeze(0), second_samples.unsqueeze(0), projections.detach(), p)
    return torch.pow(sums.mean(), 1.0 / p)


def _directions_on(dim, num_projections, device):
    """rand_projections(dim, L) from the global CPU generator (the notebook cell's draw, same sequence), copied to
    `device` without stalling the host: staged in pinned memory and copied with non_blocking."""
    projections = rand_projections(dim, num_projections)
    if torch.device(device).type != "cuda":
        return projections.to(device)
    return projections.pin_memory().to(device, non_blocking=True)


def augmented_sliced_wassersten_distance(first_samples, second_samples, num_projections, phi, phi_op, p=2, max_iter=10,
                                         lam=20, device="cuda", net_type="fc"):
    """The notebooks' ASWD baseline (Flow_cube.ipynb, the cell that starts with `def rand_projections`; run by every
    gradient-flow notebook as functions=[..., "ASWD", ...]): sliced-W of the clouds augmented by the caller's module
    `phi` (the notebook's Mapping(3): x -> cat(x, Linear(x)), 6 coordinates).  Same signature and spelling as the cell.

    `max_iter` ascent steps of `phi_op` on phi against the detached clouds, each with loss
    lam * (|phi x| + |phi y|).mean() - (mean_l S_l * 512 / n)^(1/p), then one final evaluation (mean_l S_l)^(1/p),
    differentiable w.r.t. both clouds and phi's parameters.  Every evaluation draws rand_projections(D', L) from the
    global CPU generator, D' = phi's output width, in the cell's order.  `net_type` is accepted and unused, as in the
    cell.  The sorts and their gradients run on the D-generic HIP kernels (esw_slice_sums)."""
    first_samples_detach = first_samples.detach()
    second_samples_detach = second_samples.detach()
    for _ in range(max_iter):
        first_samples_transform = phi(first_samples_detach)
        second_samples_transform = phi(second_samples_detach)
        reg = lam * (torch.norm(first_samples_transform, p=2, dim=1)
                     + torch.norm(second_samples_transform, p=2, dim=1)).mean()
        projections = _directions_on(first_samples_transform.shape[-1], num_projections, device)
        sums = esw_slice_sums(first_samples_transform.unsqueeze(0), second_samples_transform.unsqueeze(0), projections,
                              p)[0]
        wasserstein_distance = sums * 512 / first_samples_detach.shape[0]
        wasserstein_distance = torch.pow(wasserstein_distance.mean(), 1.0 / p)
        loss = reg - wasserstein_distance
        phi_op.zero_grad()
        loss.backward()
        phi_op.step()
    first_samples_transform = phi(first_samples)
    second_samples_transform = phi(second_samples)
    projections = _directions_on(first_samples_transform.shape[-1], num_projections, device)
    sums = esw_slice_sums(first_samples_transform.unsqueeze(0), second_samples_transform.unsqueeze(0), projections, p)
    return torch.pow(sums.mean(), 1.0 / p)


augmented_sliced_wasserstein_distance = augmented_sliced_wassersten_distance
