"""The sphere encoder of the phi-max wrappers: `transform_to_sphere` (max_spherical_sliced_w.py:334-350) and
`transform_to_sphere_fast` (max_spherical_sliced_w_fast.py:323-338), with the per-point network and the angle map on the
HIP path (csrc/shw_sphere_map.hip, include/shw.h shw_sphere_map_*).

    sphere_map(x, params)             the fused op: one forward kernel, one recomputing backward kernel (+ a small reduction)
    sphere_map_composed(x, params)    the same math in torch operations (any device / dtype)
    transform_to_sphere()             the reference's module, its state-dict layout; transform_to_sphere_fast the same

Per point: z1 = tanh(W1 x + b1), z2 = tanh(W2 z1 + b2), o = W3 z2 + b3, theta1 = pi (tanh(o0) / 2 + 1/2),
theta2 = pi tanh(o1), y = (sin theta1 cos theta2, sin theta1 sin theta2, cos theta1).

PARAMETERS, the kernels' input: one flat buffer of 142 values in state-dict order -- W1 row-major (16, 3), b1, W2 (4, 16),
b2, W3 (2, 4), b3 -- which is one `torch.cat` of the six tensors; autograd splits the buffer's gradient back.
"""
from __future__ import annotations

import math

import torch
import torch.nn.functional as F
from torch import nn

from . import _lib
from .ssw import _stream_ptr

POINT_DIM, HIDDEN1, HIDDEN2, ANGLES = 3, 16, 4, 2                   # include/shw.h shw_sphere_map_supported
_SHAPES = ((HIDDEN1, POINT_DIM), (HIDDEN1,), (HIDDEN2, HIDDEN1), (HIDDEN2,), (ANGLES, HIDDEN2), (ANGLES,))
PARAM_COUNT = sum(math.prod(s) for s in _SHAPES)                    # 142


def sphere_map_composed(x, params):
    """(..., 3) points, the flat parameter buffer (142,) -> (..., 3) unit vectors, in the torch operations of the
    reference's forward (:345-348), on any device and dtype (x and the parameters of one dtype).  The fallback of the
    module and the reference of the tests."""
    if params.dim() != 1 or params.numel() != PARAM_COUNT:
        raise ValueError(f"params must have shape ({PARAM_COUNT},), got {tuple(params.shape)}")
    if x.shape[-1] != POINT_DIM:
        raise ValueError(f"the sphere map takes points of dimension {POINT_DIM}, got x of shape {tuple(x.shape)}")
    w1, b1, w2, b2, w3, b3 = (t.view(s) for t, s in zip(params.split([math.prod(s) for s in _SHAPES]), _SHAPES))
    o = F.linear(torch.tanh(F.linear(torch.tanh(F.linear(x, w1, b1)), w2, b2)), w3, b3)
    return _angle_map(o)


def _angle_map(o):
    theta_1 = math.pi * (torch.tanh(o[..., 0]) / 2 + 0.5)
    theta_2 = math.pi * torch.tanh(o[..., 1])
    return torch.stack([torch.sin(theta_1) * torch.cos(theta_2), torch.sin(theta_1) * torch.sin(theta_2),
                        torch.cos(theta_1)], dim=-1)


class _SphereMap(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, params):
        lib = _lib.load()
        dev = x.device
        y = torch.empty_like(x)
        with torch.cuda.device(dev):
            _lib.check(lib.shw_sphere_map_forward(x.data_ptr(), params.data_ptr(), x.numel() // POINT_DIM, y.data_ptr(),
                                                  _stream_ptr(dev)), "shw_sphere_map_forward")
        ctx.save_for_backward(x, params)
        return y

    @staticmethod
    def backward(ctx, gy):
        lib = _lib.load()
        x, params = ctx.saved_tensors
        dev = x.device
        points = x.numel() // POINT_DIM
        gy = gy.to(torch.float32).contiguous()
        gx = torch.empty_like(x) if ctx.needs_input_grad[0] else None
        gp = work = None
        if ctx.needs_input_grad[1]:
            gp = torch.empty_like(params)
            work = torch.empty(max(lib.shw_sphere_map_workspace_bytes(points) // 4, 1), dtype=torch.float32, device=dev)
        with torch.cuda.device(dev):
            _lib.check(lib.shw_sphere_map_backward(x.data_ptr(), params.data_ptr(), gy.data_ptr(), points,
                                                   None if gx is None else gx.data_ptr(),
                                                   None if gp is None else gp.data_ptr(),
                                                   None if work is None else work.data_ptr(), _stream_ptr(dev)),
                       "shw_sphere_map_backward")
        return gx, gp


def sphere_map(x, params):
    """(N, 3) or (B, N, 3) float32 device points, the flat parameter buffer (142,) -> the points on the unit sphere, same
    shape.  One kernel forward, one (plus a small reduction) backward; differentiable w.r.t. the points and w.r.t. the
    parameters, and only the gradients that are needed are computed.  The parameter gradient is summed without atomics:
    the same bits on every run.  Nothing is saved but x and the parameters; all allocation is torch's and nothing
    synchronises, so the op can be captured in a graph."""
    for name, t in (("x", x), ("params", params)):
        if not isinstance(t, torch.Tensor):
            raise TypeError(f"{name} must be a torch.Tensor")
        if not t.is_cuda:
            raise RuntimeError(f"{name} is on {t.device}: the MI355X HIP path needs device tensors "
                               "(sphere_map_composed runs anywhere)")
        if t.dtype != torch.float32:
            raise TypeError(f"{name} must be float32, got {t.dtype}")
    if x.dim() not in (2, 3) or x.shape[-1] != POINT_DIM:
        raise ValueError(f"the fused sphere map takes (N, {POINT_DIM}) or (B, N, {POINT_DIM}) points; got x of shape "
                         f"{tuple(x.shape)}")
    if params.dim() != 1 or params.numel() != PARAM_COUNT:
        raise ValueError(f"params must have shape ({PARAM_COUNT},), got {tuple(params.shape)}")
    if params.device != x.device:
        raise ValueError("x and params must be on one device")
    return _SphereMap.apply(x.contiguous(), params.contiguous())


class transform_to_sphere(nn.Module):
    """`transform_to_sphere()` of max_spherical_sliced_w.py:334-350: forward(x) maps (B, N, 3) points onto the unit sphere.
    One member, `net = Sequential(Linear(3, 16), Tanh, Linear(16, 4), Tanh, Linear(4, 2))` with nn.Linear's default
    initialisation, so the state-dict keys (`net.0.weight` ... `net.4.bias`), the values drawn from a seed and the order of
    `parameters()` are the reference's.  A float32 device input takes the fused path (`sphere_map`); CPU, float64,
    `self.fused = False`, or a `net` edited to other widths or activations, the composed one."""

    def __init__(self):
        super().__init__()
        self.fused = True
        self.net = nn.Sequential(nn.Linear(POINT_DIM, HIDDEN1), nn.Tanh(), nn.Linear(HIDDEN1, HIDDEN2), nn.Tanh(),
                                 nn.Linear(HIDDEN2, ANGLES))

    def _is_reference_net(self):
        mods = list(self.net)
        return (len(mods) == 5 and all(isinstance(m, nn.Tanh) for m in mods[1::2])
                and all(isinstance(m, nn.Linear) and m.bias is not None for m in mods[0::2])
                and tuple(tuple(p.shape) for p in self.net.parameters()) == _SHAPES)

    def packed_params(self):
        """the six tensors as the kernels' flat buffer, differentiable"""
        return torch.cat([p.reshape(-1) for p in self.net.parameters()])

    def forward(self, x):
        if x.dim() != 3:
            raise ValueError(f"transform_to_sphere takes (B, N, {POINT_DIM}) points, got x of shape {tuple(x.shape)}")
        if not self._is_reference_net():
            return _angle_map(self.net(x))
        params = self.packed_params()
        if self.fused and x.is_cuda and x.dtype == torch.float32 and params.dtype == torch.float32:
            return sphere_map(x, params)
        return sphere_map_composed(x, params)


class transform_to_sphere_fast(transform_to_sphere):
    """max_spherical_sliced_w_fast.py:323-338: the same network under the batched file's name"""


__all__ = ["sphere_map", "sphere_map_composed", "transform_to_sphere", "transform_to_sphere_fast"]
