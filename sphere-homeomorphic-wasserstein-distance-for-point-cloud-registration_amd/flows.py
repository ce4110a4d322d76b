"""The sphere map phi of the trainers: `Norm_Flow_structure` (s2_wasserstein.py:134-163), with the Residual flow's
per-point network on the HIP path (csrc/shw_flow.hip, include/shw.h shw_flow_residual_*).

    residual_flow(x, packed_params, hidden, layers, flows)            the fused op: forward and backward kernels
    residual_flow_composed(x, packed_params, hidden, layers, flows)   the same math in torch operations (any device / dtype)
    Norm_Flow_structure(input_dim, flow_name, n_flow_layer)           the trainers' module, reference state-dict layout
    Norm_Flow_structure_optuna(..., Residual_hidden_units, Residual_hidden_layers)

What the trainers use of a Residual flow is z <- z + MLP(z) per point: the reference's flow also estimates a
log-determinant (a geometric draw, a `randn_like`, n + 2 vector-Jacobian products), and `Norm_Flow_structure.forward`
discards it, in train and in eval mode alike, so it is not computed here and the module consumes no random numbers.  The
MLP is `layers` pairs [Swish, Linear], the activation BEFORE every linear layer (on the raw coordinates too):
a(x) = x sigmoid(x softplus(beta)) / 1.1; the linear layer uses W / max(1, sigma / 0.95) with sigma = u^T W v and u, v
buffers that only `update_lipschitz` moves (the trainers never call it).

PACKED EFFECTIVE PARAMETERS, the kernels' input: per flow, per layer, softplus(beta), then the effective weight row-major
(out, in), then the bias.  `packed_params()` builds the buffer from the raw parameters with ordinary differentiable torch
operations, a handful per group of equally shaped layers, so the gradient the backward kernel returns for the buffer
reaches beta, weight (through the division and through sigma) and bias by autograd.

The Planar flow is reproduced as the reference computes it, which depends on the input's rank: its `w` has shape (1, 3)
and the sum runs over axis 1.  For (N, 3) that is the coordinate axis, the usual z + u_hat tanh(w . z + b).  For (B, N, 3)
axis 1 is the POINT axis: lin = w * sum_n z_n + b has shape (B, 1, 3) and every cloud is translated by u_hat * tanh(lin).
21 parameters and a few operations per layer: composed torch, no kernel.
"""
from __future__ import annotations

import math

import torch
import torch.nn.functional as F
from torch import nn

from . import _lib
from .ssw import _stream_ptr

POINT_DIM = 3
MAX_HIDDEN, MIN_LAYERS, MAX_LAYERS, MAX_FLOWS = 32, 2, 8, 16        # include/shw.h shw_flow_residual_supported
LIPSCHITZ_COEFF = 0.95
SWISH_DIVISOR = 1.1
_ENVELOPE = (f"the fused residual flow takes points of dimension {POINT_DIM}, 1 <= hidden <= {MAX_HIDDEN}, "
             f"{MIN_LAYERS} <= layers <= {MAX_LAYERS}, 1 <= flows <= {MAX_FLOWS}")


def residual_flow_supported(dim, hidden, layers, flows):
    return (dim == POINT_DIM and 1 <= hidden <= MAX_HIDDEN and MIN_LAYERS <= layers <= MAX_LAYERS
            and 1 <= flows <= MAX_FLOWS)


def _layer_shapes(dim, hidden, layers):
    """(out, in) of the `layers` linear layers of one flow"""
    channels = [dim] + [hidden] * (layers - 1) + [dim]
    return [(channels[k + 1], channels[k]) for k in range(layers)]


def residual_param_count(hidden, layers, dim=POINT_DIM):
    """floats of the packed parameters of one flow"""
    return sum(1 + o * i + o for o, i in _layer_shapes(dim, hidden, layers))


def residual_flow_composed(x, packed_params, hidden, layers, flows):
    """(..., D) points, packed effective parameters -> (..., D): `flows` blocks z <- z + MLP(z) in torch operations, on any
    device and dtype (x and the parameters of one dtype).  The fallback of the module and the reference of the tests."""
    dim = x.shape[-1]
    shapes = _layer_shapes(dim, hidden, layers)
    if packed_params.dim() != 1 or packed_params.numel() != flows * residual_param_count(hidden, layers, dim):
        raise ValueError(f"packed_params must hold {flows} x {residual_param_count(hidden, layers, dim)} values, got "
                         f"{tuple(packed_params.shape)}")
    z, off = x, 0
    for _ in range(flows):
        h = z
        for out, inp in shapes:
            gamma = packed_params[off]
            weight = packed_params[off + 1:off + 1 + out * inp].view(out, inp)
            bias = packed_params[off + 1 + out * inp:off + 1 + out * inp + out]
            h = F.linear(h * torch.sigmoid(h * gamma) / SWISH_DIVISOR, weight, bias)
            off += 1 + out * inp + out
        z = z + h
    return z


class _ResidualFlow(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, packed, hidden, layers, flows):
        lib = _lib.load()
        dev = x.device
        y = torch.empty_like(x)
        with torch.cuda.device(dev):
            _lib.check(lib.shw_flow_residual_forward(x.data_ptr(), packed.data_ptr(), x.numel() // POINT_DIM, hidden,
                                                     layers, flows, y.data_ptr(), _stream_ptr(dev)),
                       "shw_flow_residual_forward")
        ctx.save_for_backward(x, packed)
        ctx.shape = (hidden, layers, flows)
        return y

    @staticmethod
    def backward(ctx, gy):
        lib = _lib.load()
        x, packed = ctx.saved_tensors
        hidden, layers, flows = ctx.shape
        dev = x.device
        points = x.numel() // POINT_DIM
        gy = gy.to(torch.float32).contiguous()
        gx = torch.empty_like(x) if ctx.needs_input_grad[0] else None
        gp = work = None
        if ctx.needs_input_grad[1]:
            gp = torch.empty_like(packed)
            nbytes = lib.shw_flow_residual_workspace_bytes(points, hidden, layers, flows)
            work = torch.empty(max(nbytes // 4, 1), dtype=torch.float32, device=dev)
        with torch.cuda.device(dev):
            _lib.check(lib.shw_flow_residual_backward(x.data_ptr(), packed.data_ptr(), gy.data_ptr(), points, hidden,
                                                      layers, flows, None if gx is None else gx.data_ptr(),
                                                      None if gp is None else gp.data_ptr(),
                                                      None if work is None else work.data_ptr(), _stream_ptr(dev)),
                       "shw_flow_residual_backward")
        return gx, gp, None, None, None


def residual_flow(x, packed_params, hidden, layers, flows):
    """(N, 3) or (B, N, 3) float32 device points, packed effective parameters (flows * residual_param_count(hidden, layers),)
    -> the points mapped by `flows` residual blocks, same shape.  One kernel forward, one (plus a small reduction)
    backward; differentiable w.r.t. the points and w.r.t. the packed parameters, and only the gradients that are needed
    are computed.  The parameter gradient is summed without atomics: the same bits on every run.  Nothing is saved but x
    and the parameters; all allocation is torch's and nothing synchronises, so the op can be captured in a graph.
    Outside the envelope (dimension 3, 1 <= hidden <= 32, 2 <= layers <= 8, 1 <= flows <= 16): ValueError."""
    for name, t in (("x", x), ("packed_params", packed_params)):
        if not isinstance(t, torch.Tensor):
            raise TypeError(f"{name} must be a torch.Tensor")
        if not t.is_cuda:
            raise RuntimeError(f"{name} is on {t.device}: the MI355X HIP path needs device tensors "
                               "(residual_flow_composed runs anywhere)")
        if t.dtype != torch.float32:
            raise TypeError(f"{name} must be float32, got {t.dtype}")
    hidden, layers, flows = int(hidden), int(layers), int(flows)
    if x.dim() not in (2, 3) or not residual_flow_supported(x.shape[-1], hidden, layers, flows):
        raise ValueError(f"{_ENVELOPE}; got x of shape {tuple(x.shape)}, hidden={hidden}, layers={layers}, flows={flows}")
    count = flows * residual_param_count(hidden, layers)
    if packed_params.dim() != 1 or packed_params.numel() != count:
        raise ValueError(f"packed_params must have shape ({count},), got {tuple(packed_params.shape)}")
    if packed_params.device != x.device:
        raise ValueError("x and packed_params must be on one device")
    return _ResidualFlow.apply(x.contiguous(), packed_params.contiguous(), hidden, layers, flows)


# ------------------------------------------------------------------------------------------------ the modules
class Swish(nn.Module):
    """x sigmoid(x softplus(beta)) / 1.1, beta a (1,) parameter starting at 0.5 (nets/lipschitz.py:642-648)"""

    def __init__(self):
        super().__init__()
        self.beta = nn.Parameter(torch.tensor([0.5]))

    def forward(self, x):
        return x * torch.sigmoid(x * F.softplus(self.beta)) / SWISH_DIVISOR


class InducedNormLinear(nn.Module):
    """Linear layer whose weight is divided by max(1, sigma / coeff), sigma = u^T W v the power-iteration estimate of
    its spectral norm (nets/lipschitz.py:132-274, the 2-norm case the trainers use).  u, v, scale are buffers."""

    def __init__(self, in_features, out_features, coeff=LIPSCHITZ_COEFF, zero_init=False, n_iterations=5):
        super().__init__()
        self.in_features, self.out_features, self.coeff, self.n_iterations = in_features, out_features, coeff, n_iterations
        self.weight = nn.Parameter(torch.empty(out_features, in_features))
        self.bias = nn.Parameter(torch.empty(out_features))
        nn.init.kaiming_uniform_(self.weight, a=math.sqrt(5))
        if zero_init:
            self.weight.data.div_(1000)
        bound = 1 / math.sqrt(in_features)
        nn.init.uniform_(self.bias, -bound, bound)
        self.register_buffer("scale", torch.tensor(0.0))
        self.register_buffer("u", F.normalize(torch.empty(out_features).normal_(0, 1), dim=0))
        self.register_buffer("v", F.normalize(torch.empty(in_features).normal_(0, 1), dim=0))
        self.power_iteration(200)

    @torch.no_grad()
    def power_iteration(self, n_iterations=None):
        """u <- W v / |W v|, v <- W^T u / |W^T u|, `n_iterations` times; then scale <- u^T W v"""
        weight = self.weight.detach()
        u, v = self.u, self.v
        for _ in range(self.n_iterations if n_iterations is None else n_iterations):
            u = F.normalize(torch.mv(weight, v), dim=0)
            v = F.normalize(torch.mv(weight.t(), u), dim=0)
        self.u.copy_(u)
        self.v.copy_(v)
        self.scale.copy_(torch.dot(self.u, torch.mv(weight, self.v)))

    def compute_weight(self):
        sigma = torch.dot(self.u, torch.mv(self.weight, self.v))
        with torch.no_grad():
            self.scale.copy_(sigma)
        return self.weight / torch.clamp(sigma / self.coeff, min=1.0)

    def forward(self, x):
        return F.linear(x, self.compute_weight(), self.bias)


class LipschitzMLP(nn.Module):
    """[Swish, InducedNormLinear] per pair of consecutive channels; the last layer starts at 1/1000 scale"""

    def __init__(self, channels, lipschitz_const=LIPSCHITZ_COEFF, max_lipschitz_iter=5, init_zeros=True):
        super().__init__()
        n = len(channels) - 1
        layers = []
        for k in range(n):
            layers += [Swish(), InducedNormLinear(channels[k], channels[k + 1], lipschitz_const,
                                                  zero_init=init_zeros and k == n - 1, n_iterations=max_lipschitz_iter)]
        self.net = nn.Sequential(*layers)

    def forward(self, x):
        return self.net(x)


class iResBlock(nn.Module):
    """Holder of the network, with the parameters and buffers of the reference's log-determinant estimator so that its
    snapshots load: geom_p and lamb are parameters that take part in nothing and never receive a gradient."""

    def __init__(self, nnet, geom_p=0.5, lamb=2.0):
        super().__init__()
        self.nnet = nnet
        self.geom_p = nn.Parameter(torch.tensor(math.log(geom_p) - math.log(1.0 - geom_p), dtype=torch.float64))
        self.lamb = nn.Parameter(torch.tensor(lamb))
        self.register_buffer("last_n_samples", torch.zeros(1))
        self.register_buffer("last_firmom", torch.zeros(1))
        self.register_buffer("last_secmom", torch.zeros(1))

    def forward(self, x):
        return x + self.nnet(x)


class Residual(nn.Module):
    """One residual flow, layer by layer in torch; returns the points only"""

    def __init__(self, net):
        super().__init__()
        self.iresblock = iResBlock(net)

    def forward(self, z):
        return self.iresblock(z)


class Planar(nn.Module):
    """z + u_hat tanh(lin) with the reference's axis-1 sum (flows/planar.py:51-64; module docstring); points only"""

    def __init__(self, shape):
        super().__init__()
        size = 1
        for s in shape:
            size *= s
        self.u = nn.Parameter(torch.empty(shape)[None])
        nn.init.uniform_(self.u, -math.sqrt(2), math.sqrt(2))
        self.w = nn.Parameter(torch.empty(shape)[None])
        nn.init.uniform_(self.w, -math.sqrt(2.0 / size), math.sqrt(2.0 / size))
        self.b = nn.Parameter(torch.zeros(1))

    def forward(self, z):
        lin = torch.sum(self.w * z, list(range(1, self.w.dim())), keepdim=True) + self.b
        inner = torch.sum(self.w * self.u)
        u_hat = self.u + (torch.log(1 + torch.exp(inner)) - 1 - inner) * self.w / torch.sum(self.w ** 2)
        return z + u_hat * torch.tanh(lin)


class Norm_Flow_structure(nn.Module):
    """`Norm_Flow_structure(input_dim=3, flow_name="Planar", n_flow_layer=3)` of s2_wasserstein.py:134-163: forward(x)
    returns the mapped points.  Parameters, buffers, their names, shapes and order are the reference's, so
    `load_state_dict` takes its snapshots (train_W_COS.py:260-261) and an optimizer built from `parameters()` sees the same
    sequence.  "Residual": 7 linear layers of width 8 per flow; a float32 device input of dimension 3 inside the kernel's
    envelope takes the fused path (`residual_flow`), everything else -- CPU, float64, other dimensions, hidden > 32, or
    `self.fused = False` -- the composed one (`residual_flow_composed`), both from `packed_params()`.  "Planar": composed
    torch in both input ranks (module docstring).  train() and eval() compute the same values, as in the reference; no
    random numbers are drawn, where the reference draws a geometric sample and a `randn_like` per flow and call."""

    hidden_units, hidden_layers = 8, 7

    def __init__(self, input_dim=3, flow_name="Planar", n_flow_layer=3):
        super().__init__()
        self.input_dim, self.flow_name, self.fused = input_dim, flow_name, True
        self.net = nn.ModuleList(self.create__NF_structure(flow_name, input_dim, n_flow_layer))

    def create__NF_structure(self, flow_name, input_dim, n_flow_layer):
        if flow_name == "Planar":
            return [Planar((input_dim,)) for _ in range(n_flow_layer)]
        if flow_name == "Residual":
            channels = [input_dim] + [self.hidden_units] * (self.hidden_layers - 1) + [input_dim]
            return [Residual(LipschitzMLP(channels, init_zeros=True, lipschitz_const=LIPSCHITZ_COEFF))
                    for _ in range(n_flow_layer)]
        raise ValueError("Flow name is not valid")

    def _pairs(self, flow):
        mods = list(flow.iresblock.nnet.net)
        return list(zip(mods[0::2], mods[1::2]))

    def packed_params(self):
        """the packed effective parameters of every flow, differentiable w.r.t. beta, weight and bias (Residual only).
        Equally shaped layers are stacked, so the cost is a few operations per group, not per layer."""
        if self.flow_name != "Residual":
            raise ValueError("packed_params() is defined for the Residual flow")
        layers, flows = self.hidden_layers, len(self.net)
        roles = [[0]] if layers == 1 else [[0], list(range(1, layers - 1)), [layers - 1]]
        per_flow = [self._pairs(flow) for flow in self.net]
        blocks = []
        for ks in roles:
            if not ks:
                continue
            pairs = [per_flow[f][k] for f in range(flows) for k in ks]
            weight = torch.stack([lin.weight for _, lin in pairs])
            u = torch.stack([lin.u for _, lin in pairs])
            v = torch.stack([lin.v for _, lin in pairs])
            sigma = (u[:, :, None] * weight * v[:, None, :]).sum((1, 2))
            w_eff = weight / torch.clamp(sigma / pairs[0][1].coeff, min=1.0)[:, None, None]
            gamma = F.softplus(torch.cat([act.beta for act, _ in pairs]))
            bias = torch.stack([lin.bias for _, lin in pairs])
            blocks.append(torch.cat([gamma[:, None], w_eff.flatten(1), bias], 1).reshape(flows, -1))
        return torch.cat(blocks, 1).reshape(-1)

    def forward_layers(self, x):
        """the layer-by-layer module path (also refreshes every `scale` buffer)"""
        for flow in self.net:
            x = flow(x)
        return x

    def forward(self, x):
        if self.flow_name != "Residual":
            return self.forward_layers(x)
        hidden, layers, flows = self.hidden_units, self.hidden_layers, len(self.net)
        if flows == 0:
            return x
        packed = self.packed_params()
        if (self.fused and x.is_cuda and x.dtype == torch.float32 and packed.dtype == torch.float32 and x.dim() in (2, 3)
                and residual_flow_supported(x.shape[-1], hidden, layers, flows) and self.input_dim == POINT_DIM):
            return residual_flow(x, packed, hidden, layers, flows)
        return residual_flow_composed(x, packed, hidden, layers, flows)

    @torch.no_grad()
    def update_lipschitz(self, n_iterations=5):
        """power iteration on every linear layer's u, v (what the reference's compute_weight(update=True) does)"""
        for m in self.modules():
            if isinstance(m, InducedNormLinear):
                m.power_iteration(n_iterations)


class Norm_Flow_structure_optuna(Norm_Flow_structure):
    """s2_wasserstein.py:171-201: the same with the Residual network's width and its number of linear layers given"""

    def __init__(self, input_dim=3, flow_name="Planar", n_flow_layer=3, Residual_hidden_units=8, Residual_hidden_layers=3):
        self.Residual_hidden_units, self.Residual_hidden_layers = Residual_hidden_units, Residual_hidden_layers
        self.hidden_units, self.hidden_layers = Residual_hidden_units, Residual_hidden_layers
        super().__init__(input_dim, flow_name, n_flow_layer)


__all__ = ["residual_flow", "residual_flow_composed", "residual_flow_supported", "residual_param_count",
           "Norm_Flow_structure", "Norm_Flow_structure_optuna"]
