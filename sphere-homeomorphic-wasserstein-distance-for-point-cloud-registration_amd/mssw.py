"""The minibatch Residual-MSSW loss of mini_batch_Residual_MSSW.py: its sphere encoder `transform_to_sphere(flow_name,
n_flow_layer)` (:392-406) with the per-point work on the HIP path (csrc/shw_mssw.hip, include/shw.h shw_mssw_*), and its
wrapper `max_spherical_wassersten_distance_Residual` (:413-451).

    residual_sphere_map(x, params, affine, flows)            the fused op: one forward kernel, one recomputing backward
    residual_sphere_map_composed(x, params, affine, flows)   the same math in torch operations (any device / dtype)
    MLP_Architecture, Flow_structure, ActNorm, transform_to_sphere     the reference's modules, its state-dict layout
    max_spherical_wassersten_distance_Residual               the wrapper: a random minibatch of pairs per ascent step

Per point (b, n) of a (B, N, 3) cloud: h1 = relu(W1 x + b1) (8), h2 = relu(W2 h1 + b2) (8), z = W3 h2 + b3 (2); per flow
an i-ResNet block on MLP = `flows.LipschitzMLP([2, 4, 2], 0.9)`, then z <- z exp(s[n]) + t[n]; then the angle map of
sphere_map.py.  The scale and shift belong to the POINT INDEX: the reference's `ActNorm(2)` holds s, t of shape (1, 2),
takes mean and unbiased std over the batch axis only on its first forward, and thereby turns both into (1, N, 2).  A
module initialised at N points refuses any other N; it takes any B.  B = 1 at initialisation gives NaN, as there.

THE DIRECTION OF THE BLOCKS.  The reference builds `nf.flows.Residual(net, reduce_memory=True)` (:380) with the class's
default `reverse=True`: its forward applies the INVERSE of z -> z + MLP(z), by a fixed-point loop whose loose stopping
rule looks at the whole batch (class Residual below).  That is the default here, `reverse=True`, in composed torch, and
what fixture G21 pins.  `reverse=False` applies the block itself, z <- z + MLP(z), per point: the direction the kernels
fuse, opt-in because it is another map than the reference's.  The fused op and its composed twin are forward blocks.

PARAMETERS, the kernels' input: `params`, flat: the encoder in state-dict order (W1 (8, 3), b1, W2 (8, 8), b2, W3 (2, 8),
b3: 122 values), then per flow the packed effective parameters in flows.py's convention (softplus(beta0), W_eff,0 (4, 2),
c0, softplus(beta1), W_eff,1 (2, 4), c1: 24 values); `affine` (F, N, 4): (s0, s1, t0, t1) per flow and point index.  Both
are built from the raw parameters with differentiable torch operations, so autograd carries the kernels' gradients back.

As in flows.py, the log-determinant the reference's Residual estimates and `Flow_structure.forward` throws away is not
computed: train() and eval() give the same values and NO RANDOM NUMBERS ARE DRAWN, where the reference in train mode
draws a geometric sample and a `randn_like` per flow and call from the global generators -- a caller who draws the SSW
directions from the global torch generator sees another stream than with the reference.  "Planar" sums over the point axis
of a (B, N, 2) input (flows.py docstring): every layer is a per-cloud translation, a few operations, and stays composed
torch for the reason flows.py gives.
"""
from __future__ import annotations

import math

import numpy as np
import torch
import torch.nn.functional as F
from torch import nn

from . import _lib
from . import flows as _flows
from .flows import SWISH_DIVISOR, LipschitzMLP, Planar
from .modules import _sum_over_pairs
from .sphere_map import _angle_map
from .ssw import _stream_ptr, sliced_wasserstein_sphere

POINT_DIM, ENC_HIDDEN, LATENT, FLOW_HIDDEN, FLOW_LAYERS, MAX_FLOWS = 3, 8, 2, 4, 2, 8   # include/shw.h shw_mssw_supported
LIPSCHITZ_COEFF = 0.9
_ENC_SHAPES = ((ENC_HIDDEN, POINT_DIM), (ENC_HIDDEN,), (ENC_HIDDEN, ENC_HIDDEN), (ENC_HIDDEN,), (LATENT, ENC_HIDDEN),
               (LATENT,))
ENC_PARAM_COUNT = sum(math.prod(s) for s in _ENC_SHAPES)                                # 122
FLOW_PARAM_COUNT = 2 + 2 * LATENT * FLOW_HIDDEN + FLOW_HIDDEN + LATENT                  # 24


def residual_sphere_map_param_count(flows):
    return ENC_PARAM_COUNT + FLOW_PARAM_COUNT * int(flows)


def _check_shapes(x, params, affine, flows):
    if x.dim() != 3 or x.shape[-1] != POINT_DIM:
        raise ValueError(f"the residual sphere map takes (B, N, {POINT_DIM}) points; got x of shape {tuple(x.shape)}")
    count = residual_sphere_map_param_count(flows)
    if params.dim() != 1 or params.numel() != count:
        raise ValueError(f"params must have shape ({count},), got {tuple(params.shape)}")
    if tuple(affine.shape) != (flows, x.shape[1], 4):
        raise ValueError(f"affine must have shape ({flows}, {x.shape[1]}, 4), got {tuple(affine.shape)}")


def residual_sphere_map_composed(x, params, affine, flows):
    """(B, N, 3) points, the flat parameter buffer (122 + 24 flows,), affine (flows, N, 4) -> (B, N, 3) unit vectors, in
    torch operations on any device and dtype (all three of one dtype), any flows >= 0.  The encoder runs as the reference
    runs it, Conv1d on the permuted input.  The fallback of the module and the reference of the tests."""
    flows = int(flows)
    _check_shapes(x, params, affine, flows)
    enc = params[:ENC_PARAM_COUNT].split([math.prod(s) for s in _ENC_SHAPES])
    w1, b1, w2, b2, w3, b3 = (t.view(s) for t, s in zip(enc, _ENC_SHAPES))
    h = x.permute(0, 2, 1)
    h = F.relu(F.conv1d(h, w1[:, :, None], b1))
    h = F.relu(F.conv1d(h, w2[:, :, None], b2))
    z = F.conv1d(h, w3[:, :, None], b3).permute(0, 2, 1).contiguous()
    off = ENC_PARAM_COUNT
    for f in range(flows):
        h = z
        for out, inp in ((FLOW_HIDDEN, LATENT), (LATENT, FLOW_HIDDEN)):
            gamma = params[off]
            weight = params[off + 1:off + 1 + out * inp].view(out, inp)
            bias = params[off + 1 + out * inp:off + 1 + out * inp + out]
            h = F.linear(h * torch.sigmoid(h * gamma) / SWISH_DIVISOR, weight, bias)
            off += 1 + out * inp + out
        z = (z + h) * torch.exp(affine[f, :, :LATENT]) + affine[f, :, LATENT:]
    return _angle_map(z)


class _ResidualSphereMap(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, params, affine, flows):
        lib = _lib.load()
        dev = x.device
        y = torch.empty_like(x)
        with torch.cuda.device(dev):
            _lib.check(lib.shw_mssw_forward(x.data_ptr(), params.data_ptr(), affine.data_ptr(), x.shape[0], x.shape[1],
                                            flows, y.data_ptr(), _stream_ptr(dev)), "shw_mssw_forward")
        ctx.save_for_backward(x, params, affine)
        ctx.flows = flows
        return y

    @staticmethod
    def backward(ctx, gy):
        lib = _lib.load()
        x, params, affine = ctx.saved_tensors
        dev = x.device
        gy = gy.to(torch.float32).contiguous()
        gx = torch.empty_like(x) if ctx.needs_input_grad[0] else None
        gp = torch.empty_like(params) if ctx.needs_input_grad[1] else None
        ga = torch.empty_like(affine) if ctx.needs_input_grad[2] else None
        work = None
        if gp is not None or ga is not None:
            nbytes = lib.shw_mssw_workspace_bytes(x.shape[0], x.shape[1], ctx.flows)
            work = torch.empty(max(nbytes // 4, 1), dtype=torch.float32, device=dev)
        ptr = lambda t: None if t is None else t.data_ptr()                                  # noqa: E731
        with torch.cuda.device(dev):
            _lib.check(lib.shw_mssw_backward(x.data_ptr(), params.data_ptr(), affine.data_ptr(), gy.data_ptr(), x.shape[0],
                                             x.shape[1], ctx.flows, ptr(gx), ptr(gp), ptr(ga), ptr(work),
                                             _stream_ptr(dev)), "shw_mssw_backward")
        return gx, gp, ga, None


def residual_sphere_map(x, params, affine, flows):
    """(B, N, 3) float32 device points, the flat parameter buffer (122 + 24 flows,), affine (flows, N, 4) -> the points on
    the unit sphere, same shape.  One kernel forward, one (plus small reductions) backward; differentiable w.r.t. the
    points, the parameters and the scales and shifts, and only the gradients that are needed are computed.  The gradient
    of `affine` sums over the batch axis, that of `params` over all points, both without atomics: the same bits on every
    run.  Nothing is saved but the inputs; all allocation is torch's and nothing synchronises, so the op can be captured
    in a graph.  Outside 1 <= flows <= 8: ValueError (residual_sphere_map_composed takes any)."""
    for name, t in (("x", x), ("params", params), ("affine", affine)):
        if not isinstance(t, torch.Tensor):
            raise TypeError(f"{name} must be a torch.Tensor")
        if not t.is_cuda:
            raise RuntimeError(f"{name} is on {t.device}: the MI355X HIP path needs device tensors "
                               "(residual_sphere_map_composed runs anywhere)")
        if t.dtype != torch.float32:
            raise TypeError(f"{name} must be float32, got {t.dtype}")
    flows = int(flows)
    if not 1 <= flows <= MAX_FLOWS:
        raise ValueError(f"the fused residual sphere map takes 1 <= flows <= {MAX_FLOWS}, got flows={flows}")
    _check_shapes(x, params, affine, flows)
    if params.device != x.device or affine.device != x.device:
        raise ValueError("x, params and affine must be on one device")
    return _ResidualSphereMap.apply(x.contiguous(), params.contiguous(), affine.contiguous(), flows)


# ------------------------------------------------------------------------------------------------ the modules
class MLP_Architecture(nn.Module):
    """`MLP_Architecture(emb_dims=2)` of :327-355: Conv1d(3, 8, 1), ReLU, Conv1d(8, 8, 1), ReLU, Conv1d(8, emb_dims, 1)
    on the permuted input.  The three convolutions are members AND entries of `net`, as there, so the state dict holds
    every tensor twice (`conv1.weight` and `net.0.weight`) and `parameters()` yields it once."""

    def __init__(self, emb_dims=2):
        super().__init__()
        self.emb_dims = emb_dims
        self.conv1 = nn.Conv1d(POINT_DIM, ENC_HIDDEN, 1)
        self.conv2 = nn.Conv1d(ENC_HIDDEN, ENC_HIDDEN, 1)
        self.conv3 = nn.Conv1d(ENC_HIDDEN, emb_dims, 1)
        self.relu = nn.ReLU()
        self.net = nn.Sequential(self.conv1, self.relu, self.conv2, self.relu, self.conv3)

    def forward(self, input_data):
        return self.net(input_data.permute(0, 2, 1)).permute(0, 2, 1)


class ActNorm(nn.Module):
    """`ActNorm(shape)` of the reference's flows/normalization.py: z exp(s) + t with s, t parameters of shape
    (1, *shape), initialised from the first input: s = -log(std(z) + 1e-6), t = -mean(z) exp(s), mean and unbiased std
    over the axes on which s has size 1 AT CONSTRUCTION, keepdim -- so for shape (2,) and a (B, N, 2) input both become
    (1, N, 2).  `data_dep_init_done` is the reference's buffer (replaced by a CPU tensor(1.0) there too); `initialised` is
    the Python flag beside it that the forward tests, so that no call after the first reads the device.  Loading a snapshot
    taken after initialisation re-shapes s, t and leaves the module initialised."""

    def __init__(self, shape):
        super().__init__()
        if isinstance(shape, int):
            shape = (shape,)
        self.s = nn.Parameter(torch.zeros(shape)[None])
        self.t = nn.Parameter(torch.zeros(shape)[None])
        self.batch_dims = [i for i, n in enumerate(self.s.shape) if n == 1]
        self.register_buffer("data_dep_init_done", torch.tensor(0.0))
        self.initialised = False

    def _load_from_state_dict(self, state_dict, prefix, *args, **kwargs):
        for name in ("s", "t"):
            value = state_dict.get(prefix + name)
            param = getattr(self, name)
            if value is not None and value.shape != param.shape:
                param.data = param.data.new_zeros(value.shape)
        done = state_dict.get(prefix + "data_dep_init_done")
        if done is not None:
            self.initialised = bool(float(done) > 0.0)
        super()._load_from_state_dict(state_dict, prefix, *args, **kwargs)

    def forward(self, z):
        if not self.initialised:
            with torch.no_grad():
                s_init = -torch.log(z.std(dim=self.batch_dims, keepdim=True) + 1e-6)
                self.s.data = s_init
                self.t.data = -z.mean(dim=self.batch_dims, keepdim=True) * torch.exp(s_init)
            self.data_dep_init_done = torch.tensor(1.0)
            self.initialised = True
        return z * torch.exp(self.s) + self.t


class Residual(_flows.Residual):
    """`nf.flows.Residual(net, reduce_memory=True)` as mini_batch_Residual_MSSW.py:380 builds it, that is with the class's
    default `reverse=True`: forward(y) is the INVERSE of x -> x + net(x), by the reference's fixed-point iteration
    (flows/residual.py:133-142) -- x <- y - net(x) from x = y, until every entry of the whole batch moved by less than
    sqrt(1e-5 + 1e-5 |y|), at most 1001 further steps -- with autograd through the unrolled steps, as there.  The stopping
    rule is global: the number of steps, and with it every point's value to within that loose tolerance, depends on the
    whole input, and each step reads one flag back from the device, as in the reference.  `reverse=False` is the block
    itself, y + net(y), what the trainers' Norm_Flow_structure applies: per point, one evaluation, no read-back."""

    def __init__(self, net, reverse=True):
        super().__init__(net)
        self.reverse = reverse

    def forward(self, z):
        if not self.reverse:
            return self.iresblock(z)
        nnet = self.iresblock.nnet
        x, x_prev = z - nnet(z), z
        tol = 1e-5 + z.abs() * 1e-5
        steps = 0
        while not torch.all((x - x_prev) ** 2 / tol < 1):
            x, x_prev = z - nnet(x), x
            steps += 1
            if steps > 1000:
                break
        return x


class Flow_structure(nn.Module):
    """`Flow_structure(input_dim=2, flow_name="Planar", n_flow_layer=3)` of :359-390: "Planar", n_flow_layer planar flows;
    "Residual", n_flow_layer pairs of an i-ResNet block on LipschitzMLP([d, 4, d], lipschitz_const=0.9), applied in the
    direction `reverse` (class Residual; True is the reference's), and an ActNorm(d).  forward(x) returns the mapped points
    (the reference drops every log-determinant)."""

    hidden_units, hidden_layers = FLOW_HIDDEN, FLOW_LAYERS

    def __init__(self, input_dim=2, flow_name="Planar", n_flow_layer=3, reverse=True):
        super().__init__()
        self.input_dim, self.flow_name, self.reverse = input_dim, flow_name, reverse
        self.net = nn.ModuleList(self.create__NF_structure(flow_name, input_dim, n_flow_layer))

    def create__NF_structure(self, flow_name, input_dim, n_flow_layer):
        if flow_name == "Planar":
            return [Planar((input_dim,)) for _ in range(n_flow_layer)]
        if flow_name == "Residual":
            channels = [input_dim] + [self.hidden_units] * (self.hidden_layers - 1) + [input_dim]
            flows = []
            for _ in range(n_flow_layer):
                flows += [Residual(LipschitzMLP(channels, init_zeros=True, lipschitz_const=LIPSCHITZ_COEFF), self.reverse),
                          ActNorm(input_dim)]
            return flows
        raise ValueError("Flow name is not valid")

    def forward(self, x):
        for flow in self.net:
            x = flow(x)
        return x


class transform_to_sphere(nn.Module):
    """`transform_to_sphere(flow_name, n_flow_layer=3, two_d_encoder=MLP_Architecture, flow=Flow_structure)` of :392-406:
    forward(x) maps (B, N, 3) points onto the unit sphere.  State-dict keys, shapes, the values drawn from a seed and the
    order of `parameters()` are the reference's.

    `reverse=True` (default) is the reference's map, every block applied as its inverse (module docstring): the layers
    themselves, composed torch, one flag read back from the device per fixed-point step, as there.  `reverse=False` applies
    the blocks forward: the call that initialises the ActNorm layers from its input runs the layers; afterwards a float32
    device input with flow_name "Residual", an untouched structure, at most 8 flows and `self.fused` on takes the fused
    path (`residual_sphere_map` on `packed_params()` and `packed_affine()`); CPU, float64, more than 8 flows or
    `fused = False` take `residual_sphere_map_composed`, an edited encoder or flow the layers themselves, and after the
    first call that forward reads nothing back from the device.  "Planar" is composed torch (module docstring).  Another
    N than the initialised one: ValueError.  train() and eval() compute the same values and
    no random numbers are drawn (module docstring).  A state dict saved after initialisation loads into a fresh module
    and leaves it initialised, which the reference's own class cannot do."""

    def __init__(self, flow_name, n_flow_layer=3, two_d_encoder=MLP_Architecture, flow=Flow_structure, reverse=True):
        super().__init__()
        self.flow_name, self.fused = flow_name, True         # (fused matters with reverse=False only)
        self.net = two_d_encoder()
        self.flows = flow(flow_name=flow_name, n_flow_layer=n_flow_layer, **({} if reverse else {"reverse": False}))

    def _pairs(self):
        """[(Residual, ActNorm)] when the structure is the reference's Residual one with forward blocks, else None"""
        enc = self.net
        if not (type(enc) is MLP_Architecture and isinstance(getattr(enc, "net", None), nn.Sequential)
                and len(enc.net) == 5 and enc.net[0] is enc.conv1 and enc.net[2] is enc.conv2 and enc.net[4] is enc.conv3
                and all(type(m) is nn.ReLU for m in (enc.net[1], enc.net[3]))
                and all(type(c) is nn.Conv1d and c.bias is not None for c in (enc.conv1, enc.conv2, enc.conv3))
                and tuple(tuple(p.shape) for p in enc.parameters()) == tuple(s + (1,) if len(s) == 2 else s
                                                                             for s in _ENC_SHAPES)):
            return None
        if self.flow_name != "Residual" or type(self.flows) is not Flow_structure:
            return None
        mods = list(self.flows.net)
        pairs = list(zip(mods[0::2], mods[1::2]))
        if len(mods) % 2 or not pairs:
            return None
        for res, act in pairs:
            if (type(res) is not Residual or res.reverse or type(act) is not ActNorm
                    or type(res.iresblock.nnet) is not LipschitzMLP):
                return None
            layers = list(res.iresblock.nnet.net)
            if (len(layers) != 4 or tuple(layers[1].weight.shape) != (FLOW_HIDDEN, LATENT)
                    or tuple(layers[3].weight.shape) != (LATENT, FLOW_HIDDEN) or act.s.dim() != 3 or act.s.shape[-1] != LATENT
                    or act.s.shape != act.t.shape):
                return None
        return pairs

    def packed_params(self):
        """the kernels' flat parameter buffer, differentiable w.r.t. every raw parameter (Residual only)"""
        pairs = self._pairs()
        if pairs is None:
            raise ValueError("packed_params() is defined for the reference's Residual structure with reverse=False")
        blocks = []
        for k in (0, 1):
            acts = [res.iresblock.nnet.net[2 * k] for res, _ in pairs]
            lins = [res.iresblock.nnet.net[2 * k + 1] for res, _ in pairs]
            weight = torch.stack([lin.weight for lin in lins])
            u, v = torch.stack([lin.u for lin in lins]), torch.stack([lin.v for lin in lins])
            sigma = (u[:, :, None] * weight * v[:, None, :]).sum((1, 2))
            w_eff = weight / torch.clamp(sigma / lins[0].coeff, min=1.0)[:, None, None]
            gamma = F.softplus(torch.cat([act.beta for act in acts]))
            blocks.append(torch.cat([gamma[:, None], w_eff.flatten(1), torch.stack([lin.bias for lin in lins])], 1))
        return torch.cat([p.reshape(-1) for p in self.net.parameters()] + [torch.cat(blocks, 1).reshape(-1)])

    def packed_affine(self):
        """(flows, N, 4): (s0, s1, t0, t1) per flow and point index, differentiable (Residual only, after initialisation)"""
        pairs = self._pairs()
        if pairs is None:
            raise ValueError("packed_affine() is defined for the reference's Residual structure with reverse=False")
        return torch.cat([torch.cat([act.s, act.t], -1) for _, act in pairs], 0)

    def acts_per_cloud(self):
        """True when a cloud's map does not depend on the other clouds of the batch: everything but the reference's
        reversed Residual blocks, whose stopping rule is global"""
        return not any(isinstance(m, Residual) and m.reverse for m in self.flows.modules())

    def is_initialised(self):
        """True when no ActNorm layer is waiting for its first input"""
        return all(m.initialised for m in self.flows.modules() if isinstance(m, ActNorm))

    def forward_layers(self, x):
        """the layer-by-layer module path (also refreshes every `scale` buffer)"""
        return _angle_map(self.flows(self.net(x).contiguous()))

    def forward(self, x):
        if x.dim() != 3 or x.shape[-1] != POINT_DIM:
            raise ValueError(f"transform_to_sphere takes (B, N, {POINT_DIM}) points, got x of shape {tuple(x.shape)}")
        if not self.is_initialised():
            return self.forward_layers(x)
        for m in self.flows.modules():
            if isinstance(m, ActNorm) and m.s.dim() == 3 and m.s.shape[1] != x.shape[1]:
                raise ValueError(f"this transform_to_sphere was initialised on clouds of {m.s.shape[1]} points (its ActNorm "
                                 f"scales belong to the point index); got clouds of {x.shape[1]} points")
        pairs = self._pairs()
        if pairs is None or any(act.s.shape[1] != x.shape[1] for _, act in pairs):
            return self.forward_layers(x)
        params, affine = self.packed_params(), self.packed_affine()
        if (self.fused and x.is_cuda and x.dtype == torch.float32 and params.dtype == torch.float32
                and affine.dtype == torch.float32 and len(pairs) <= MAX_FLOWS):
            return residual_sphere_map(x, params, affine, len(pairs))
        return residual_sphere_map_composed(x, params, affine, len(pairs))


# ------------------------------------------------------------------------------------------------ the wrapper
class max_spherical_wassersten_distance_Residual(nn.Module):
    """phi-max wrapper with a random minibatch of pairs per ascent step (:413-451): `forward(first, second, train_or_test)
    -> (ssw, phi(first), phi(second))`.  Per inner iteration, `np.random.choice(B, psi_minibatch_size, replace=False)`
    from numpy's global generator (one call per iteration, as there), the sum of the per-pair SSW over those pairs in the
    drawn order, and the ascent step; then the sum over all pairs on the non-detached inputs.  "test" skips the loop.
    (The reference's log-determinant estimator draws from numpy's global generator between those calls; this package does
    not, so from one numpy seed the minibatches are other ones than the reference's.)

    When SSW is this package's per-pair function the selected pairs go through one batched launch, their direction sets
    drawn in the reference's order (modules._sum_over_pairs).  When phi is an initialised `mssw.transform_to_sphere` that
    acts per cloud (forward blocks or Planar) and `subset_map` is on, the inner loop maps only the selected clouds: their
    values are those of the full map and the parameter gradients differ by the order of summation only.  With the
    reference's reversed blocks the stopping rule sees the whole batch, so the full batch is mapped, as there; so it is by
    a call that still has to initialise phi."""

    def __init__(self, num_projections, phi, phi_op, SSW=sliced_wasserstein_sphere, p=2, max_iter=10, psi_minibatch_size=5,
                 device="cuda", verbose=False):
        super().__init__()
        self.num_projections, self.phi, self.SSW, self.phi_op = num_projections, phi, SSW, phi_op
        self.p, self.max_iter, self.psi_minibatch_size = p, max_iter, psi_minibatch_size
        self.device, self.verbose, self.subset_map = device, verbose, True
        self.on_inner_value = None       # optional observer of the per-iteration ssw (the reference prints it, :442)

    def _ssw(self, a, b):
        return _sum_over_pairs(self.SSW, a, b, self.num_projections, self.device, self.p)

    def forward(self, first_samples, second_samples, train_or_test="train"):
        first_detach, second_detach = first_samples.detach(), second_samples.detach()
        if train_or_test == "train":
            for _ in range(self.max_iter):
                subset = (self.subset_map and isinstance(self.phi, transform_to_sphere) and self.phi.is_initialised()
                          and self.phi.acts_per_cloud())
                if not subset:
                    first_t, second_t = self.phi(first_detach), self.phi(second_detach)
                mini_batch = np.random.choice(len(first_detach), size=self.psi_minibatch_size, replace=False)
                index = torch.as_tensor(mini_batch, device=first_detach.device)
                if subset:
                    ssw = self._ssw(self.phi(first_detach[index]), self.phi(second_detach[index]))
                else:
                    ssw = self._ssw(first_t[index], second_t[index])
                loss = -ssw                                   # gradient ascent on phi (:438)
                self.phi_op.zero_grad()
                loss.backward(retain_graph=True)
                self.phi_op.step()
                if self.verbose:
                    print(ssw.item())
                if self.on_inner_value is not None:
                    self.on_inner_value(float(ssw.detach().sum()))
        elif train_or_test != "test":
            raise ValueError("train_or_test must be 'train' or 'test'")
        first_t, second_t = self.phi(first_samples), self.phi(second_samples)
        return self._ssw(first_t, second_t), first_t, second_t


__all__ = ["residual_sphere_map", "residual_sphere_map_composed", "residual_sphere_map_param_count", "MLP_Architecture",
           "Flow_structure", "ActNorm", "transform_to_sphere", "max_spherical_wassersten_distance_Residual"]
