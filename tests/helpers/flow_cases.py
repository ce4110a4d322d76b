"""Shared cases of the sphere-map tests (tests/test_flows_cpu.py, tests/test_flows_gpu.py): fixture G18 read back into
tensors, random packed parameters, and the float64 / float32 references of the composed path, each computed once.

Error rule (the one of tests/test_line_weight_grad_gpu.py): a float32 result is compared with the composed path in float64
on the same float32 parameters and inputs, per tensor, on max |error| / max |reference entry|; the bound is 4 x the
deviation of the float32 composed path from the float64 one on the same data, with a floor of 1e-6."""
import functools
import os
from collections import OrderedDict

import numpy as np
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "golden", "g18_flows.npz")
FLOOR = 1e-6
COEFF = 0.95
# (hidden, layers, flows): the trainers' shape with 3 and with 8 flows, one flow, a width that fills no register group,
# two layers (no hidden-to-hidden layer), a width above 8, and the corners of the envelope
SHAPES = [(8, 7, 3), (8, 7, 8), (8, 3, 1), (5, 2, 2), (12, 4, 3), (32, 8, 2), (1, 2, 16)]
# point counts 1, 63, 64, 65, 257, 1023, 4099 (lane, wave and block edges, several blocks with a ragged last one), in both
# input ranks
INPUT_SHAPES = [(1, 3), (1, 63, 3), (64, 3), (5, 13, 3), (257, 3), (3, 341, 3), (4099, 3)]


def max_dev(got, ref):
    got, ref = torch.as_tensor(got).double().cpu(), torch.as_tensor(ref).double().cpu()
    assert got.shape == ref.shape, (got.shape, ref.shape)
    if ref.numel() == 0:
        return 0.0
    scale = float(ref.abs().max())
    return float((got - ref).abs().max()) / (scale if scale > 0 else 1.0)


def bound_of(f32, f64):
    return max(4.0 * max_dev(f32, f64), FLOOR)


# ------------------------------------------------------------------------------------------------ fixture G18
@functools.lru_cache(maxsize=None)
def _g18():
    return np.load(GOLDEN, allow_pickle=False)


def g18_tensor(name):
    return torch.from_numpy(_g18()[name].copy())


@functools.lru_cache(maxsize=None)
def g18_state(case):
    """the reference's state dict as constructed: OrderedDict name -> tensor of the reference's shape and dtype"""
    g = _g18()
    values, off, state = g[f"{case}.state_values"], 0, OrderedDict()
    for name, shape, dtype in zip(g[f"{case}.state_names"], g[f"{case}.state_shapes"], g[f"{case}.state_dtypes"]):
        shape = tuple(int(s) for s in str(shape).split("x")) if str(shape) else ()
        count = int(np.prod(shape, dtype=np.int64))
        state[str(name)] = torch.from_numpy(values[off:off + count].copy()).reshape(shape).to(getattr(torch, str(dtype)))
        off += count
    assert off == len(values)
    return state


def g18_param_names(case):
    return [str(n) for n in _g18()[f"{case}.param_names"]]


@functools.lru_cache(maxsize=None)
def g18_grads(case, xk):
    """name -> the reference's gradient of sum(out * cotangent), for the parameters that receive one"""
    g, state = _g18(), g18_state(case)
    values, off, grads = g[f"{case}.{xk}.grad_values"], 0, OrderedDict()
    for name in g[f"{case}.{xk}.grad_names"]:
        shape = state[str(name)].shape
        count = int(np.prod(shape, dtype=np.int64))
        grads[str(name)] = torch.from_numpy(values[off:off + count].copy()).reshape(shape)
        off += count
    assert off == len(values)
    return grads


def g18_module(shw, case):
    """this package's structure of the case's shape, loaded strictly from the reference's state dict"""
    if case == "planar":
        phi = shw.Norm_Flow_structure(3, "Planar", 3)
    elif case == "res":
        phi = shw.Norm_Flow_structure(3, "Residual", 3)
    else:
        phi = shw.Norm_Flow_structure_optuna(3, "Residual", 3, Residual_hidden_units=5, Residual_hidden_layers=3)
    phi.load_state_dict(g18_state(case), strict=True)
    return phi


# ------------------------------------------------------------------------------------------------ random packed parameters
def layer_shapes(hidden, layers, dim=3):
    channels = [dim] + [hidden] * (layers - 1) + [dim]
    return [(channels[k + 1], channels[k]) for k in range(layers)]


@functools.lru_cache(maxsize=None)
def random_packed(hidden, layers, flows, seed=0):
    """float32 packed effective parameters: softplus(beta) with beta around 0.5, weights whose spectral norm alternates
    between 1.3 and 0.7 before the division by max(1, sigma / 0.95) (so about half the layers are normalised), biases of
    order 0.3"""
    g = torch.Generator().manual_seed(1000 * hidden + 100 * layers + flows + seed)
    parts, flip = [], 0
    for _ in range(flows):
        for out, inp in layer_shapes(hidden, layers):
            beta = 0.5 + 0.5 * torch.randn(1, generator=g, dtype=torch.float64)
            w = torch.randn(out, inp, generator=g, dtype=torch.float64)
            sigma = float(torch.linalg.svdvals(w)[0])
            w = w * ((1.3 if flip % 2 == 0 else 0.7) / sigma)
            flip += 1
            sigma = float(torch.linalg.svdvals(w)[0])
            w_eff = w / max(1.0, sigma / COEFF)
            b = 0.3 * torch.randn(out, generator=g, dtype=torch.float64)
            parts += [torch.nn.functional.softplus(beta), w_eff.reshape(-1), b]
    return torch.cat(parts).float()


@functools.lru_cache(maxsize=None)
def points_and_cotangent(shape, seed=0):
    g = torch.Generator().manual_seed(7 + seed + sum(shape))
    return torch.randn(*shape, generator=g), torch.randn(*shape, generator=g)


def composed_reference(shw, x, packed, cot, hidden, layers, flows, dtype):
    """value, d/dx, d/dpacked of sum(composed(x) * cot) in `dtype` on the CPU"""
    xs = x.detach().cpu().to(dtype).requires_grad_()
    ps = packed.detach().cpu().to(dtype).requires_grad_()
    y = shw.residual_flow_composed(xs, ps, hidden, layers, flows)
    (y * cot.detach().cpu().to(dtype)).sum().backward()
    return y.detach(), xs.grad, ps.grad


_REFS = {}


def references(shw, shape, hidden, layers, flows):
    """(x, packed, cot, float64 triple, float32 triple) of a random case, computed once and shared"""
    key = (tuple(shape), hidden, layers, flows)
    if key not in _REFS:
        x, cot = points_and_cotangent(tuple(shape))
        packed = random_packed(hidden, layers, flows)
        _REFS[key] = (x, packed, cot, composed_reference(shw, x, packed, cot, hidden, layers, flows, torch.float64),
                      composed_reference(shw, x, packed, cot, hidden, layers, flows, torch.float32))
    return _REFS[key]
