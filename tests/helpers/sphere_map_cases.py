"""Shared cases of the sphere-encoder tests (tests/test_sphere_map_cpu.py, tests/test_sphere_map_gpu.py): fixture G20 read
back into tensors (tools/make_golden_sphere_map.py wrote it), the three parameter sets, and the float64 / float32
references of the composed path, each computed once.

Error rule (tests/helpers/flow_cases.py): a float32 result is compared with the composed path in float64
on the same float32 parameters and inputs, per tensor, on max |error| / max |reference entry|; the bound is 4 x the
deviation of the float32 composed path from the float64 one on the same data, with a floor of 1e-6."""
import functools
import os
from collections import OrderedDict

import numpy as np
import torch

from helpers.flow_cases import bound_of, max_dev  # noqa: F401  (the rule itself, re-exported)

GOLDEN = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "golden", "g20_sphere_map.npz")
PARAM_COUNT = 142
SHAPES = ((16, 3), (16,), (4, 16), (4,), (2, 4), (2,))
NAMES = ("net.0.weight", "net.0.bias", "net.2.weight", "net.2.bias", "net.4.weight", "net.4.bias")
OFFSET = dict(zip(NAMES, (0, 48, 64, 128, 132, 140)))
# point counts 1, 63, 64, 65, 257, 3 x 341, 4099 (lane, wave and block edges, several blocks with a ragged last one), in
# both input ranks
INPUT_SHAPES = [(1, 3), (1, 63, 3), (64, 3), (5, 13, 3), (257, 3), (3, 341, 3), (4099, 3)]
PARAM_SETS = ("init", "x3", "order5")


# ------------------------------------------------------------------------------------------------ fixture G20
@functools.lru_cache(maxsize=None)
def _g20():
    return np.load(GOLDEN, allow_pickle=False)


def g20_tensor(name):
    return torch.from_numpy(np.array(_g20()[name]))


def split_params(flat):
    """flat (142,) -> OrderedDict state-dict name -> tensor of the reference's shape"""
    flat = torch.as_tensor(flat)
    assert flat.shape == (PARAM_COUNT,), flat.shape
    parts = flat.split([int(np.prod(s)) for s in SHAPES])
    return OrderedDict((n, p.reshape(s).clone()) for n, p, s in zip(NAMES, parts, SHAPES))


def g20_state(scale):
    """the reference's state dict: "s1" as constructed from seed 0, "s3" the same with every weight x 3"""
    g = _g20()
    assert tuple(str(n) for n in g["a.state_names"]) == NAMES
    assert tuple(tuple(int(v) for v in str(s).split("x")) for s in g["a.state_shapes"]) == SHAPES
    return split_params(g20_tensor(f"a.{scale}.params"))


def g20_module(shw, scale, fast=False):
    phi = shw.transform_to_sphere_fast() if fast else shw.transform_to_sphere()
    phi.load_state_dict(g20_state(scale), strict=True)
    return phi


def g20_run(dtype_name, tag, mode):
    """what the reference's wrapper `tag` ("pair" / "fast") left in `mode`, run in `dtype_name` ("f32" / "f64"): dict of
    ssw, trace, params, phi_first, phi_second, g_first, g_second (numpy)"""
    g = _g20()
    flat, off, run = g[f"b.{dtype_name}.{tag}_{mode}"], 0, {"trace": np.zeros(0)}
    for name, shape in zip(g[f"b.fields_{mode}"], g[f"b.shapes_{mode}"]):
        shape = tuple(int(v) for v in str(shape).split("x"))
        count = int(np.prod(shape))
        run[str(name)] = flat[off:off + count].reshape(shape)
        off += count
    assert off == len(flat)
    if mode == "test":
        run["phi_first"], run["phi_second"] = g[f"b.{dtype_name}.test.phi_first"], g[f"b.{dtype_name}.test.phi_second"]
    return run


# ------------------------------------------------------------------------------------------------ parameter sets
@functools.lru_cache(maxsize=None)
def param_set(name):
    """flat float32 parameters: "init" the reference's state as constructed, "x3" its weights x 3, "order5" random with
    pre-activations of order 5 in every layer for points of order 1 (most units saturated, some not)"""
    if name == "init":
        return g20_tensor("a.s1.params")
    if name == "x3":
        return g20_tensor("a.s3.params")
    assert name == "order5"
    g = torch.Generator().manual_seed(55)
    parts = []
    for (out, inp), sigma in zip(SHAPES[0::2], (5.0 / 3 ** 0.5, 5.0 / 4, 5.0 / 2)):
        parts += [sigma * torch.randn(out * inp, generator=g), torch.randn(out, generator=g)]
    return torch.cat(parts)


@functools.lru_cache(maxsize=None)
def points_and_cotangent(shape, seed=0):
    g = torch.Generator().manual_seed(20 + seed + sum(shape))
    return torch.randn(*shape, generator=g), torch.randn(*shape, generator=g)


def special_points():
    """130 points drawn from +-1e4, +-88, +-50, +-1, +-0 and subnormals, every value on every coordinate at least once"""
    special = torch.tensor([1e4, -1e4, 88.0, -88.0, 50.0, -50.0, 1.0, -1.0, 0.0, -0.0, 1e-40, -1e-40, 3e-39])
    g = torch.Generator().manual_seed(5)
    x = special[torch.randint(len(special), (130, 3), generator=g)]
    x[:len(special)] = special[:, None]
    return x, torch.randn(130, 3, generator=g)


def composed_reference(shw, x, params, cot, dtype):
    """value, d/dx, d/dparams of sum(composed(x) * cot) in `dtype` on the CPU"""
    xs = x.detach().cpu().to(dtype).requires_grad_()
    ps = params.detach().cpu().to(dtype).requires_grad_()
    y = shw.sphere_map_composed(xs, ps)
    (y * cot.detach().cpu().to(dtype)).sum().backward()
    return y.detach(), xs.grad, ps.grad


_REFS = {}


def references(shw, shape, pname):
    """(x, params, cot, float64 triple, float32 triple) of a case, computed once and shared"""
    key = (tuple(shape), pname)
    if key not in _REFS:
        x, cot = points_and_cotangent(tuple(shape))
        params = param_set(pname)
        _REFS[key] = (x, params, cot, composed_reference(shw, x, params, cot, torch.float64),
                      composed_reference(shw, x, params, cot, torch.float32))
    return _REFS[key]


def module_results(phi, x, cot):
    """[(name, tensor)] of the module's output, d/dx and its six parameter gradients of sum(phi(x) * cot), on the CPU"""
    x = x.detach().clone().requires_grad_()
    phi.zero_grad()
    y = phi(x)
    (y * cot.to(x.device, x.dtype)).sum().backward()
    return ([("value", y.detach().cpu()), ("d/dx", x.grad.cpu())]
            + [(n, p.grad.detach().cpu()) for n, p in phi.named_parameters()])


def two_tile_points(lib):
    """the smallest point count at which some backward workgroup takes two tiles and the last tile is ragged"""
    cap = lib.shw_sphere_map_backward_blocks(1 << 40)
    points = 64 * cap + 1
    assert lib.shw_sphere_map_backward_blocks(points) == cap == lib.shw_sphere_map_backward_blocks(points - 1)
    assert lib.shw_sphere_map_backward_blocks(64 * cap - 63) == cap and lib.shw_sphere_map_backward_blocks(64 * cap - 64) == cap - 1
    return points
