"""Shared cases of the registration-network tests (tests/test_pcrnet_cpu.py, tests/test_pcrnet_gpu.py) and of
tools/make_golden_pcrnet.py: fixture G19 read back, random trunks, the head's fixed weights, and the float64 / float32
references of the composed path, each computed once.

Error rule (tests/helpers/flow_cases.py): a float32 result is compared with the composed path in float64 on the same
float32 parameters and inputs, per tensor, on max |error| / max |reference entry|; the bound is 4 x the deviation of the
float32 composed CPU path from the float64 one on the same data, with a floor.

Margin condition: a flipped arg-max moves a whole gradient contribution from one point to another, so every case asserts,
in float64, that in every channel of every cloud the best last pre-activation exceeds the best one at a point with other
coordinates by at least MARGIN * max |z5|, and that no channel's best value lies within that distance of 0 (so "dead" means
the same in both precisions).  Seeds are chosen for which this holds (`find_seed` searches them on the CPU)."""
import functools
import os
from collections import OrderedDict

import numpy as np
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "golden", "g19_pcrnet.npz")
FLOOR = 1e-6
MARGIN = 1e-4
POINT_TILE = 64                         # csrc/shw_pointnet.hip kPnPoints
HIDDEN = (64, 64, 64, 128)


def max_dev(got, ref):
    got, ref = torch.as_tensor(got).double().cpu(), torch.as_tensor(ref).double().cpu()
    assert got.shape == ref.shape, (got.shape, ref.shape)
    if ref.numel() == 0:
        return 0.0
    scale = float(ref.abs().max())
    return float((got - ref).abs().max()) / (scale if scale > 0 else 1.0)


def bound_of(f32, f64, floor=FLOOR):
    return max(4.0 * max_dev(f32, f64), floor)


# ------------------------------------------------------------------------------------------------ the head's weights
_LCG_A, _LCG_C, _BLOCK = 1664525, 1013904223, 4096


def lcg_integers(count, seed):
    """`count` integers in [-128, 128): the top byte of s <- 1664525 s + 1013904223 (mod 2^32), s_0 = seed, minus 128.
    The first 4096 states come from the recurrence one by one, the rest from its 4096-step jump, block by block."""
    first = np.empty(_BLOCK, dtype=np.uint64)
    s, a_jump, c_jump = seed & 0xFFFFFFFF, 1, 0
    for k in range(_BLOCK):
        s = (_LCG_A * s + _LCG_C) & 0xFFFFFFFF
        first[k] = s
        a_jump, c_jump = (a_jump * _LCG_A) & 0xFFFFFFFF, (c_jump * _LCG_A + _LCG_C) & 0xFFFFFFFF
    blocks = [first]
    while len(blocks) * _BLOCK < count:
        blocks.append((blocks[-1] * np.uint64(a_jump) + np.uint64(c_jump)) & np.uint64(0xFFFFFFFF))
    states = np.concatenate(blocks)[:count]
    return (states >> np.uint64(24)).astype(np.int64) - 128


def fill_head(model, seed=19):
    """the head's weights and biases: lcg_integers scaled by the power of two nearest to 1 / (128 sqrt(fan_in)), so every
    entry is exact in float32 and lies within 1 / sqrt(fan_in) of 0 up to that rounding.  2.1 M values that no fixture stores."""
    with torch.no_grad():
        for k, layer in enumerate(m for m in model.linear if isinstance(m, torch.nn.Linear)):
            scale = 2.0 ** round(float(np.log2(1.0 / (128.0 * np.sqrt(layer.in_features)))))
            for j, t in enumerate((layer.weight, layer.bias)):
                values = lcg_integers(t.numel(), seed + 100 * k + j).astype(np.float64) * scale
                t.copy_(torch.from_numpy(values).reshape(t.shape).to(t.dtype))
    return model


# ------------------------------------------------------------------------------------------------ random trunks
def layer_shapes(emb):
    channels = (3,) + HIDDEN + (emb,)
    return [(channels[k + 1], channels[k]) for k in range(5)]


@functools.lru_cache(maxsize=None)
def trunk_params(emb, seed=0):
    """float32 packed parameters W1 b1 .. W5 b5: weights uniform in +-sqrt(3 / fan_in) (unit gain: the features keep
    varying from point to point through the five layers, where Conv1d's default range lets the biases dominate and every
    channel's values crowd together), biases uniform in +-0.2"""
    g = torch.Generator().manual_seed(7919 * emb + seed)
    parts = []
    for out, inp in layer_shapes(emb):
        parts += [(torch.rand(out * inp, generator=g, dtype=torch.float64) * 2 - 1) * np.sqrt(3.0 / inp),
                  (torch.rand(out, generator=g, dtype=torch.float64) * 2 - 1) * 0.2]
    return torch.cat(parts).float()


def last_bias_slice(emb):
    total = sum(o * i + o for o, i in layer_shapes(emb))
    return slice(total - emb, total)


def last_weight_slice(emb):
    total = sum(o * i + o for o, i in layer_shapes(emb))
    return slice(total - emb - emb * 128, total - emb)


def preactivation(shw, x, params, emb):
    """z5 (B, N, emb): the last layer before its ReLU, in the dtype of x"""
    layers = shw.unpack_pointnet_params(params, emb)
    h = x
    for weight, bias in layers[:-1]:
        h = torch.relu(torch.nn.functional.linear(h, weight, bias))
    return torch.nn.functional.linear(h, layers[-1][0], layers[-1][1])


def margin_report(x64, z5, live_only=False):
    """(smallest gap of a channel's best value to the best one at a point with other coordinates, smallest |best value|),
    both relative to max |z5|, and the (B, emb) arg-max with ties at the lowest index.  `live_only` leaves the gap of the
    channels whose best value is negative out (the case with a bias of -10: their arg-max carries no gradient and the
    bias inflates max |z5|); the distance from 0 is taken over every channel either way."""
    B, N, emb = z5.shape
    scale = float(z5.abs().max())
    top = z5.max(dim=1)[0]
    index = torch.arange(N).view(1, N, 1).expand(B, N, emb)
    arg = torch.where(z5 == top[:, None, :], index, torch.full_like(index, N)).min(dim=1)[0]
    # points that differ from the arg-max point in some coordinate
    at = torch.gather(x64, 1, arg.reshape(B, -1, 1).expand(B, emb, 3))              # (B, emb, 3)
    other = (x64[:, :, None, :] != at[:, None, :, :]).any(-1)                           # (B, N, emb)
    rest = torch.where(other, z5, torch.full_like(z5, -float("inf"))).max(dim=1)[0]
    gaps = (top - rest) / scale
    if live_only:
        gaps = torch.where(top > 0, gaps, torch.full_like(gaps, float("inf")))
    gap = float(gaps.min()) if N > 1 and bool(other.any()) else float("inf")
    return gap, float((top.abs() / scale).min()), arg


def assert_margin(x, params, emb, shw, what="", live_only=False):
    """the margin condition on float32 data, checked in float64; returns the float64 arg-max"""
    x64, p64 = x.detach().cpu().double(), params.detach().cpu().double()
    gap, away, arg = margin_report(x64, preactivation(shw, x64, p64, emb), live_only)
    assert gap >= MARGIN and away >= MARGIN, (what, gap, away)
    return arg


def reference(shw, x, params, cot, emb, dtype):
    """value, d/dx, d/dparams of sum(composed(x) * cot) in `dtype` on the CPU"""
    xs = x.detach().cpu().to(dtype).requires_grad_()
    ps = params.detach().cpu().to(dtype).requires_grad_()
    y = shw.pointnet_max_features_composed(xs, ps, emb)
    (y * cot.detach().cpu().to(dtype)).sum().backward()
    return y.detach(), xs.grad, ps.grad


def make_inputs(emb, B, N, seed, doubled=False, dead_half=False, copies=0):
    """`copies` > 0: that many clouds, each the case's B = 1 cloud with its points in another order -- the margin
    condition is a property of a cloud's set of points, so it carries over from the one cloud to any number of them"""
    g = torch.Generator().manual_seed(100003 * seed + 1009 * emb + 31 * B + N)
    x = torch.randn(B, N, 3, generator=g)
    if copies:
        assert B == 1
        x = torch.stack([x[0, torch.randperm(N, generator=g)] for _ in range(copies)])
        B = copies
    if doubled:                                     # every point occurs twice: at n and at n + N / 2
        assert N % 2 == 0
        x = torch.cat([x[:, :N // 2], x[:, :N // 2]], dim=1).contiguous()
    cot = torch.randn(B, emb, generator=g)
    params = trunk_params(emb, seed).clone()
    if dead_half:
        bias = params[last_bias_slice(emb)]
        bias[emb // 2:] = -10.0
    return x, params, cot


def find_seed(shw, emb, B, N, doubled=False, dead_half=False, tries=400):
    """the first seed whose case meets the margin condition (used when the cases below were written)"""
    for seed in range(tries):
        x, params, _ = make_inputs(emb, B, N, seed, doubled, dead_half)
        gap, away, _ = margin_report(x.double(), preactivation(shw, x.double(), params.double(), emb), dead_half)
        if gap >= MARGIN and away >= MARGIN:
            return seed
    raise AssertionError((emb, B, N, doubled, dead_half))


_CASES = {}


def case(shw, emb, B, N, seed, doubled=False, dead_half=False, copies=0):
    """dict: x, params, cot (float32), argmax (float64 reference's, lowest index on ties), f64 and f32 triples
    (feat, gx, gparams) of the composed CPU path; computed once and shared.  Asserts the margin condition."""
    key = (emb, B, N, seed, doubled, dead_half, copies)
    if key not in _CASES:
        x, params, cot = make_inputs(emb, B, N, seed, doubled, dead_half, copies)
        arg = assert_margin(x, params, emb, shw, key, live_only=dead_half)
        _CASES[key] = {"x": x, "params": params, "cot": cot, "argmax": arg,
                       "f64": reference(shw, x, params, cot, emb, torch.float64),
                       "f32": reference(shw, x, params, cot, emb, torch.float32)}
    return _CASES[key]


# ------------------------------------------------------------------------------------------------ fixture G19
@functools.lru_cache(maxsize=None)
def g19():
    return np.load(GOLDEN, allow_pickle=False)


def g19_tensor(name):
    return torch.from_numpy(g19()[name].copy())


def g19_trunk_state():
    """conv1.weight .. conv5.bias of the fixture's emb_dims = 64 trunk, in the reference's shapes"""
    return OrderedDict((str(n), g19_tensor(f"trunk.{n}")) for n in g19()["trunk.names"])


def g19_model(shw, dropout=0.0):
    """this package's PCRNet(MLP_Architecture(64)) with the fixture's trunk and the head of `fill_head`"""
    model = shw.PCRNet(shw.MLP_Architecture(64), droput=dropout)
    model.feature_model.load_state_dict(g19_trunk_state(), strict=True)
    return fill_head(model)


def run_pcrnet_checked(shw, model, template, source, k):
    """model(template, source, k) with the margin condition asserted on the input of every trunk call"""
    trunk = model.feature_model
    original = trunk.pooled

    def checked(x, packed=None):
        assert_margin(x, trunk.packed_params() if packed is None else packed, trunk.emb_dims, shw, "PCRNet trunk call")
        return original(x, packed)

    trunk.pooled = checked
    try:
        return model(template, source, k)
    finally:
        del trunk.pooled


def pcrnet_model(shw, seed, emb=64):
    """float32 PCRNet(MLP_Architecture(emb)) with the trunk of `trunk_params(emb, seed)` and the head of `fill_head`"""
    model = shw.PCRNet(shw.MLP_Architecture(emb))
    with torch.no_grad():
        for n, (weight, bias) in enumerate(shw.unpack_pointnet_params(trunk_params(emb, seed), emb), start=1):
            conv = getattr(model.feature_model, f"conv{n}")
            conv.weight.copy_(weight[:, :, None])
            conv.bias.copy_(bias)
    return fill_head(model)


def pcrnet_run(shw, model, template, source, cot, k, checked=False):
    """outputs and name -> gradient of sum(transformed_source * cot) for every parameter, on the model's device / dtype"""
    model.zero_grad()
    runner = (lambda t, s, n: run_pcrnet_checked(shw, model, t, s, n)) if checked else model
    out = runner(template, source, k)
    (out["transformed_source"] * cot).sum().backward()
    return ({name: value.detach() for name, value in out.items()},
            OrderedDict((name, p.grad.detach().clone()) for name, p in model.named_parameters()))


def pcrnet_inputs(seed, B=2, N=130):
    g = torch.Generator().manual_seed(4001 + seed)
    return (torch.randn(B, N, 3, generator=g), torch.randn(B, N, 3, generator=g), torch.randn(B, N, 3, generator=g))


_PCRNET = {}


def pcrnet_case(shw, k, seed):
    """(model float32 on the CPU, template, source, cot, float64 (outputs, grads), float32 CPU (outputs, grads)); the
    float64 run asserts the margin condition on every trunk call"""
    if (k, seed) not in _PCRNET:
        import copy
        model = pcrnet_model(shw, seed)
        template, source, cot = pcrnet_inputs(seed)
        f64 = pcrnet_run(shw, copy.deepcopy(model).double(), template.double(), source.double(), cot.double(), k, checked=True)
        f32 = pcrnet_run(shw, copy.deepcopy(model), template, source, cot, k)
        _PCRNET[(k, seed)] = (model, template, source, cot, f64, f32)
    return _PCRNET[(k, seed)]


def find_pcrnet_seed(shw, k, tries=400):
    for seed in range(tries):
        try:
            pcrnet_case(shw, k, seed)
            return seed
        except AssertionError:
            continue
    raise AssertionError(k)


def named_grads(names, flat, shapes):
    out, off = OrderedDict(), 0
    for n in names:
        count = int(np.prod(shapes[str(n)], dtype=np.int64))
        out[str(n)] = torch.from_numpy(flat[off:off + count].copy()).reshape(shapes[str(n)])
        off += count
    assert off == len(flat)
    return out
