"""Shared cases of the Residual-MSSW tests (tests/test_mssw_cpu.py, tests/test_mssw_gpu.py): fixture G21 read back into
tensors (tools/make_golden_mssw.py wrote it), the parameter sets of the fused op, and the float64 / float32 references of
the composed path, each computed once.

Error rule (tests/helpers/sphere_map_cases.py): a float32 result is compared with the composed path in float64 on the same
float32 parameters and inputs, per tensor, on max |error| / max |reference entry|; the bound is 4 x the deviation of the
float32 composed path from the float64 one on the same data, with a floor of 1e-6.

The ReLU kinks: a point one of whose 16 encoder pre-activations is within rounding of zero may land on the other side in
float32, and its gradient is then wrong by a whole unit, in the composed float32 path as much as in the kernel.  `keep_mask`
finds, in float64, the points with |pre| < 1e-5 (sum |w_i z_i| + |b|) in any unit -- 20 to 100 x the rounding of an 8-term
float32 sum -- and `references` sets the cotangent of those points to zero, which removes them from every gradient on both
sides alike; it asserts that at most 1 % of a case's points went.
"""
import functools
import os
from collections import OrderedDict

import numpy as np
import torch

from helpers.flow_cases import bound_of, max_dev  # noqa: F401  (the rule itself, re-exported)

GOLDEN = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "golden", "g21_mssw.npz")
ENC_COUNT, FLOW_COUNT, MAX_FLOWS = 122, 24, 8
ENC_SHAPES = ((8, 3), (8,), (8, 8), (8,), (2, 8), (2,))
CASES = {"res2": ("Residual", 2), "res3": ("Residual", 3), "planar3": ("Planar", 3)}
VARIANTS = [("res2", "init"), ("res2", "pert"), ("res3", "init"), ("res3", "pert"), ("planar3", "init")]
# (B, N): one point, a batch on one index, a ragged second wave, exactly one wave per cloud, several blocks with tiles
# that straddle clouds, many clouds of few points
SHAPES = [(1, 1), (2, 1), (1, 65), (2, 64), (3, 341), (257, 3)]
FLOWS = [1, 2, 3, 8]
PARAM_SETS = ("init", "pert", "x3", "affine1")
KINK_MARGIN, KINK_CAP = 1e-5, 0.01


def param_count(flows):
    return ENC_COUNT + FLOW_COUNT * flows


# ------------------------------------------------------------------------------------------------ fixture G21
@functools.lru_cache(maxsize=None)
def _g21():
    return np.load(GOLDEN, allow_pickle=False)


def g21_tensor(name):
    return torch.from_numpy(np.array(_g21()[name]))


def g21_names(case, var, what="state_names"):
    return [str(n) for n in _g21()[f"a.{case}.{var}.{what}"]]


@functools.lru_cache(maxsize=None)
def g21_state(case, var, dname, which):
    """the reference's state dict before (`which` 0) or after (1) its first forward, run in `dname` ("f32" / "f64")"""
    g = _g21()
    dtype = torch.float32 if dname == "f32" else torch.float64
    values, off, state = g[f"a.{case}.{var}.{dname}.state{which}"], 0, OrderedDict()
    for name, shape in zip(g21_names(case, var), g[f"a.{case}.{var}.{dname}.state{which}_shapes"]):
        shape = tuple(int(s) for s in str(shape).split("x")) if str(shape) else ()
        count = int(np.prod(shape, dtype=np.int64))
        t = torch.from_numpy(values[off:off + count].copy()).reshape(shape)
        state[name] = t if name.endswith("geom_p") else t.to(dtype)     # geom_p is float64 in the reference
        off += count
    assert off == len(values)
    return state


def g21_grads(case, var, dname):
    """name -> the reference's gradient of sum(out * cotangent), for the parameters that receive one"""
    g, state = _g21(), g21_state(case, var, dname, 1)
    values, off, grads = g[f"a.{case}.{var}.{dname}.grad_values"], 0, OrderedDict()
    for name in g[f"a.{case}.{var}.{dname}.grad_names"]:
        shape = state[str(name)].shape
        count = int(np.prod(shape, dtype=np.int64))
        grads[str(name)] = torch.from_numpy(values[off:off + count].copy()).reshape(shape)
        off += count
    assert off == len(values)
    return grads


def g21_module(shw, case, var="init", dname="f32", which=0, reverse=True):
    """this package's module of the case, strictly loaded from the reference's state; reverse=False: the same parameters
    with the residual blocks applied forward, the direction the fused path covers"""
    flow_name, n_flow_layer = CASES[case]
    phi = shw.mssw.transform_to_sphere(flow_name, n_flow_layer=n_flow_layer, reverse=reverse)
    if dname == "f64":
        phi = phi.double()
    phi.load_state_dict(g21_state(case, var, dname, which), strict=True)
    return phi


def module_results(phi, x, cot):
    """OrderedDict of the module's output, d/dx and its parameter gradients of sum(phi(x) * cot), on the CPU"""
    x = x.detach().clone().requires_grad_()
    phi.zero_grad()
    y = phi(x)
    (y * cot.to(x.device, x.dtype)).sum().backward()
    out = OrderedDict([("value", y.detach().cpu()), ("d/dx", x.grad.cpu())])
    out.update((n, p.grad.detach().cpu()) for n, p in phi.named_parameters() if p.grad is not None)
    return out


def g21_run(dname, mode):
    """what the reference's wrapper left in `mode`, run in `dname`: dict of numpy arrays"""
    g = _g21()
    return {k: g[f"b.{dname}.{mode}.{k}"] for k in ("ssw", "trace", "indices", "params", "phi_first", "phi_second",
                                                      "g_first", "g_second")}


def g21_wrapper_module(shw, dtype=torch.float32, reverse=True):
    """phi of fixture (b) before its initialising call: case res2, variant pert"""
    return g21_module(shw, "res2", "pert", reverse=reverse).to(dtype)


def fixture_b_tolerances(mode):
    """per quantity, the larger of 4 x the gap between the fixture's float32 and float64 runs and the tolerances of
    tests/test_r2_gpu.py:66-98 (1e-4 relative; 1e-3 absolute; gradients 5e-2 of scale with under 2 % of the entries over
    2e-3 of scale); the gaps themselves are returned too"""
    a, b = g21_run("f32", mode), g21_run("f64", mode)
    gaps = {"ssw": float(np.max(np.abs(a["ssw"] - b["ssw"]) / np.abs(b["ssw"])))}
    gaps["trace"] = float(np.max(np.abs(a["trace"] - b["trace"]) / np.abs(b["trace"]))) if len(b["trace"]) else 0.0
    gaps["params"] = float(np.abs(a["params"] - b["params"]).max())
    gaps["maps"] = max(float(np.abs(a[k] - b[k]).max()) for k in ("phi_first", "phi_second"))
    gaps["grad max"] = max(float(np.abs(a[k] - b[k]).max() / np.abs(b[k]).max()) for k in ("g_first", "g_second"))
    gaps["grad share"] = max(float((np.abs(a[k] - b[k]) > 2e-3 * np.abs(b[k]).max()).mean()) for k in ("g_first", "g_second"))
    floor = {"ssw": 1e-4, "trace": 1e-4, "params": 1e-3, "maps": 1e-3, "grad max": 5e-2, "grad share": 0.02}
    return {k: max(4 * gaps[k], floor[k]) for k in floor}, gaps


def fixture_b_figures(val, trace, params, fa, fb, ga, gb, want):
    """the figures `fixture_b_tolerances` bounds, of a run against a stored one"""
    num = lambda t: np.asarray(t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else t, dtype=np.float64)  # noqa: E731
    fig = {"ssw": float(np.max(np.abs(num(val).reshape(-1) - want["ssw"]) / np.abs(want["ssw"])))}
    assert len(trace) == len(want["trace"])
    if len(trace):
        fig["trace"] = float(np.max(np.abs(num(trace) - want["trace"]) / np.abs(want["trace"])))
    fig["params"] = float(np.abs(num(params) - want["params"]).max())
    fig["maps"] = max(float(np.abs(num(fa) - want["phi_first"]).max()), float(np.abs(num(fb) - want["phi_second"]).max()))
    errs = [(np.abs(num(g) - want[k]), np.abs(want[k]).max()) for g, k in ((ga, "g_first"), (gb, "g_second"))]
    fig["grad max"] = max(float(e.max() / s) for e, s in errs)
    fig["grad share"] = max(float((e > 2e-3 * s).mean()) for e, s in errs)
    return fig


def flat_parameters(phi):
    return torch.cat([p.detach().double().reshape(-1).cpu() for p in phi.parameters()])


# ------------------------------------------------------------------------------------------------ parameter sets
def perturb_(phi, factor=1.0):
    """the fixture's perturbation of the i-ResNet weights (tools/make_golden_mssw.py), then the encoder's weights and each
    block's first layer x `factor` (the second layer stays under the clamp)"""
    turn = 0
    with torch.no_grad():
        for name, p in phi.named_parameters():
            if ".iresblock.nnet.net." in name and name.endswith(".weight"):
                if name.endswith("net.3.weight"):
                    p *= 1000.0
                p *= 2.0 if turn % 2 == 0 else 0.6
                turn += 1
            elif name.endswith(".beta"):
                p += 0.3 if turn % 2 else -0.2
            if name.endswith(".weight") and not name.endswith("net.3.weight"):
                p *= factor


@functools.lru_cache(maxsize=None)
def param_set(shw, name, flows, points):
    """(params (122 + 24 flows,), affine (flows, points, 4)), float32.  "init": the module as constructed from seed 0, its
    ActNorm layers initialised on four random clouds; "pert": the i-ResNet weights perturbed as in the fixture first;
    "x3": the encoder's weights and each block's first layer x 3 on top, both branches of max(1, sigma / 0.9) present; "affine1": as "pert", s and
    t random of order 1"""
    torch.manual_seed(0)
    phi = shw.mssw.transform_to_sphere("Residual", n_flow_layer=flows, reverse=False)
    if name != "init":
        perturb_(phi, 3.0 if name == "x3" else 1.0)
    g = torch.Generator().manual_seed(100 * flows + points)
    with torch.no_grad():
        phi(torch.randn(4, points, 3, generator=g))
        if name == "x3":
            sigma = [float(m.scale) for m in phi.modules() if hasattr(m, "scale")]
            assert any(s > 0.9 for s in sigma) and any(s < 0.9 for s in sigma), sigma
        affine = phi.packed_affine()
        if name == "affine1":
            affine = torch.randn(affine.shape, generator=g)
        return phi.packed_params().clone(), affine.clone()


@functools.lru_cache(maxsize=None)
def points_and_cotangent(shape, seed=0):
    g = torch.Generator().manual_seed(21 + seed + 1000 * shape[0] + shape[1])
    return torch.randn(*shape, 3, generator=g), torch.randn(*shape, 3, generator=g)


def special_points():
    """(2, 65, 3) points drawn from +-1e4, +-88, +-1, +-0 and subnormals, every value on every coordinate at least once"""
    special = torch.tensor([1e4, -1e4, 88.0, -88.0, 1.0, -1.0, 0.0, -0.0, 1e-40, -1e-40, 3e-39])
    g = torch.Generator().manual_seed(5)
    x = special[torch.randint(len(special), (130, 3), generator=g)]
    x[:len(special)] = special[:, None]
    return x.reshape(2, 65, 3).clone(), torch.randn(2, 65, 3, generator=g)


def keep_mask(x, params):
    """(B, N) bool: False where one of the 16 ReLU pre-activations is, in float64, within KINK_MARGIN of its kink"""
    p = params.detach().cpu().double()
    off, z, keep = 0, x.detach().cpu().double(), torch.ones(x.shape[:-1], dtype=torch.bool)
    for k, ((out, inp), _) in enumerate(zip(ENC_SHAPES[0::2], ENC_SHAPES[1::2])):
        w, b = p[off:off + out * inp].view(out, inp), p[off + out * inp:off + out * inp + out]
        off += out * inp + out
        pre = z @ w.t() + b
        mass = z.abs() @ w.abs().t() + b.abs()
        if k < 2:
            keep &= (pre.abs() >= KINK_MARGIN * mass).all(-1)
            z = pre.clamp_min(0)
    return keep


def composed_reference(shw, x, params, affine, cot, flows, dtype):
    """value, d/dx, d/dparams, d/daffine of sum(composed(x) * cot) in `dtype` on the CPU"""
    xs, ps, fs = (t.detach().cpu().to(dtype).requires_grad_() for t in (x, params, affine))
    y = shw.residual_sphere_map_composed(xs, ps, fs, flows)
    (y * cot.detach().cpu().to(dtype)).sum().backward()
    return y.detach(), xs.grad, ps.grad, fs.grad


def masked_cotangent(x, params, cot):
    keep = keep_mask(x, params)
    dropped = int((~keep).sum())
    assert dropped <= KINK_CAP * keep.numel(), (dropped, keep.numel())
    return cot * keep[..., None]


_REFS = {}


def references(shw, shape, flows, pname):
    """(x, params, affine, cot, float64 quadruple, float32 quadruple) of a case, computed once and shared; the cotangent
    is zero at the points `keep_mask` drops"""
    key = (tuple(shape), flows, pname)
    if key not in _REFS:
        x, cot = points_and_cotangent(tuple(shape))
        params, affine = param_set(shw, pname, flows, shape[1])
        cot = masked_cotangent(x, params, cot)
        _REFS[key] = (x, params, affine, cot, composed_reference(shw, x, params, affine, cot, flows, torch.float64),
                      composed_reference(shw, x, params, affine, cot, flows, torch.float32))
    return _REFS[key]


def two_tile_points(lib):
    """the smallest point count at which some backward workgroup takes two tiles and the last tile is ragged"""
    cap = lib.shw_mssw_backward_blocks(1 << 40)
    points = 64 * cap + 1
    assert lib.shw_mssw_backward_blocks(points) == cap == lib.shw_mssw_backward_blocks(points - 1)
    assert lib.shw_mssw_backward_blocks(64 * cap - 63) == cap and lib.shw_mssw_backward_blocks(64 * cap - 64) == cap - 1
    return points
