"""GPU checks of the fused sphere encoder (csrc/shw_sphere_map.hip sphere_map_forward_kernel, sphere_map_backward_kernel,
sphere_map_param_reduce_kernel; sphere_map.py sphere_map, transform_to_sphere[_fast]) against the composed path in float64,
against fixture G20 (what the reference's encoder and wrappers computed) and inside the phi-max wrappers.

Bound (tests/helpers/sphere_map_cases.py): a float32 result against the composed path in float64 on the same float32
parameters and inputs, per tensor, on max |error| / max |reference entry|; the bound is 4 x the deviation of the FLOAT32
composed path from the float64 one on the same data, computed here, with a floor of 1e-6.

Every test calls shw.sphere_map, shw.transform_to_sphere[_fast] or a shw_sphere_map_* entry, which did not exist before:
without the feature each fails.

Measured on MI355X (worst over the cases).  Sizes and ranks, values / d/dx / d/dparams: as constructed
2.6e-7 / 3.6e-7 / 7.2e-7 (bounds 1.0e-6 to 1.5e-6), weights x 3 5.6e-7 / 1.1e-6 / 4.5e-7 (1.0e-6 to 5.1e-6), pre-activations
of order 5 2.4e-6 / 3.2e-6 / 1.2e-6 (the float32 composed path: 6.7e-6 / 5.4e-6 / 1.6e-6; bounds 1.0e-6 to 2.7e-5; the one
point of (1, 3) is saturated in every unit, its gradients are 1e-7 of nothing and 2.9e-3 off, as the composed path's are
5e-2).  Two tiles per block, 65 537 points: 6.8e-7 / 3.3e-7 / 5.2e-7.  Special inputs: at most 2.8e-7 / 3.5e-7 / 2.1e-7.
With plain fmaf chains for the pre-activations the special inputs missed at order 5 (d/dx 2.2e-6, bound 1.0e-6; all
unsaturated special points share one set of activations, so one chain's rounding decides): the kernels sum the
pre-activations with one rounding since (csrc/shw_sphere_map.hip dot_rounded_once).  Unit norm: 1.2e-7 (composed 9.9e-8).
Fixture (a): at most 4.3e-7 from float64 and 5.7e-7 from the reference's float32 values (bounds 1.0e-6 to 2.9e-6).
Fixture (b), against the reference's float32 and float64 runs alike: values and trace at most 6.4e-7 (1e-4), parameters
1.1e-6 and maps 2.9e-6 (1e-3), input gradients 2.2e-4 of the largest entry (5e-2), no entry over 2e-3.  Graphed ascent:
bit-identical to the eager one.
"""
import numpy as np
import pytest
import torch

from helpers.sphere_map_cases import (INPUT_SHAPES, NAMES, OFFSET, PARAM_COUNT, PARAM_SETS, bound_of, composed_reference,
                                      g20_module, g20_run, g20_tensor, max_dev, module_results, param_set, references,
                                      special_points, split_params, two_tile_points)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def shw():
    import shw_amd
    shw_amd._lib.load()
    return shw_amd


def fused(shw, x, params, cot, want_x=True, want_p=True):
    """value, d/dx, d/dparams of sum(sphere_map(x) * cot) on the device (None where not asked for)"""
    xd = x.to(DEV).requires_grad_(want_x)
    pd = params.to(DEV).requires_grad_(want_p)
    y = shw.sphere_map(xd, pd)
    assert y.shape == x.shape and y.dtype == torch.float32 and y.is_contiguous()
    (y * cot.to(DEV)).sum().backward()
    return y.detach(), xd.grad, pd.grad


def check(label, got, f64, f32):
    for name, g, r, f in zip(("value", "d/dx", "d/dparams"), got, f64, f32):
        assert torch.isfinite(g).all(), (label, name)
        worst, bound = max_dev(g, r), bound_of(f, r)
        print(f"{label} {name}: gpu {worst:.2e} bound {bound:.2e}")
        assert worst <= bound, (label, name, worst, bound)


# ------------------------------------------------------------------------------------------------ 1
@pytest.mark.parametrize("shape", INPUT_SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("pname", PARAM_SETS)
def test_values_and_gradients_against_float64(shw, pname, shape):
    x, params, cot, f64, f32 = references(shw, shape, pname)
    check(f"{pname} {shape}", fused(shw, x, params, cot), f64, f32)


# ------------------------------------------------------------------------------------------------ 2
def test_two_tiles_per_block_with_a_ragged_last_tile(shw):
    """one point more than 64 x the cap on backward workgroups: workgroup 0 takes a second tile, of one point, and adds
    it to the partial vector its first tile stored; under the rule, and the same bits on a second run"""
    lib = shw._lib.load()
    points = two_tile_points(lib)
    assert lib.shw_sphere_map_backward_blocks(points) * 64 < points
    x, params, cot, f64, f32 = references(shw, (points, 3), "x3")
    first = fused(shw, x, params, cot)
    check(f"two tiles, {points} points", first, f64, f32)
    second = fused(shw, x, params, cot)
    for a, b in zip(first, second):
        assert torch.equal(a, b)


# ------------------------------------------------------------------------------------------------ 3
@pytest.mark.parametrize("pname", ["x3", "order5"])
@pytest.mark.parametrize("shape", [(65, 3), (3, 341, 3)], ids=lambda s: "x".join(map(str, s)))
def test_only_the_gradients_asked_for_and_the_same_bits(shw, shape, pname):
    """points only (the trainer's case), parameters only (the inner ascent's), both: what a variant produces is, bit for
    bit, what `both` produces; and so is the forward under no_grad"""
    x, params, cot, _, _ = references(shw, shape, pname)
    y, gx, gp = fused(shw, x, params, cot)
    y1, gx1, gp1 = fused(shw, x, params, cot, want_p=False)
    y2, gx2, gp2 = fused(shw, x, params, cot, want_x=False)
    assert gp1 is None and gx2 is None
    assert torch.equal(y, y1) and torch.equal(y, y2)
    assert torch.equal(gx, gx1) and torch.equal(gp, gp2)
    with torch.no_grad():
        assert torch.equal(shw.sphere_map(x.to(DEV), params.to(DEV)), y)


# ------------------------------------------------------------------------------------------------ 4
@pytest.mark.parametrize("pname", PARAM_SETS)
def test_special_inputs_stay_finite(shw, pname):
    """+-1e4, +-88, +-50, +-1, +-0 and subnormal coordinates: tanh saturates to exactly +-1, nothing becomes NaN or inf, and
    the results are within the bound of the float64 path"""
    x, cot = special_points()
    params = param_set(pname)
    f64 = composed_reference(shw, x, params, cot, torch.float64)
    f32 = composed_reference(shw, x, params, cot, torch.float32)
    assert all(torch.isfinite(t).all() for t in f64 + f32)
    check(f"special inputs {pname}", fused(shw, x, params, cot), f64, f32)


@pytest.mark.parametrize("sign", [1.0, -1.0])
def test_saturated_first_angle_is_a_pole_with_zero_gradient(shw, sign):
    """b3[0] = +-60: tanh(o0) is exactly +-1 in float32, theta1 is pi or 0, the point is the pole (0, 0, -+1) and nothing
    flows back through t1: the gradients of the first row of W3 and of b3[0] are exactly 0, and d/dx is what the second
    angle alone passes -- 0 as well, since sin theta1 = 0 multiplies it"""
    x, cot = special_points()
    params = param_set("x3").clone()
    params[OFFSET["net.4.bias"]] = 60.0 * sign
    y, gx, gp = fused(shw, x, params, cot)
    assert torch.isfinite(y).all() and torch.isfinite(gx).all() and torch.isfinite(gp).all()
    assert y[:, :2].abs().max() <= 1e-7 and torch.equal(y[:, 2], torch.full_like(y[:, 2], -sign))
    grads = split_params(gp.cpu())
    assert not grads["net.4.weight"][0].any() and grads["net.4.bias"][0] == 0
    f64 = composed_reference(shw, x, params, cot, torch.float64)
    f32 = composed_reference(shw, x, params, cot, torch.float32)
    worst, bound = max_dev(y, f64[0]), bound_of(f32[0], f64[0])
    print(f"pole {sign:+.0f}: value {worst:.2e} bound {bound:.2e}, largest |d/dx| {float(gx.abs().max()):.2e}, "
          f"float64 {float(f64[1].abs().max()):.2e}")
    assert worst <= bound
    assert gx.abs().max() <= 1e-6 * cot.abs().max()             # float64: sin(pi) ~ 1e-16 times the second angle's slope


# ------------------------------------------------------------------------------------------------ 5
@pytest.mark.parametrize("pname", PARAM_SETS)
def test_unit_norm(shw, pname):
    """max | |y| - 1 | at most 4 x the float32 composed path's own worst on the same data, floor 2^-22"""
    x, params, _, _, f32 = references(shw, (4099, 3), pname)
    with torch.no_grad():
        y = shw.sphere_map(x.to(DEV), params.to(DEV))
    off = float((y.double().norm(dim=-1) - 1).abs().max())
    composed = float((f32[0].double().norm(dim=-1) - 1).abs().max())
    print(f"unit norm {pname}: gpu {off:.2e} composed float32 {composed:.2e}")
    assert off <= max(4 * composed, 2.0 ** -22)


# ------------------------------------------------------------------------------------------------ 6
@pytest.mark.parametrize("fast", [False, True], ids=["transform_to_sphere", "transform_to_sphere_fast"])
@pytest.mark.parametrize("scale", ["s1", "s3"])
def test_fixture_a_on_the_device(shw, scale, fast):
    """the module loaded from the reference's state, on the reference's input, fused path: output, d/dx and the six
    parameter gradients against the float64 composed path and against what the reference itself stored (float32), both
    with the rule's bound"""
    x, cot = g20_tensor("a.x"), g20_tensor("a.cot")
    phi = g20_module(shw, scale, fast).to(DEV)
    got = module_results(phi, x.to(DEV), cot)
    assert got[0][1].dtype == torch.float32 and [n for n, _ in got[2:]] == list(NAMES)
    params = g20_tensor(f"a.{scale}.params")
    f64, f32 = ([y, gx] + list(split_params(gp).values())
                for y, gx, gp in (composed_reference(shw, x, params, cot, dt) for dt in (torch.float64, torch.float32)))
    stored = [g20_tensor(f"a.{scale}.out"), g20_tensor(f"a.{scale}.grad_x")]
    stored += list(split_params(g20_tensor(f"a.{scale}.grad_params")).values())
    missed = []
    for (name, g), r, f, s in zip(got, f64, f32, stored):
        bound = bound_of(f, r)
        to64, to_ref = max_dev(g, r), max_dev(g, s)
        print(f"fixture (a) {scale} {name}: gpu to float64 {to64:.2e} to the reference {to_ref:.2e} bound {bound:.2e}")
        if not torch.isfinite(g).all() or to64 > bound or to_ref > bound:
            missed.append((name, to64, to_ref, bound))
    assert not missed, missed


# ------------------------------------------------------------------------------------------------ 7
def test_non_contiguous_input(shw):
    x, params, cot, _, _ = references(shw, (3, 341, 3), "x3")
    wide = torch.zeros(3, 682, 3)
    wide[:, ::2] = x
    wide = wide.to(DEV)
    assert not wide[:, ::2].is_contiguous()
    y, gx, gp = fused(shw, x, params, cot)
    leaf = wide.clone().requires_grad_()
    pd = params.to(DEV).requires_grad_()
    yv = shw.sphere_map(leaf[:, ::2], pd)
    (yv * cot.to(DEV)).sum().backward()
    assert torch.equal(yv.detach(), y) and torch.equal(pd.grad, gp)
    assert torch.equal(leaf.grad[:, ::2], gx) and not leaf.grad[:, 1::2].any()


def test_float64_on_the_device_and_the_refusals(shw):
    x = torch.randn(2, 65, 3, device=DEV)
    params = param_set("x3").to(DEV)
    phi = g20_module(shw, "s3").to(DEV).double()
    with torch.no_grad():
        got = phi(x.double())
        assert got.dtype == torch.float64 and torch.equal(got, shw.sphere_map_composed(x.double(), params.double()))
    phi = phi.float()
    with torch.no_grad():                                           # fused on: the kernels' bits; off: the composed path's
        assert torch.equal(phi(x), shw.sphere_map(x, params))
        phi.fused = False
        assert torch.equal(phi(x), shw.sphere_map_composed(x, params))
    with pytest.raises(ValueError, match="142"):
        shw.sphere_map(x, params[:-1])
    with pytest.raises(ValueError, match="142"):
        shw.sphere_map(x, torch.zeros(PARAM_COUNT + 1, device=DEV))
    with pytest.raises(ValueError):
        shw.sphere_map(torch.randn(65, 4, device=DEV), params)
    with pytest.raises(ValueError):
        shw.sphere_map(torch.randn(65 * 3, device=DEV), params)
    with pytest.raises(TypeError):
        shw.sphere_map(x.double(), params)
    with pytest.raises(TypeError):
        shw.sphere_map(x, params.double())
    with pytest.raises(RuntimeError, match="needs device tensors"):
        shw.sphere_map(x, params.cpu())


# ------------------------------------------------------------------------------------------------ 8
def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.max(np.abs(a - b) / np.maximum(np.abs(b), 1e-30)))


@pytest.mark.parametrize("tag", ["pair", "fast"])
@pytest.mark.parametrize("mode", ["train", "test"])
def test_fixture_b_wrappers_against_the_real_wrappers(shw, tag, mode):
    """Both wrappers, phi the fused module from the x 3 state, the reference's Adam, SSW = this package's sliced_cost on
    the fixture's fixed frames, against what the REAL wrappers did with the REAL encoder -- in float32 and in float64, the
    fixture's own two runs being at least 4 x inside each tolerance of one another.  Tolerances of
    tests/test_r2_gpu.py:66-98: trace and returned value 1e-4 relative, parameters and mapped clouds 1e-3 absolute, input
    gradients max error < 5e-2 scale with fewer than 2 % of the entries over 2e-3 scale."""
    g = {k: g20_tensor(k) for k in ("b.first", "b.second", "b.U_pair", "b.U_batch", "b.lr", "b.betas", "b.max_iter")}
    U = g["b.U_pair" if tag == "pair" else "b.U_batch"].to(DEV)
    cls = shw.max_spherical_wassersten_distance if tag == "pair" else shw.max_spherical_wassersten_distance_fast
    ssw = lambda a, b, L, device, p=2: shw.sliced_cost(a, b, U, p=p)                 # noqa: E731
    phi = g20_module(shw, "s3", fast=tag == "fast").to(DEV)
    assert phi.fused
    opt = torch.optim.Adam(phi.parameters(), lr=float(g["b.lr"]), betas=tuple(float(b) for b in g["b.betas"]))
    crit = cls(U.shape[-3], phi, ssw, opt, p=2, max_iter=int(g["b.max_iter"]), device=DEV)
    trace = []
    crit.on_inner_value = trace.append
    a, b = g["b.first"].to(DEV).requires_grad_(True), g["b.second"].to(DEV).requires_grad_(True)
    val, fa, fb = crit(a, b, train_or_test=mode)
    opt.zero_grad()
    val.sum().backward()                                    # the trainer back-propagates the returned value
    missed = []
    for dtype_name in ("f32", "f64"):
        want = g20_run(dtype_name, tag, mode)
        figures = {"ssw": (rel(val.detach().cpu().numpy().reshape(-1), want["ssw"]), 1e-4)}
        assert len(trace) == len(want["trace"])
        if trace:
            figures["trace"] = (rel(np.array(trace), want["trace"]), 1e-4)
        figures["params"] = (float(np.abs(phi.packed_params().detach().cpu().numpy() - want["params"]).max()), 1e-3)
        figures["phi_first"] = (float(np.abs(fa.detach().cpu().numpy() - want["phi_first"]).max()), 1e-3)
        figures["phi_second"] = (float(np.abs(fb.detach().cpu().numpy() - want["phi_second"]).max()), 1e-3)
        for name, got in (("g_first", a.grad), ("g_second", b.grad)):
            scale = np.abs(want[name]).max()
            err = np.abs(got.cpu().numpy() - want[name])
            figures[name + " max"] = (float(err.max() / scale), 5e-2)
            figures[name + " share over 2e-3"] = (float((err > 2e-3 * scale).mean()), 0.02)
        print(f"fixture (b) {tag} {mode} against {dtype_name}:", {k: f"{v[0]:.1e}" for k, v in figures.items()})
        missed += [(dtype_name, k, v) for k, v in figures.items() if not v[0] < v[1]]
    assert not missed, missed


# ------------------------------------------------------------------------------------------------ 9
def ascent_run(shw, first, second, frames, graph):
    """two trainer-level calls of the batched wrapper (max_iter = 3) from the x 3 state -> the returned values, the
    parameters and the maps of the second call"""
    phi = g20_module(shw, "s3", fast=True).to(DEV)
    opt = torch.optim.Adam(phi.parameters(), lr=0.01, betas=(0.5, 0.999), capturable=True)
    ssw = lambda a, b, L, device, p=2: shw.sliced_cost(a, b, frames, p=p)            # noqa: E731
    crit = shw.max_spherical_wassersten_distance_fast(16, phi, ssw, opt, p=2, max_iter=3, device=DEV, graph=graph)
    trace, values = [], []
    crit.on_inner_value = trace.append
    for _ in range(2):
        val, fa, fb = crit(first, second, "train")
        values.append(val.detach().clone())
    if graph:
        assert len(crit._graphed._graphs) == 1               # captured during the first call, replayed since
    return torch.stack(values), torch.tensor(trace), phi.packed_params().detach().clone(), fa.detach(), fb.detach()


def test_graphed_ascent_gives_the_bits_of_the_eager_one(shw):
    """max_spherical_wassersten_distance_fast(graph=True) with Adam(capturable=True): the first call runs two eager
    iterations and captures the third, the second call is three replays; values, the per-iteration trace, the
    parameters and the maps equal the eager run's bit for bit"""
    first, second, frames = (g20_tensor(k).to(DEV) for k in ("b.first", "b.second", "b.U_batch"))
    eager = ascent_run(shw, first, second, frames, graph=False)
    graphed = ascent_run(shw, first, second, frames, graph=True)
    assert len(eager[1]) == 6
    for name, e, r in zip(("values", "trace", "parameters", "phi(first)", "phi(second)"), eager, graphed):
        assert torch.isfinite(e).all() and torch.equal(e, r), name
    assert not torch.equal(eager[2].cpu(), param_set("x3"))      # the ascent moved phi
