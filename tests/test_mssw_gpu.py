"""GPU checks of the Residual-MSSW sphere encoder (csrc/shw_mssw.hip mssw_forward_kernel, mssw_backward_kernel,
mssw_param_reduce_kernel, mssw_affine_reduce_kernel; mssw.py residual_sphere_map, transform_to_sphere,
max_spherical_wassersten_distance_Residual) against the composed path in float64, against fixture G21 (what the
reference's own module and wrapper computed) and inside the wrapper.

Every test calls shw.residual_sphere_map, shw.mssw or a shw_mssw_* entry, which did not exist before: without the feature
each fails.

Bound of the fused op (tests/helpers/mssw_cases.py): a float32 result against the composed path in float64 on the same
float32 parameters and inputs, per tensor, on max |error| / max |reference entry|; the bound is 4 x the deviation of the
FLOAT32 composed path from the float64 one on the same data, computed here, with a floor of 1e-6.  Points within 1e-5 of a
ReLU kink carry a zero cotangent (at most 1 % of a case; the helper asserts it).  The module on the device against fixture
(a): 4 x the deviation of the reference's own float32 run from its float64 run, floor 1e-6.  The wrapper against fixture
(b): per quantity the larger of 4 x the gap between the fixture's two runs and the tolerances of
tests/test_r2_gpu.py:66-98, computed from the fixture (helpers.mssw_cases.fixture_b_tolerances; the gaps: DESIGN.md 3.19).

Measured on MI355X.  Sizes (1, 1), (2, 1), (1, 65), (2, 64), (3, 341), (257, 3), each with
F in {1, 2, 3, 8}; values / d/dx / d/dparams / d/daffine, worst figure over the 24 cases and, in brackets, the worst share
of a bound: as constructed with data-initialised ActNorm 3.5e-7 / 3.2e-7 / 8.8e-7 / 6.4e-7 (0.17); perturbed i-ResNet
weights 3.7e-7 / 3.3e-7 / 1.6e-6 / 8.3e-7 (0.17); weights x 3 with both clamp branches 3.2e-7 / 1.4e-6 / 1.1e-6 / 1.6e-6 (0.56);
`s`, `t` random of order 1 3.7e-7 / 2.0e-5 / 1.1e-4 / 1.1e-4 (0.34).
One point more than 64 x 1024 (B = 1): 3.8e-7 / 1.2e-7 / 1.5e-6 / 2.3e-7 (bounds 1.2e-4 to 4.1e-4), the same bits on a second
run.  The kink case: d/dx and the gradients of W1, b1, W2, b2, W3 exactly 0 on the device as in torch.  Special inputs
(+-1e4, +-88, +-1, +-0, subnormals): finite, at most 6.6e-7 (bounds 1.4e-6 to 4.5e-5); unit norm 1.04e-7 (composed float32
4.2e-8, floor 2.4e-7).  Every subset of the three gradients and the forward under no_grad: the bits of the full call.
On the device (reversed blocks composed, the HIP sliced loss, the stored minibatches) against the reference's float32 /
float64 run: train -- value 1.1e-7 / 2.7e-7, trace 2.1e-7 / 3.3e-7, parameters 3.6e-5 / 4.0e-5, maps 1.7e-5 / 2.2e-5, input
gradients 5.4e-6 / 7.0e-5; test -- 0 / 5.5e-8, 3.4e-5 / 3.9e-5, 6.9e-6 / 5.1e-6, 2.0e-5 / 4.1e-3 with 0.28 % over 2e-3
(tolerances 1e-4, 1e-4, 1e-3, 1e-3, 5e-2, 2 %: the larger of 4 x the gaps and the floor of tests/test_r2_gpu.py is the floor
everywhere).  Fixture (a) on the device: float64 within 9.1e-9 of the stored float64 run on every tensor; float32 output
and d/dx within 1.4e-5 (bounds 2.1e-6 to 3.6e-5).  Forward blocks in the wrapper, fused against composed, gradient steps:
train -- value 5.5e-7, trace 8.6e-7, parameters 3.2e-8, maps 1.5e-5, input gradients 7.7e-4; test -- 1.1e-7, 0, 1.1e-5, 5.6e-3
with 0.14 % over 2e-3; the subset map gives the figures of the full map.  With Adam the same comparison is meaningless
for this phi: composed against composed, subset map against full map, parameters 1.4e-4 and maps 4.4e-2 -- Adam's first steps
are `lr g / (|g| + 1e-8)`, which turns a rounding-level difference in a small gradient entry into a step of order `lr`,
and the map multiplies a parameter difference by the product of its `1 / std` scales.
With float32 arithmetic in the kernels (one rounding per encoder pre-activation, fmaf chains in the blocks) the case
(1, 1), F = 1, perturbed weights missed: d/dparams 2.06e-6 against 1.29e-6, d/daffine 2.03e-6 against 1.12e-6; the kernels
evaluate the network in float64 since, and the same case measures 3.4e-8 and 6.1e-8.
"""
import numpy as np
import pytest
import torch

from helpers.mssw_cases import (FLOWS, PARAM_SETS, SHAPES, VARIANTS, bound_of, composed_reference, fixture_b_figures,
                                fixture_b_tolerances, flat_parameters, g21_grads, g21_module, g21_run, g21_tensor,
                                g21_wrapper_module, masked_cotangent, max_dev, module_results, param_count, param_set,
                                references, special_points, two_tile_points)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAMES = ("value", "d/dx", "d/dparams", "d/daffine")


@pytest.fixture(scope="module")
def shw():
    import shw_amd
    shw_amd._lib.load()
    return shw_amd


def fused(shw, x, params, affine, cot, flows, want=(True, True, True)):
    """value, d/dx, d/dparams, d/daffine of sum(residual_sphere_map(x) * cot) on the device (None where not asked for)"""
    leaves = [t.detach().to(DEV).clone().requires_grad_(w) for t, w in zip((x, params, affine), want)]
    y = shw.residual_sphere_map(*leaves, flows)
    assert y.shape == x.shape and y.dtype == torch.float32 and y.is_contiguous()
    if any(want):
        (y * cot.to(DEV)).sum().backward()
    return (y.detach(),) + tuple(t.grad for t in leaves)


def misses(label, got, f64, f32):
    out = []
    for name, g, r, f in zip(NAMES, got, f64, f32):
        worst, bound = max_dev(g, r), bound_of(f, r)
        print(f"{label} {name}: gpu {worst:.2e} bound {bound:.2e}")
        if not torch.isfinite(g).all() or worst > bound:
            out.append((label, name, worst, bound))
    return out


# ------------------------------------------------------------------------------------------------ 1
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("flows", FLOWS)
def test_values_and_gradients_against_float64(shw, flows, shape):
    missed = []
    for pname in PARAM_SETS:
        x, params, affine, cot, f64, f32 = references(shw, shape, flows, pname)
        missed += misses(f"{pname} {shape} F={flows}", fused(shw, x, params, affine, cot, flows), f64, f32)
    assert not missed, missed


# ------------------------------------------------------------------------------------------------ 2
def test_two_tiles_per_block_with_a_ragged_last_tile(shw):
    """B = 1 and one point more than 64 x the cap on backward workgroups: workgroup 0 takes a second tile, of one point,
    and adds it to the partial vector its first tile stored; under the rule, and the same bits on a second run"""
    lib = shw._lib.load()
    points = two_tile_points(lib)
    assert lib.shw_mssw_backward_blocks(points) * 64 < points
    x, params, affine, cot, f64, f32 = references(shw, (1, points), 2, "pert")
    first = fused(shw, x, params, affine, cot, 2)
    assert not misses(f"two tiles, {points} points", first, f64, f32)
    second = fused(shw, x, params, affine, cot, 2)
    for a, b in zip(first, second):
        assert torch.equal(a, b)


# ------------------------------------------------------------------------------------------------ 3
def test_the_relu_slope_at_exactly_zero_is_zero(shw):
    """points at exactly 0 and zero encoder biases: all 16 pre-activations are exactly 0 on both paths, and torch's slope
    there is 0: nothing passes the ReLUs, so d/dx and the gradients of W1, b1, W2, b2 are exactly 0, and so is that of W3
    (it multiplies h2 = 0); b3 and the flows receive theirs"""
    params, affine = (t.clone() for t in param_set(shw, "pert", 2, 65))
    params[24:32] = 0
    params[96:104] = 0
    x = torch.zeros(2, 65, 3)
    cot = torch.randn(2, 65, 3, generator=torch.Generator().manual_seed(3))
    got = fused(shw, x, params, affine, cot, 2)
    f64 = composed_reference(shw, x, params, affine, cot, 2, torch.float64)
    f32 = composed_reference(shw, x, params, affine, cot, 2, torch.float32)
    for g in (got, f32, f64):
        assert not g[1].any() and not g[2][:120].any()
        assert g[2][120:].abs().min() > 0 and g[3].abs().max() > 0
    assert not misses("kink", got, f64, f32)


# ------------------------------------------------------------------------------------------------ 4
@pytest.mark.parametrize("shape", [(1, 65), (3, 341)], ids=lambda s: "x".join(map(str, s)))
def test_only_the_gradients_asked_for_and_the_same_bits(shw, shape):
    """every subset of the three gradients: what a variant produces is, bit for bit, what `all three` produces; and so is
    the forward under no_grad"""
    x, params, affine, cot, _, _ = references(shw, shape, 3, "x3")
    full = fused(shw, x, params, affine, cot, 3)
    for want in ((True, False, False), (False, True, False), (False, False, True), (True, True, False), (False, True, True)):
        got = fused(shw, x, params, affine, cot, 3, want)
        assert torch.equal(got[0], full[0])
        for w, g, f in zip(want, got[1:], full[1:]):
            assert (g is None) if not w else torch.equal(g, f), want
    with torch.no_grad():
        assert torch.equal(shw.residual_sphere_map(x.to(DEV), params.to(DEV), affine.to(DEV), 3), full[0])


# ------------------------------------------------------------------------------------------------ 5
@pytest.mark.parametrize("pname", PARAM_SETS)
def test_special_inputs_stay_finite_and_on_the_sphere(shw, pname):
    """+-1e4, +-88, +-1, +-0 and subnormal coordinates: nothing becomes NaN or inf, the results are within the bound of
    the float64 path, and | |y| - 1 | is at most 4 x the float32 composed path's own worst, floor 2^-22"""
    x, cot = special_points()
    params, affine = param_set(shw, pname, 3, 65)
    cot = masked_cotangent(x, params, cot)
    f64 = composed_reference(shw, x, params, affine, cot, 3, torch.float64)
    f32 = composed_reference(shw, x, params, affine, cot, 3, torch.float32)
    assert all(torch.isfinite(t).all() for t in f64 + f32)
    got = fused(shw, x, params, affine, cot, 3)
    assert not misses(f"special inputs {pname}", got, f64, f32)
    off = float((got[0].double().norm(dim=-1) - 1).abs().max())
    composed = float((f32[0].double().norm(dim=-1) - 1).abs().max())
    print(f"unit norm {pname}: gpu {off:.2e} composed float32 {composed:.2e}")
    assert off <= max(4 * composed, 2.0 ** -22)


# ------------------------------------------------------------------------------------------------ 6
@pytest.mark.parametrize("variant", VARIANTS, ids="-".join)
def test_fixture_a_on_the_device(shw, variant):
    """the module loaded from the reference's state and initialised on the device from the reference's input; the
    reference's reversed blocks and Planar are composed torch on the device.  In float64: output, d/dx and every parameter
    gradient against the reference's stored float64 run, bound as in tests/test_mssw_cpu.py (the deviation of the
    reference's float32 run from it, floor 1e-9: its float64 run rounds every normalising factor to float32).  In float32:
    output and d/dx, which are per point, against both stored runs with 4 x the deviation of the one from the other, floor
    1e-6.  The float32 parameter gradients on the device are torch's own sums over the 350 points in another order than
    on the CPU, nothing of this package computes them, and one sample of a float32 error on a cancelling sum bounds
    nothing (measured: 3.3e-6 on a Planar bias against a sample of 0.7e-6): they are printed, and held to the reference
    on the CPU, where they come out bit for bit."""
    case, var = variant
    x, cot = g21_tensor("a.x").to(DEV), g21_tensor("a.cot")
    stored = {d: dict([("value", g21_tensor(f"a.{case}.{var}.{d}.out_train")), ("d/dx", g21_tensor(f"a.{case}.{var}.{d}.grad_x"))]
                      + list(g21_grads(case, var, d).items())) for d in ("f32", "f64")}
    missed = []
    for dname, dtype in (("f64", torch.float64), ("f32", torch.float32)):
        phi = g21_module(shw, case, var, dname).to(DEV)
        phi(x.to(dtype))
        got = module_results(phi, x.to(dtype), cot)
        assert list(got) == list(stored[dname]) and got["value"].dtype == dtype
        for name, g in got.items():
            gap = max_dev(stored["f32"][name], stored["f64"][name])
            bound = max(gap, 1e-9) if dname == "f64" else max(4 * gap, 1e-6)
            to32, to64 = max_dev(g, stored["f32"][name]), max_dev(g, stored["f64"][name])
            print(f"fixture (a) {case} {var} {dname} {name}: gpu to the reference's float32 {to32:.2e} float64 {to64:.2e} "
                  f"bound {bound:.2e}")
            held = dname == "f64" or name in ("value", "d/dx")
            if not torch.isfinite(g).all() or (held and (to64 > bound or (dname == "f32" and to32 > bound))):
                missed.append((dname, name, to32, to64, bound))
    assert not missed, missed


def forward_module(shw, n_flow_layer=2):
    """fixture (a)'s perturbed parameters with the blocks applied forward (the fused direction), initialised on a.x"""
    phi = g21_module(shw, "res2" if n_flow_layer == 2 else "res3", "pert", reverse=False).to(DEV)
    phi(g21_tensor("a.x").to(DEV))
    return phi


@pytest.mark.parametrize("n_flow_layer", [2, 3])
def test_the_forward_module_takes_the_fused_path_after_its_initialising_call(shw, n_flow_layer):
    x, cot = g21_tensor("a.x"), g21_tensor("a.cot")
    phi = g21_module(shw, "res2" if n_flow_layer == 2 else "res3", "pert", reverse=False).to(DEV)
    cot = masked_cotangent(x, torch.cat([p.detach().reshape(-1).cpu() for p in phi.net.parameters()]), cot)
    calls = []
    real = shw.mssw.residual_sphere_map
    shw.mssw.residual_sphere_map = lambda *a: calls.append(1) or real(*a)
    try:
        phi(x.to(DEV))                                               # initialises: composed, layer by layer
        assert calls == [] and phi.is_initialised()
        got = module_results(phi, x.to(DEV), cot)
        assert calls == [1]
    finally:
        shw.mssw.residual_sphere_map = real
    # against float64 on the same float32 parameters, per parameter, under the rule
    ref = {}
    for dtype in (torch.float64, torch.float32):
        twin = g21_module(shw, "res2" if n_flow_layer == 2 else "res3", "pert", reverse=False)
        twin.load_state_dict({k: v.cpu() for k, v in phi.state_dict().items()}, strict=True)
        twin = twin.to(dtype)
        ref[dtype] = module_results(twin, x.to(dtype), cot)
    missed = []
    for name, g in got.items():
        worst, bound = max_dev(g, ref[torch.float64][name]), bound_of(ref[torch.float32][name], ref[torch.float64][name])
        print(f"forward module F={n_flow_layer} {name}: gpu {worst:.2e} bound {bound:.2e}")
        if not torch.isfinite(g).all() or worst > bound:
            missed.append((name, worst, bound))
    assert not missed, missed


def test_fused_off_float64_non_contiguous_input_and_the_refusals(shw):
    phi = forward_module(shw)
    x = torch.randn(3, 70, 3, device=DEV, generator=torch.Generator(DEV).manual_seed(1))
    params, affine = phi.packed_params().detach(), phi.packed_affine().detach()
    with torch.no_grad():                                           # fused on: the kernels' bits; off: the composed path's
        y = phi(x)
        assert torch.equal(y, shw.residual_sphere_map(x, params, affine, 2))
        phi.fused = False
        assert torch.equal(phi(x), shw.residual_sphere_map_composed(x, params, affine, 2))
        phi.fused = True
        got = phi.double()(x.double())
        assert got.dtype == torch.float64 and max_dev(y, got) <= 1e-5
        phi = phi.float()
    # a non-contiguous input
    wide = torch.zeros(3, 140, 3, device=DEV)
    wide[:, ::2] = x
    assert not wide[:, ::2].is_contiguous()
    cot = torch.randn(3, 70, 3, device=DEV, generator=torch.Generator(DEV).manual_seed(2))
    ref = fused(shw, x, params, affine, cot, 2)
    leaf, pd, ad = (t.detach().clone().requires_grad_() for t in (wide, params, affine))
    yv = shw.residual_sphere_map(leaf[:, ::2], pd, ad, 2)
    (yv * cot).sum().backward()
    assert torch.equal(yv.detach(), ref[0]) and torch.equal(pd.grad, ref[2]) and torch.equal(ad.grad, ref[3])
    assert torch.equal(leaf.grad[:, ::2], ref[1]) and not leaf.grad[:, 1::2].any()
    # another N, and what the op cannot take
    with pytest.raises(ValueError, match=r"70 points.*64 points"):
        phi(torch.randn(3, 64, 3, device=DEV))
    with pytest.raises(ValueError, match="170"):
        shw.residual_sphere_map(x, params[:-1], affine, 2)
    with pytest.raises(ValueError, match=r"\(2, 70, 4\)"):
        shw.residual_sphere_map(x, params, affine[:, :69], 2)
    with pytest.raises(ValueError, match="flows"):
        shw.residual_sphere_map(x, torch.zeros(param_count(9), device=DEV), torch.zeros(9, 70, 4, device=DEV), 9)
    with pytest.raises(ValueError):
        shw.residual_sphere_map(x[0], params, affine, 2)
    with pytest.raises(TypeError):
        shw.residual_sphere_map(x.double(), params, affine, 2)
    with pytest.raises(TypeError):
        shw.residual_sphere_map(x, params, affine.double(), 2)
    with pytest.raises(RuntimeError, match="needs device tensors"):
        shw.residual_sphere_map(x, params.cpu(), affine, 2)
    empty = shw.residual_sphere_map(x[:0].requires_grad_(), params.clone().requires_grad_(), affine, 2)
    assert empty.shape == (0, 70, 3)


# ------------------------------------------------------------------------------------------------ 7
def run_wrapper(shw, mode, reverse=True, fused_flag=True, subset_map=True, replay=None, adam=True):
    """the wrapper on the device on fixture (b)'s inputs: phi from the fixture's state, initialised on b.first as there,
    the reference's Adam, SSW = this package's sliced_cost on the fixture's frames"""
    B, N, L, iters, mini = (int(v) for v in g21_tensor("b.config"))
    U = g21_tensor("b.U").to(DEV)
    first, second = g21_tensor("b.first").to(DEV), g21_tensor("b.second").to(DEV)
    np.random.seed(int(g21_tensor("b.seed")))
    phi = g21_wrapper_module(shw, reverse=reverse).to(DEV)
    phi.fused = fused_flag
    phi(first)
    if adam:
        opt = torch.optim.Adam(phi.parameters(), lr=float(g21_tensor("b.lr")), betas=tuple(float(b) for b in g21_tensor("b.betas")))
    else:
        opt = torch.optim.SGD(phi.parameters(), lr=1e-4)
    ssw = lambda a, b, num_projections, device, p=2: shw.sliced_cost(a, b, U, p=p)              # noqa: E731
    crit = shw.max_spherical_wassersten_distance_Residual(L, phi, opt, SSW=ssw, p=2, max_iter=iters,
                                                          psi_minibatch_size=mini, device=DEV)
    crit.subset_map = subset_map
    trace, drawn, choice = [], [], np.random.choice
    crit.on_inner_value = trace.append

    def recording_choice(*args, **kwargs):
        drawn.append(choice(*args, **kwargs) if replay is None else np.array(replay[len(drawn)]))
        return drawn[-1]

    a, b = first.clone().requires_grad_(), second.clone().requires_grad_()
    np.random.choice = recording_choice
    try:
        val, fa, fb = crit(a, b, train_or_test=mode)
    finally:
        np.random.choice = choice
    opt.zero_grad()
    val.sum().backward()
    return dict(val=val.detach(), trace=np.array(trace), params=flat_parameters(phi), fa=fa.detach(), fb=fb.detach(),
                ga=a.grad, gb=b.grad, indices=np.array(drawn, dtype=np.int64).reshape(-1, mini))


def as_stored(run):
    num = lambda t: t.detach().cpu().double().numpy()                                            # noqa: E731
    return dict(ssw=num(run["val"]).reshape(-1), trace=run["trace"], params=num(run["params"]), phi_first=num(run["fa"]),
                phi_second=num(run["fb"]), g_first=num(run["ga"]), g_second=num(run["gb"]))


def figures_of(run, want):
    return fixture_b_figures(run["val"], run["trace"], run["params"], run["fa"], run["fb"], run["ga"], run["gb"], want)


@pytest.mark.parametrize("mode", ["train", "test"])
def test_fixture_b_wrapper_against_the_real_wrapper(shw, mode):
    """the reference's module (reversed blocks, composed on the device), the stored minibatches, the HIP sliced loss:
    against what the REAL wrapper did with the REAL encoder and sliced_cost, in float32 and in float64"""
    run = run_wrapper(shw, mode, replay=g21_run("f32", mode)["indices"])
    tolerance, gaps = fixture_b_tolerances(mode)
    missed = []
    for against in ("f32", "f64"):
        fig = figures_of(run, g21_run(against, mode))
        print(f"fixture (b) {mode} against {against}:", {k: f"{v:.1e}" for k, v in fig.items()},
              "tolerance", {k: f"{v:.1e}" for k, v in tolerance.items()})
        missed += [(against, k, v, tolerance[k]) for k, v in fig.items() if not v <= tolerance[k]]
    assert not missed, missed


@pytest.mark.parametrize("mode", ["train", "test"])
def test_the_wrapper_with_the_fused_module_against_the_composed_one(shw, mode):
    """forward blocks: phi fused against phi composed (fused = False), the subset map on against off -- the same
    minibatches; returned value, trace, parameters, maps and input gradients under the fixture-(b) tolerances.  The ascent
    steps are plain gradient steps (SGD, lr 1e-4), not Adam's: Adam's first steps are lr g / (|g| + 1e-8), which turns a
    rounding-level difference in a small gradient entry into a step of order lr, and this phi carries a parameter
    difference into the maps multiplied by the product of its 1 / std scales -- measured with Adam, composed path, subset
    map against full map: parameters 1.4e-4, maps 4.4e-2.  With gradient steps a difference in the gradients stays one."""
    base = run_wrapper(shw, mode, reverse=False, fused_flag=False, subset_map=False, adam=False)
    tolerance, _ = fixture_b_tolerances(mode)
    missed = []
    for label, kwargs in (("fused, full map", dict(fused_flag=True, subset_map=False)),
                          ("fused, subset map", dict(fused_flag=True, subset_map=True)),
                          ("composed, subset map", dict(fused_flag=False, subset_map=True))):
        run = run_wrapper(shw, mode, reverse=False, adam=False, **kwargs)
        assert np.array_equal(run["indices"], base["indices"])
        fig = figures_of(run, as_stored(base))
        print(f"wrapper {mode} {label} against composed, full map:", {k: f"{v:.1e}" for k, v in fig.items()})
        missed += [(label, k, v, tolerance[k]) for k, v in fig.items() if not v <= tolerance[k]]
    assert not missed, missed
