"""CPU checks of the Residual-MSSW sphere encoder and wrapper (mssw.py): the modules and the composed path against fixture
G21, which holds what the reference's own mini_batch_Residual_MSSW.py computes (tools/make_golden_mssw.py); the state-dict
contract before and after the data-dependent initialisation; the wrapper's host logic; the C entries' argument handling.

Every test uses shw.mssw, shw.residual_sphere_map[_composed], shw.max_spherical_wassersten_distance_Residual or a
shw_mssw_* entry: without the feature each fails on the missing attribute.

Bounds.  The module in float32 against the reference's stored float32 and float64 runs: per tensor, max |error| / max
|reference entry| at most 4 x the deviation of the reference's own float32 run from its float64 run, floor 1e-6 (the rule of
tests/helpers/mssw_cases.py with the reference's two runs in the place of the composed path's).  In float64 against the
stored float64 run: that deviation itself (not 4 x it), floor 1e-9.  The reference's float64 run is not float64
throughout: its `torch.max(torch.ones(1), sigma / coeff)` promotes to float32, so every normalising factor, two per flow,
is rounded to float32 (1e-8 of a weight, seen here layer by layer); that is a handful of float32 roundings against the
float32 run's dozens per value, so the float64 discrepancy stays under the float32 one.  The wrapper in float32 against
both stored runs: per quantity the larger of 4 x the gap between the fixture's two runs and the tolerances of
tests/test_r2_gpu.py:66-98 (helpers.mssw_cases.fixture_b_tolerances); in float64 against the float64 run: that gap, floor
1e-9.

Measured here.  The module in float32 against the reference's float32 values: 0 on every tensor of every case (the same
torch operations in the same order, the reversed blocks' fixed-point loop included); against its float64 values at most
2.2e-5 (bounds from 1.0e-6 to 1.2e-4); in float64 at most 2.4e-8 (a Swish beta; bounds from 1.8e-7).  The ActNorm
initialisation in float32: equal to the reference's bit for bit.  The wrapper, float32, train / test mode, against the
reference's float32 run: returned value 0 / 1.1e-7, trace 1.2e-7, parameters 9.5e-7 / 0, maps 5.0e-6 / 0, input gradients
1.9e-6 / 7.9e-6 of the largest entry; against its float64 run: 3.8e-7 / 1.7e-7, 3.5e-7, 2.1e-5 / 1.9e-5, 4.4e-5 / 6.6e-6,
7.0e-5 / 4.1e-3 with 0.28 % of the entries over 2e-3 (the fixture's own gaps: the same figures); in float64 at most 1.1e-7
(maps; the float32-rounded factors).  Forward blocks, float64, subset map against full map: at most 2.6e-11.
"""
import re

import numpy as np
import pytest
import torch

from helpers.mssw_cases import (CASES, VARIANTS, bound_of, composed_reference, fixture_b_figures, fixture_b_tolerances,
                                flat_parameters, g21_grads, g21_module, g21_names, g21_run, g21_state, g21_tensor,
                                g21_wrapper_module, max_dev, module_results, param_count, param_set)


@pytest.fixture(scope="module")
def shw():
    import shw_amd
    return shw_amd


def ids(v):
    return "-".join(v) if isinstance(v, tuple) else str(v)


# ------------------------------------------------------------------------------------------------ the state dict
@pytest.mark.parametrize("case", list(CASES))
def test_state_dict_contract_before_and_after_the_first_forward(shw, case):
    flow_name, n_flow_layer = CASES[case]
    ref0, ref1 = g21_state(case, "init", "f32", 0), g21_state(case, "init", "f32", 1)
    torch.manual_seed(0)
    np.random.seed(0)
    phi = shw.mssw.transform_to_sphere(flow_name, n_flow_layer=n_flow_layer)
    own = phi.state_dict()
    assert list(own) == list(ref0)
    assert [n for n, _ in phi.named_parameters()] == g21_names(case, "init", "param_names")
    for name, want in ref0.items():
        assert own[name].shape == want.shape and own[name].dtype == want.dtype, name
        assert torch.equal(own[name], want), name                 # the reference's initialisation from the same seed
    if flow_name == "Residual":
        per_flow = ["geom_p", "lamb", "beta", "weight", "bias", "beta", "weight", "bias", "s", "t"]
        names = [n.rsplit(".", 1)[1] for n, _ in phi.named_parameters()][6:]
        assert names == per_flow * n_flow_layer
        assert list(own)[:12] == [f"net.{m}.{t}" for m in ("conv1", "conv2", "conv3", "net.0", "net.2", "net.4")
                                  for t in ("weight", "bias")]
        assert not phi.is_initialised()
    phi(g21_tensor("a.x"))                                           # initialises every ActNorm from its input
    own = phi.state_dict()
    assert list(own) == list(ref1) and phi.is_initialised()
    for name, want in ref1.items():
        assert own[name].shape == want.shape and own[name].dtype == want.dtype, name
        if name.endswith((".s", ".t")):
            assert want.shape == (1, 70, 2)
            # s = -log(std over five clouds): ill-conditioned where a point index's five values nearly agree, so the bound
            # is the rule's, from the reference's own float32 run against its float64 run
            want64 = g21_state(case, "init", "f64", 1)[name]
            worst, to64, bound = max_dev(own[name], want), max_dev(own[name], want64), bound_of(want, want64)
            print(f"{case} {name}: ActNorm initialisation to the reference's float32 {worst:.2e} float64 {to64:.2e} "
                  f"bound {bound:.2e}")
            assert worst <= bound and to64 <= bound, (name, worst, to64, bound)
        elif name.endswith("data_dep_init_done"):
            assert float(own[name]) == 1.0 == float(want) and own[name].device.type == "cpu"
        elif not name.endswith((".scale", ".last_n_samples", ".last_firmom", ".last_secmom")):
            # (scale is refreshed by every forward; the other three belong to the log-determinant estimator, not computed)
            assert torch.equal(own[name], want), name
    # strict loads of the reference's state, as constructed and after its initialisation
    for which in (0, 1):
        fresh = g21_module(shw, case, "init", "f32", which)
        assert fresh.is_initialised() == (which == 1 or flow_name == "Planar")
        assert all(torch.equal(a, b) for a, b in zip(fresh.state_dict().values(), g21_state(case, "init", "f32", which).values()))


def test_a_snapshot_taken_after_initialisation_loads_into_a_fresh_module(shw):
    x = g21_tensor("a.x")
    phi = g21_module(shw, "res2", "pert")
    want = phi(x)
    snapshot = {k: v.clone() for k, v in phi.state_dict().items()}
    assert snapshot["flows.net.1.s"].shape == (1, 70, 2) and float(snapshot["flows.net.1.data_dep_init_done"]) == 1.0
    fresh = shw.mssw.transform_to_sphere("Residual", n_flow_layer=2)
    assert not fresh.is_initialised() and fresh.flows.net[1].s.shape == (1, 2)
    fresh.load_state_dict(snapshot, strict=True)
    assert fresh.is_initialised() and fresh.flows.net[1].s.shape == (1, 70, 2)
    assert isinstance(fresh.flows.net[1].s, torch.nn.Parameter) and fresh.flows.net[1].s.requires_grad
    assert torch.equal(fresh(x), want)
    # and back to an uninitialised state: the flag follows the buffer
    fresh.load_state_dict(g21_state("res2", "pert", "f32", 0), strict=True)
    assert not fresh.is_initialised() and fresh.flows.net[1].s.shape == (1, 2)


def test_another_point_count_is_refused_with_both_numbers(shw):
    phi = g21_module(shw, "res2", "init", "f32", 1)
    assert phi(torch.randn(3, 70, 3)).shape == (3, 70, 3)           # any B
    with pytest.raises(ValueError, match=r"70 points.*64 points"):
        phi(torch.randn(5, 64, 3))
    with pytest.raises(ValueError, match=r"\(B, N, 3\)"):
        phi(torch.randn(70, 3))
    with pytest.raises(ValueError, match="Flow name is not valid"):
        shw.mssw.transform_to_sphere("Radial")


# ------------------------------------------------------------------------------------------------ the module's values
@pytest.mark.parametrize("variant", VARIANTS, ids=ids)
def test_fixture_a_module_against_the_reference_in_both_precisions(shw, variant):
    case, var = variant
    x, cot = g21_tensor("a.x"), g21_tensor("a.cot")
    stored = {}
    for dname in ("f32", "f64"):
        g = _g = {k: g21_tensor(f"a.{case}.{var}.{dname}.{k}") for k in ("out_train", "out_eval", "grad_x")}
        assert torch.equal(g["out_train"], _g["out_eval"])          # the reference: train == eval
        stored[dname] = dict([("value", g["out_train"]), ("d/dx", g["grad_x"])] + list(g21_grads(case, var, dname).items()))
    for dname, dtype in (("f32", torch.float32), ("f64", torch.float64)):
        phi = g21_module(shw, case, var, dname)
        phi.train()
        phi(x.to(dtype))                                             # the initialising call
        got = module_results(phi, x.to(dtype), cot)
        assert list(got) == list(stored[dname]) and got["value"].dtype == dtype
        phi.eval()
        with torch.no_grad():
            assert torch.equal(phi(x.to(dtype)), got["value"])       # train == eval here too
        for name, g in got.items():
            to32, to64 = max_dev(g, stored["f32"][name]), max_dev(g, stored["f64"][name])
            gap = max_dev(stored["f32"][name], stored["f64"][name])
            bound = max(4 * gap, 1e-6) if dname == "f32" else max(gap, 1e-9)
            print(f"fixture (a) {case} {var} {dname} {name}: to the reference's float32 {to32:.2e} float64 {to64:.2e} "
                  f"bound {bound:.2e}")
            assert torch.isfinite(g).all() and to64 <= bound and (dname == "f64" or to32 <= bound), (name, to32, to64, bound)


def test_no_random_numbers_are_drawn(shw):
    phi = g21_module(shw, "res3", "pert")
    phi.train()
    torch.manual_seed(3)
    np.random.seed(3)
    before, before_np = torch.get_rng_state(), np.random.get_state()[1].copy()
    phi(g21_tensor("a.x"))
    phi(g21_tensor("a.x")).sum().backward()
    assert torch.equal(torch.get_rng_state(), before) and np.array_equal(np.random.get_state()[1], before_np)


def test_the_module_after_initialisation_is_the_composed_path(shw):
    x, cot = g21_tensor("a.x"), g21_tensor("a.cot")
    phi = g21_module(shw, "res2", "pert", reverse=False)            # forward blocks: the direction the fused op covers
    first = phi(x)                                                   # layer by layer, initialising
    got = module_results(phi, x, cot)
    params, affine = phi.packed_params().detach(), phi.packed_affine().detach()
    assert params.shape == (param_count(2),) and affine.shape == (2, 70, 4)
    y, gx, _, _ = composed_reference(shw, x, params, affine, cot, 2, torch.float32)
    assert torch.equal(got["value"], y) and torch.equal(got["d/dx"], gx)
    assert max_dev(first, y) <= 1e-6 and (y.norm(dim=-1) - 1).abs().max() < 1e-6
    # an edited encoder runs layer by layer
    phi.net.conv2 = torch.nn.Conv1d(8, 8, 1)
    assert phi._pairs() is None and (phi(x).norm(dim=-1) - 1).abs().max() < 1e-6
    with pytest.raises(ValueError, match="Residual"):
        g21_module(shw, "planar3").packed_params()
    with pytest.raises(ValueError, match="reverse=False"):
        g21_module(shw, "res2", "pert", which=1).packed_params()    # the reference's direction has no packed form


# ------------------------------------------------------------------------------------------------ the wrapper
def run_wrapper(shw, dtype, mode, subset_map=True, initialise=True, reverse=True, replay=None):
    """`replay`: minibatches to hand out in the place of numpy's (the reference's own log-determinant estimator draws from
    numpy's global generator between its calls of np.random.choice, one geometric sample per residual block and phi call,
    which this package does not: from one seed the two draw different minibatches)"""
    from oracle import ref_mirror
    B, N, L, iters, mini = (int(v) for v in g21_tensor("b.config"))
    U = g21_tensor("b.U").to(dtype)
    first, second = g21_tensor("b.first").to(dtype), g21_tensor("b.second").to(dtype)
    seed = int(g21_tensor("b.seed"))
    torch.manual_seed(seed)
    np.random.seed(seed)
    phi = g21_wrapper_module(shw, dtype, reverse)
    if initialise:
        phi(first)
    opt = torch.optim.Adam(phi.parameters(), lr=float(g21_tensor("b.lr")), betas=tuple(float(b) for b in g21_tensor("b.betas")))
    ssw = lambda a, b, num_projections, device, p=2: ref_mirror.sliced_cost(a, b, U, p=p)       # noqa: E731
    crit = shw.max_spherical_wassersten_distance_Residual(L, phi, opt, SSW=ssw, p=2, max_iter=iters, psi_minibatch_size=mini,
                                                          device="cpu")
    crit.subset_map = subset_map
    trace, drawn, choice = [], [], np.random.choice
    crit.on_inner_value = trace.append

    def recording_choice(*args, **kwargs):
        assert args == (B,) and kwargs == dict(size=mini, replace=False)
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
                ga=a.grad, gb=b.grad, indices=np.array(drawn, dtype=np.int64).reshape(-1, mini), phi=phi)


def figures_of(run, want):
    return fixture_b_figures(run["val"], run["trace"], run["params"], run["fa"], run["fb"], run["ga"], run["gb"], want)


@pytest.mark.parametrize("dname", ["f32", "f64"])
@pytest.mark.parametrize("mode", ["train", "test"])
def test_fixture_b_wrapper_host_logic_with_the_cpu_oracle_as_ssw(shw, mode, dname):
    """The package's wrapper with the CPU module as phi, the reference's Adam and the CPU oracle on the fixture's frames as
    SSW must retrace what the REAL wrapper did with the REAL encoder and sliced_cost (:413-451): the minibatches drawn,
    the values printed, the parameters after the ascent, the returned value, the maps and both input gradients."""
    assert [int(v) for v in g21_tensor("b.config")] == [6, 40, 16, 3, 2]
    want = g21_run(dname, mode)
    run = run_wrapper(shw, torch.float32 if dname == "f32" else torch.float64, mode, replay=want["indices"])
    assert np.array_equal(run["indices"], want["indices"]) and len(run["indices"]) == (3 if mode == "train" else 0)
    tolerance, gaps = fixture_b_tolerances(mode)
    for against in (("f32", "f64") if dname == "f32" else ("f64",)):
        fig = figures_of(run, g21_run(against, mode))
        print(f"fixture (b) {dname} {mode} against {against}:", {k: f"{v:.1e}" for k, v in fig.items()},
              "fixture gaps", {k: f"{v:.1e}" for k, v in gaps.items()})
        for name, figure in fig.items():
            assert figure <= (tolerance[name] if dname == "f32" else max(gaps[name], 1e-9)), (against, name, figure)


def test_the_minibatches_are_numpys_global_draws_one_call_per_iteration(shw):
    """nothing else in the wrapper or in phi consumes numpy's global generator: the minibatches are the first three
    np.random.choice(6, 2, replace=False) after the seed, and the generator is left where those three calls leave it"""
    run = run_wrapper(shw, torch.float32, "train")
    np.random.seed(int(g21_tensor("b.seed")))
    want = np.array([np.random.choice(6, size=2, replace=False) for _ in range(3)])
    assert np.array_equal(run["indices"], want)
    after = np.random.get_state()[1].copy()
    run_wrapper(shw, torch.float32, "train")
    assert np.array_equal(np.random.get_state()[1], after)


def test_the_subset_map_equals_the_full_map(shw):
    """forward blocks (phi acts per cloud), float64, so that the order of summation is all that differs: the inner loop on
    the selected clouds only against the full maps -- the same minibatches, values, parameters, maps and gradients to
    1e-9.  With the reference's reversed blocks the stopping rule is global and the wrapper maps the full batch."""
    sub, full = (run_wrapper(shw, torch.float64, "train", flag, reverse=False) for flag in (True, False))
    calls = []
    phi = g21_wrapper_module(shw, torch.float64)
    phi(g21_tensor("b.first").double())
    phi.register_forward_hook(lambda m, inp, out: calls.append(inp[0].shape[0]))
    crit = shw.max_spherical_wassersten_distance_Residual(16, phi, torch.optim.SGD(phi.parameters(), lr=0.0),
                                                          SSW=lambda a, b, L, device, p=2: (a - b).pow(2).sum(),
                                                          max_iter=1, psi_minibatch_size=2, device="cpu")
    crit(g21_tensor("b.first").double(), g21_tensor("b.second").double())
    assert not phi.acts_per_cloud() and calls == [6, 6, 6, 6]
    assert sub["phi"].acts_per_cloud()
    assert np.array_equal(sub["indices"], full["indices"]) and not torch.equal(sub["params"], flat_parameters(g21_wrapper_module(shw)))
    want = dict(ssw=full["val"].numpy().reshape(-1), trace=full["trace"], params=full["params"].numpy(),
                phi_first=full["fa"].numpy(), phi_second=full["fb"].numpy(), g_first=full["ga"].numpy(), g_second=full["gb"].numpy())
    fig = figures_of(sub, want)
    print("subset map against full map:", {k: f"{v:.1e}" for k, v in fig.items()})
    assert all(v <= 1e-9 for v in fig.values()), fig


def test_the_initialising_call_maps_the_full_batch(shw):
    """phi not yet initialised when the wrapper is called: the first inner iteration maps the full first batch, so the
    ActNorm layers see all B clouds as in the reference; the later iterations take the subset"""
    run = run_wrapper(shw, torch.float64, "train", True, initialise=False, reverse=False)
    ready = run_wrapper(shw, torch.float64, "train", True, initialise=True, reverse=False)
    assert run["phi"].is_initialised() and np.array_equal(run["indices"], ready["indices"])
    fig = figures_of(run, dict(ssw=ready["val"].numpy().reshape(-1), trace=ready["trace"], params=ready["params"].numpy(),
                               phi_first=ready["fa"].numpy(), phi_second=ready["fb"].numpy(), g_first=ready["ga"].numpy(),
                               g_second=ready["gb"].numpy()))
    assert all(v <= 1e-9 for v in fig.values()), fig
    with pytest.raises(ValueError, match="train_or_test"):
        shw.max_spherical_wassersten_distance_Residual(4, run["phi"], None)(torch.zeros(2, 40, 3), torch.zeros(2, 40, 3), "eval")


# ------------------------------------------------------------------------------------------------ the C entries, the op
def test_c_entries_without_a_device(shw):
    lib = shw._lib.load()
    header = open(shw._lib.os.path.join(shw._lib._HERE, "..", "include", "shw.h")).read()
    for name in ("shw_mssw_supported", "shw_mssw_param_count", "shw_mssw_backward_blocks", "shw_mssw_workspace_bytes",
                 "shw_mssw_forward", "shw_mssw_backward"):
        assert re.search(r"SHW_API\s+\w+\s+%s\s*\(" % name, header), name
        assert name in shw._lib.EXPORTED_SYMBOLS and hasattr(lib, name), name
    assert lib.shw_abi_version() == 3
    assert all(lib.shw_mssw_supported(4, 2, f) == 1 for f in range(1, 9))
    for shape in ((4, 2, 0), (4, 2, 9), (8, 2, 2), (4, 3, 2), (3, 2, 2), (0, 0, 0), (4, 2, -1)):
        assert lib.shw_mssw_supported(*shape) == 0, shape
    assert [lib.shw_mssw_param_count(f) for f in (0, 1, 2, 8, 9)] == [0, 146, 170, 314, 0]
    assert all(lib.shw_mssw_param_count(f) == param_count(f) for f in range(1, 9))
    cap = lib.shw_mssw_backward_blocks(1 << 40)
    assert cap >= 1
    assert [lib.shw_mssw_backward_blocks(n) for n in (-1, 0, 1, 64, 65, 4099)] == [0, 0, 1, 1, 2, min(65, cap)]
    assert lib.shw_mssw_backward_blocks(64 * cap) == cap == lib.shw_mssw_backward_blocks(64 * cap + 1)
    for B, N, f in ((1, 1, 1), (2, 64, 2), (3, 341, 3), (1, 64 * cap + 1, 8)):
        assert lib.shw_mssw_workspace_bytes(B, N, f) == B * N * f * 16 + lib.shw_mssw_backward_blocks(B * N) * param_count(f) * 4
    for B, N, f in ((0, 5, 2), (5, 0, 2), (-1, 5, 2), (2, 64, 0), (2, 64, 9)):
        assert lib.shw_mssw_workspace_bytes(B, N, f) == 0
    # null or invalid arguments: 1 (hipErrorInvalidValue) before any HIP call; 16 stands for an aligned address
    fwd = lambda x=16, p=16, a=16, B=2, N=64, f=2, y=16: lib.shw_mssw_forward(x, p, a, B, N, f, y, None)      # noqa: E731
    assert fwd(x=None) == 1 and fwd(p=None) == 1 and fwd(a=None) == 1 and fwd(y=None) == 1
    assert fwd(B=-1) == 1 and fwd(N=-1) == 1 and fwd(f=0) == 1 and fwd(f=9) == 1 and fwd(a=8) == 1
    assert fwd(B=0) == 0 and fwd(N=0) == 0
    bwd = lambda x=16, p=16, a=16, g=16, B=2, N=64, f=2, gx=16, gp=16, ga=16, w=16: lib.shw_mssw_backward(     # noqa: E731
        x, p, a, g, B, N, f, gx, gp, ga, w, None)
    assert bwd(x=None) == 1 and bwd(p=None) == 1 and bwd(a=None) == 1 and bwd(g=None) == 1
    assert bwd(B=-1) == 1 and bwd(N=-1) == 1 and bwd(f=0) == 1 and bwd(f=9) == 1
    assert bwd(a=8) == 1 and bwd(ga=8) == 1 and bwd(w=8) == 1                       # not 16-byte aligned
    assert bwd(w=None) == 1 and bwd(gx=None, gp=None, w=None) == 1 and bwd(gx=None, ga=None, w=None) == 1
    assert bwd(gp=None, ga=None, w=None, gx=None) == 0                               # nothing asked for


def test_the_op_refuses_what_it_cannot_take(shw):
    params, affine = param_set(shw, "pert", 2, 8)
    x = torch.zeros(2, 8, 3)
    with pytest.raises(RuntimeError, match="needs device tensors"):
        shw.residual_sphere_map(x, params, affine, 2)
    with pytest.raises(TypeError):
        shw.residual_sphere_map(x.numpy(), params, affine, 2)
    with pytest.raises(ValueError, match="170"):
        shw.residual_sphere_map_composed(x, params[:-1], affine, 2)
    with pytest.raises(ValueError, match=r"\(2, 8, 4\)"):
        shw.residual_sphere_map_composed(x, params, affine[:, :7], 2)
    with pytest.raises(ValueError, match=r"\(B, N, 3\)"):
        shw.residual_sphere_map_composed(x[0], params, affine, 2)
    with pytest.raises(ValueError, match=r"\(B, N, 3\)"):
        shw.residual_sphere_map_composed(torch.zeros(2, 8, 4), params, affine, 2)
    assert shw.residual_sphere_map_composed(x, params[:122], affine[:0], 0).shape == (2, 8, 3)   # no flow: the encoder alone
    assert shw.transform_to_sphere_Residual is shw.mssw.transform_to_sphere
    assert shw.Flow_structure is shw.mssw.Flow_structure and shw.ActNorm is shw.mssw.ActNorm
