"""GPU checks (`-m gpu`, MI355X) of the exact-W path for clouds of different sizes: csrc/shw_emd_units.hip through
emd.transport_pair_costs and once through the C ABI, against the float64 optimum of scipy.optimize.linear_sum_assignment
on the expanded unit x slot matrix, on the cases of tests/helpers/emd_units_cases.py.  Every bound is one of
tests/helpers/emd_cases.py (its docstring derives them); tests/test_emd_units_cpu.py asserts, without a GPU, what these
tests rely on from their inputs."""
import functools

import numpy as np
import pytest
import torch

from helpers import emd_cases
from helpers import emd_units_cases as cases

pytestmark = pytest.mark.gpu
IDS = [cases.case_id(c) for c in cases.CASES]


@pytest.fixture(scope="module")
def shw():
    import shw_amd
    assert torch.cuda.is_available()
    shw_amd._lib.load()
    return shw_amd


@functools.lru_cache(maxsize=None)
def kernel_run(case):
    """the kernel's outputs for the one pair of a case, as numpy (computed once per session)"""
    import shw_amd
    cloud, n, m, kind, p = case
    ref = cases.reference(case)
    x, y = torch.from_numpy(ref["x"][None].copy()).cuda(), torch.from_numpy(ref["y"][None].copy()).cuda()
    cost, targets, rounds = shw_amd.transport_pair_costs(x, y, p=p, cost=kind, return_plan=True)
    torch.cuda.synchronize()
    return cost.cpu().numpy(), targets.cpu().numpy().astype(np.int64), rounds.cpu().numpy()


@pytest.mark.parametrize("case", cases.CASES, ids=IDS)
def test_plan_is_feasible_and_within_the_bound_of_the_optimum(shw, case):
    """`targets` names every target exactly kt times; no NaN; the round count is under the cap; the float64 mean over the
    units along `targets`, recomputed on the host, is within K 2^-25 + max(16 g, 4 * 2^-24 K) of scipy's optimum; the
    returned float32 `cost` equals that host mean to float32 rounding (emd_cases.cost_bound_along)."""
    cloud, n, m, kind, p = case
    ref = cases.reference(case)
    U, ks, kt = ref["U"], ref["ks"], ref["kt"]
    cost, targets, rounds = kernel_run(case)
    assert cost.dtype == np.float32 and cost.shape == (1,) and targets.shape == (1, U) and rounds.shape == (1,)
    assert cases.feasible(targets[0], m, kt), "not a feasible unit plan"
    assert np.isfinite(cost[0])
    assert 0 <= rounds[0] < emd_cases.round_cap(U)
    if ref["K"] > 0:
        assert rounds[0] >= 1
    x, y = ref["x"], ref["y"]
    host = cases.mean_along(x, y, kind, p, targets[0], ks)
    g = cases.eval_gap(x, y, kind, p, targets[0], ks)
    gap, allowed = host - ref["opt"], emd_cases.value_bound(ref["K"], g)
    cgap, callowed = abs(float(cost[0]) - host), cases.cost_bound_along(x, y, kind, p, targets[0], ks)
    print(f"EMD units {cases.case_id(case)}: U {U} K {ref['K']:g} optimum {ref['opt']:.9e} along targets {host:.9e} gap "
          f"{gap:.3e} allowed {allowed:.3e} (g {g:.2e}); cost {cost[0]:.9e} off host {cgap:.2e} allowed {callowed:.2e}; "
          f"rounds {rounds[0]} ({rounds[0] / U:.1f} U)")
    assert -allowed <= gap <= allowed
    assert cgap <= callowed


@pytest.mark.parametrize("case", cases.CASES, ids=IDS)
def test_c_abi_gives_the_bits_of_the_python_entry(shw, case):
    cloud, n, m, kind, p = case
    ref = cases.reference(case)
    U = ref["U"]
    lib = shw._lib.load()
    assert lib.shw_emd_units_supported(n, m) == U
    x, y = torch.from_numpy(ref["x"][None].copy()).cuda(), torch.from_numpy(ref["y"][None].copy()).cuda()
    ws = torch.empty(lib.shw_emd_units_workspace_bytes(1, n, m) // 4, dtype=torch.int32, device="cuda")
    cost = torch.empty(1, device="cuda")
    targets = torch.empty(1, U, dtype=torch.int32, device="cuda")
    rounds = torch.empty(1, dtype=torch.int32, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    rc = lib.shw_emd_units_forward(x.data_ptr(), y.data_ptr(), 1, n, m, {"lp": 0, "geodesic": 1}[kind], p, ws.data_ptr(),
                                   cost.data_ptr(), targets.data_ptr(), rounds.data_ptr(), stream)
    assert rc == 0
    gx, gy, w = torch.empty_like(x), torch.empty_like(y), torch.ones(1, device="cuda")
    rc = lib.shw_emd_units_backward(x.data_ptr(), y.data_ptr(), ws.data_ptr(), w.data_ptr(), 1, n, m,
                                    {"lp": 0, "geodesic": 1}[kind], p, gx.data_ptr(), gy.data_ptr(), stream)
    assert rc == 0
    torch.cuda.synchronize()
    first = kernel_run(case)
    assert np.array_equal(cost.cpu().numpy(), first[0])
    assert np.array_equal(targets.cpu().numpy(), first[1])
    assert np.array_equal(rounds.cpu().numpy(), first[2])
    # the workspace: the target of each unit, the source of each slot (each source ks times), the flag
    ws = ws.cpu().numpy()
    assert np.array_equal(ws[:U], first[1][0]) and ws[2 * U] == 1
    assert np.array_equal(np.bincount(ws[U:2 * U], minlength=n), np.full(n, ref["ks"]))
    assert np.array_equal(np.sort(ws[U:2 * U].reshape(m, ref["kt"]), axis=1),
                          np.sort((np.argsort(first[1][0], kind="stable") // ref["ks"]).reshape(m, ref["kt"]), axis=1))
    xd, yd = x.clone().requires_grad_(True), y.clone().requires_grad_(True)
    shw.transport_pair_costs(xd, yd, p=p, cost=kind).sum().backward()
    assert torch.equal(xd.grad, gx) and torch.equal(yd.grad, gy)


def test_equal_sizes_return_the_assignment_of_the_equal_size_solver(shw):
    """ks = kt = 1: both kernels run the same integer rule on the same integer costs"""
    case = ("sphere", 65, 65, "lp", 2.0)
    ref = cases.reference(case)
    cost, targets, rounds = kernel_run(case)
    x, y = torch.from_numpy(ref["x"][None].copy()).cuda(), torch.from_numpy(ref["y"][None].copy()).cuda()
    c2, assign, r2 = shw.emd_pair_costs(x, y, p=2.0, cost="lp", return_assignment=True)
    assert np.array_equal(targets, assign.cpu().numpy())
    assert np.array_equal(rounds, r2.cpu().numpy()) and np.array_equal(cost, c2.cpu().numpy())


def test_doubled_target_costs_exactly_zero(shw):
    cost, targets, _ = kernel_run(("doubled", 33, 66, "lp", 2.0))
    assert cost[0] == 0.0
    assert np.array_equal(np.sort(targets[0].reshape(33, 2), axis=1), np.arange(66).reshape(33, 2))


def test_all_zero_clouds(shw):
    """lp: every cost is 0, K = 0, the identity comes back without a round.  Angle cost: every cost is (pi / 2)^p, every
    plan is optimal, and the round count is the largest of all cases (every slot ties) -- still under the cap."""
    cost, targets, rounds = kernel_run(("zeros", 32, 48, "lp", 2.0))
    assert cost[0] == 0.0 and rounds[0] == 0
    assert np.array_equal(targets[0], np.arange(96) // 2)
    cost, targets, rounds = kernel_run(("zeros", 32, 48, "geodesic", 2.0))
    assert 1 <= rounds[0] < emd_cases.round_cap(96)
    assert np.allclose(cost, (np.pi / 2) ** 2, rtol=1e-6, atol=0)


def run_with_grads(shw, x, y, kind, p, w):
    xd, yd = torch.tensor(x).cuda().requires_grad_(True), torch.tensor(y).cuda().requires_grad_(True)
    cost, targets, rounds = shw.transport_pair_costs(xd, yd, p=p, cost=kind, return_plan=True)
    (cost * w).sum().backward()
    return (cost.detach().cpu().numpy(), targets.cpu().numpy(), rounds.cpu().numpy(), xd.grad.cpu().numpy(),
            yd.grad.cpu().numpy())


@pytest.mark.parametrize("n,m,kind,p", cases.GRAD_CASES, ids=[f"{n}x{m}-{k}-p{p:g}" for n, m, k, p in cases.GRAD_CASES])
def test_gradients_against_float64_autograd_along_the_kernels_plan(shw, n, m, kind, p):
    """Gradients of (cost * [1, -0.5]).sum() against float64 torch autograd of (1/U) sum_q C(x[q // ks], y[targets[q]])
    along the kernel's own plan, within emd_cases.grad_bound of the gap of the float32 torch evaluation of that same
    expression, in units of the largest entry; bit for bit the same on a second run; and a row whose units (slots) go to
    different partners receives their sum (which is what the autograd reference computes)."""
    U, ks, kt = cases.units(n, m)
    x, y = cases.grad_inputs(n, m)
    w = torch.tensor(cases.GRAD_W, device="cuda")
    runs = [run_with_grads(shw, x, y, kind, p, w) for _ in range(2)]
    for a, b in zip(*runs):
        assert np.array_equal(a, b)
    cost, targets, _, gx, gy = runs[0]
    assert np.all(np.isfinite(cost))
    for b in range(len(cases.GRAD_W)):
        assert cases.feasible(targets[b], m, kt)
        if ks > 1:      # some source splits its mass over different targets
            per_source = targets[b].reshape(n, ks)
            assert (per_source.max(1) > per_source.min(1)).any()
        if kt > 1:      # some target is fed by different sources
            sources = (np.argsort(targets[b], kind="stable") // ks).reshape(m, kt)
            assert (sources.max(1) > sources.min(1)).any()
    want = cases.torch_grads(x, y, targets, ks, kind, p, torch.float64)
    f32 = cases.torch_grads(x, y, targets, ks, kind, p, torch.float32)
    for name, got, ref64, ref32 in (("gx", gx, want[0], f32[0]), ("gy", gy, want[1], f32[1])):
        g = emd_cases.of_largest(ref32, ref64)
        gap = emd_cases.of_largest(got, ref64)
        print(f"GAP emd units {kind} p={p:g} {n}x{m} {name}: kernel {gap:.3e} torch-f32 {g:.3e} allowed "
              f"{emd_cases.grad_bound(g):.3e}")
        assert np.abs(ref64).max() > 0
        assert gap < emd_cases.grad_bound(g), f"{name}: kernel gap {gap:.3e}, float32 torch gap {g:.3e}"


def test_results_are_bit_identical_from_run_to_run(shw):
    case = ("registration", 128, 512, "lp", 2.0)
    ref = cases.reference(case)
    w = torch.ones(1, device="cuda")
    runs = [run_with_grads(shw, ref["x"][None], ref["y"][None], "lp", 2.0, w) for _ in range(2)]
    for a, b in zip(*runs):
        assert np.array_equal(a, b)
    first = kernel_run(case)
    assert np.array_equal(runs[0][0], first[0]) and np.array_equal(runs[0][1], first[1])


def test_a_batch_equals_its_pairs_bit_for_bit(shw):
    n, m, kind, p = 100, 75, "lp", 3.0
    pairs = [cases.build("sphere", n, m, seed=s) for s in (0, 1)] + [cases.build("registration", n, m, seed=2)]
    x, y = np.stack([a for a, _ in pairs]), np.stack([b for _, b in pairs])
    w = torch.tensor([1.0, -0.5, 2.0], device="cuda")
    batch = run_with_grads(shw, x, y, kind, p, w)
    assert len(set(batch[0].tolist())) == 3
    for b in range(3):
        single = run_with_grads(shw, x[b:b + 1], y[b:b + 1], kind, p, w[b:b + 1])
        for whole, one in zip(batch, single):
            assert np.array_equal(whole[b:b + 1], one)


@pytest.mark.parametrize("name,kind,n,m", [("Cos_disimilarity_W", "lp", 128, 256), ("Geodesic_distance_W", "geodesic", 64, 96)])
def test_modules_send_unequal_sizes_to_the_unit_solver(shw, name, kind, n, m):
    """(B,n,3), (B,m,3): batch mean of cost_b^(1/p); (n,3), (m,3): cost^(1/p); backward() reaches both inputs"""
    pairs = [cases.build("registration", n, m, seed=s) for s in (0, 1)]
    x = torch.from_numpy(np.stack([a for a, _ in pairs])).cuda().requires_grad_(True)
    y = torch.from_numpy(np.stack([b for _, b in pairs])).cuda().requires_grad_(True)
    module = getattr(shw, name)("cuda", 2)
    pair = shw.transport_pair_costs(x, y, p=2, cost=kind)
    loss = module(x, y)
    torch.testing.assert_close(loss, pair.pow(1.0 / 2).mean(), rtol=1e-6, atol=0)
    single = module(x[0], y[0])
    assert single.dim() == 0
    torch.testing.assert_close(single, pair[0].pow(1.0 / 2), rtol=1e-6, atol=0)
    loss.backward()
    for t in (x, y):
        assert t.grad is not None and t.grad.shape == t.shape and torch.isfinite(t.grad).all() and t.grad.abs().max() > 0


def test_notebook_function_takes_one_pair_of_different_sizes(shw):
    ref = cases.reference(("registration", 128, 512, "lp", 2.0))
    x, y = torch.from_numpy(ref["x"].copy()).cuda(), torch.from_numpy(ref["y"].copy()).cuda()
    cost = shw.transport_pair_costs(x[None], y[None], p=2)
    assert torch.equal(shw.wasserstein_distance(x, y, "cuda", p=2), cost[0].pow(0.5))
    assert torch.equal(shw.wasserstein_distance(x[None], y[None], "cuda"), shw.wasserstein_distance(x, y, "cuda"))
    geo = shw.transport_pair_costs(x[None], y[None], p=1, cost="geodesic")
    assert torch.equal(shw.wasserstein_distance_geo(x, y, "cuda", p=1), geo[0])


def test_phi_max_criterion_trains_at_the_runners_shapes(shw):
    """train_RUNNER.py:193-218: 128 source points against 256 target points through
    max_cos_disimilarity_wassersten_distance(phi, Cos_disimilarity_W(device, p=2), ...) (train_W_COS.py:393-404)"""
    torch.manual_seed(0)
    pairs = [cases.build("registration", 128, 256, seed=s) for s in (0, 1)]
    src = torch.from_numpy(np.stack([a for a, _ in pairs])).cuda().requires_grad_(True)
    tgt = torch.from_numpy(np.stack([b for _, b in pairs])).cuda()
    phi = torch.nn.Linear(3, 3).cuda()
    with torch.no_grad():
        phi.weight.copy_(torch.eye(3) + 0.01 * torch.randn(3, 3))
        phi.bias.zero_()
    before = phi.weight.detach().clone()
    phi_op = torch.optim.SGD(phi.parameters(), lr=0.01)
    criteria = shw.max_cos_disimilarity_wassersten_distance(phi, shw.Cos_disimilarity_W("cuda", p=2), "cuda", phi_op,
                                                            max_iter=2)
    loss, a, b = criteria(tgt, src, train_or_test="train")
    assert loss.dim() == 0 and torch.isfinite(loss) and loss.item() > 0
    assert a.shape == tgt.shape and b.shape == src.shape
    assert not torch.equal(phi.weight.detach(), before)
    loss.backward()
    assert src.grad is not None and torch.isfinite(src.grad).all() and src.grad.abs().max() > 0
