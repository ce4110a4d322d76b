"""GPU checks (`-m gpu`, MI355X) of the exact-W path: csrc/shw_emd.hip through emd.py, against the float64 optimum of
scipy.optimize.linear_sum_assignment on the cases of tests/helpers/emd_cases.py (whose docstring derives every bound
used here; tests/test_emd_cpu.py asserts, without a GPU, what these tests rely on from their inputs).

Every case runs as a batch of two pairs, (x, y) and (y, x): both costs are symmetric, so the second pair has the same
optimum and, in the permuted cases, the permutation itself as its one optimal assignment."""
import functools

import numpy as np
import pytest
import torch

from helpers import emd_cases as cases

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
    """the kernel's outputs for the two pairs of a case, as numpy (computed once per session)"""
    import shw_amd
    cloud, n, kind, p = case
    ref = cases.reference(case)
    x = torch.from_numpy(np.stack([ref["x"], ref["y"]])).cuda()
    y = torch.from_numpy(np.stack([ref["y"], ref["x"]])).cuda()
    cost, assign, rounds = shw_amd.emd_pair_costs(x, y, p=p, cost=kind, return_assignment=True)
    torch.cuda.synchronize()
    return cost.cpu().numpy(), assign.cpu().numpy().astype(np.int64), rounds.cpu().numpy()


def pairs_of(case):
    ref = cases.reference(case)
    return [(ref["x"], ref["y"]), (ref["y"], ref["x"])]


@pytest.mark.parametrize("case", cases.CASES, ids=IDS)
def test_assignment_is_a_permutation_within_the_bound_of_the_optimum(shw, case):
    """Per pair: `assign` is a permutation; no NaN; the round count is under the cap; the float64 mean cost along
    `assign`, recomputed on the host, is within K 2^-25 + max(16 g, 4 * 2^-24 K) of scipy's optimum (g: the gap of a
    float32 NumPy evaluation of the same assignment to float64); the returned float32 `cost` equals that host mean to
    float32 rounding (emd_cases.cost_bound_along)."""
    cloud, n, kind, p = case
    ref = cases.reference(case)
    cost, assign, rounds = kernel_run(case)
    assert cost.dtype == np.float32 and cost.shape == (2,) and assign.shape == (2, n) and rounds.shape == (2,)
    for b, (x, y) in enumerate(pairs_of(case)):
        assert np.array_equal(np.sort(assign[b]), np.arange(n)), f"pair {b}: not a permutation"
        assert np.isfinite(cost[b])
        assert 0 <= rounds[b] < cases.round_cap(n)
        if ref["K"] > 0:
            assert rounds[b] >= 1
        host = cases.mean_along(x, y, kind, p, assign[b])
        g = cases.eval_gap(x, y, kind, p, assign[b])
        gap, allowed = host - ref["opt"], cases.value_bound(ref["K"], g)
        cgap, callowed = abs(float(cost[b]) - host), cases.cost_bound_along(x, y, kind, p, assign[b])
        print(f"EMD {cases.case_id(case)} pair {b}: K {ref['K']:g} optimum {ref['opt']:.9e} along assign {host:.9e} gap "
              f"{gap:.3e} allowed {allowed:.3e} (g {g:.2e}); cost {cost[b]:.9e} off host {cgap:.2e} allowed "
              f"{callowed:.2e}; rounds {rounds[b]} ({rounds[b] / n:.1f} n)")
        assert -allowed <= gap <= allowed
        assert cgap <= callowed


@pytest.mark.parametrize("case", [c for c in cases.CASES if c[0] == "permuted"],
                         ids=[cases.case_id(c) for c in cases.CASES if c[0] == "permuted"])
def test_permuted_cloud_costs_zero_and_returns_the_inverse_permutation(shw, case):
    ref = cases.reference(case)
    cost, assign, _ = kernel_run(case)
    inverse = ref["extra"]["inverse"]
    assert cost[0] == 0.0 and cost[1] == 0.0
    assert np.array_equal(assign[0], inverse)
    assert np.array_equal(assign[1], np.argsort(inverse))        # (y, x): the permutation itself


@pytest.mark.parametrize("case", [c for c in cases.CASES if c[0] == "zeros"],
                         ids=[cases.case_id(c) for c in cases.CASES if c[0] == "zeros"])
def test_all_zero_clouds(shw, case):
    """lp: every cost is 0, K = 0, the identity comes back without a round.  Angle cost: every cost is (pi / 2)^p, any
    permutation is optimal, and the round count is the largest of all cases (every target ties) -- still under the cap."""
    cloud, n, kind, p = case
    cost, assign, rounds = kernel_run(case)
    assert np.all(np.isfinite(cost)) and np.all(rounds >= 0) and np.all(rounds < cases.round_cap(n))
    if kind == "lp":
        assert np.all(cost == 0.0) and np.all(rounds == 0)
        assert np.array_equal(assign, np.tile(np.arange(n), (2, 1)))
    else:
        assert np.allclose(cost, (np.pi / 2) ** p, rtol=1e-6, atol=0)


def test_results_are_bit_identical_from_run_to_run(shw):
    case = ("clusters", 512, "lp", 2.0)
    ref = cases.reference(case)
    x = torch.from_numpy(np.stack([ref["x"], ref["y"]])).cuda()
    y = torch.from_numpy(np.stack([ref["y"], ref["x"]])).cuda()
    first = kernel_run(case)
    cost, assign, rounds = shw.emd_pair_costs(x, y, p=2.0, cost="lp", return_assignment=True)
    assert np.array_equal(cost.cpu().numpy(), first[0])
    assert np.array_equal(assign.cpu().numpy(), first[1])
    assert np.array_equal(rounds.cpu().numpy(), first[2])


@pytest.mark.parametrize("n,kind,p", cases.GRAD_CASES, ids=[f"{n}-{k}-p{p:g}" for n, k, p in cases.GRAD_CASES])
def test_gradients_against_float64_autograd_along_the_kernels_assignment(shw, n, kind, p):
    """Gradients of (cost * [1, -0.5]).sum() against float64 torch autograd of mean_i C(x_i, y_sigma(i)) along the kernel's
    own sigma, within 16 x the gap of the float32 torch evaluation of that same expression (floor 8 * 2^-24 where the
    two torch runs agree exactly; ceiling 1e-4, as the Chamfer gradient test), in units of the largest entry; and bit
    for bit the same on a second run."""
    x, y = cases.grad_inputs(n)
    w = torch.tensor(cases.GRAD_W, device="cuda")
    runs = []
    for _ in range(2):
        xd, yd = torch.from_numpy(x).cuda().requires_grad_(True), torch.from_numpy(y).cuda().requires_grad_(True)
        cost, assign, _ = shw.emd_pair_costs(xd, yd, p=p, cost=kind, return_assignment=True)
        (cost * w).sum().backward()
        runs.append((cost.detach().cpu().numpy(), assign.cpu().numpy(), xd.grad.cpu().numpy(), yd.grad.cpu().numpy()))
    for a, b in zip(*runs):
        assert np.array_equal(a, b)
    cost, assign, gx, gy = runs[0]
    assert np.all(np.isfinite(cost))
    want = cases.torch_grads(x, y, assign, kind, p, torch.float64)
    f32 = cases.torch_grads(x, y, assign, kind, p, torch.float32)
    for name, got, ref64, ref32 in (("gx", gx, want[0], f32[0]), ("gy", gy, want[1], f32[1])):
        g = cases.of_largest(ref32, ref64)
        gap = cases.of_largest(got, ref64)
        print(f"GAP emd {kind} p={p:g} n={n} {name}: kernel {gap:.3e} torch-f32 {g:.3e} allowed {cases.grad_bound(g):.3e}")
        assert np.abs(ref64).max() > 0
        assert gap < cases.grad_bound(g), f"{name}: kernel gap {gap:.3e}, float32 torch gap {g:.3e}"


@pytest.mark.parametrize("name,kind", [("Cos_disimilarity_W", "lp"), ("Geodesic_distance_W", "geodesic")])
@pytest.mark.parametrize("p", [1, 2])
def test_modules_apply_the_references_reduction(shw, name, kind, p):
    """(B,n,3): batch mean of cost_b^(1/p); (n,3): cost^(1/p) -- computed here from emd_pair_costs"""
    ref = cases.reference(("registration", 257, "lp", 2.0))
    x = torch.from_numpy(np.stack([ref["x"], ref["y"], ref["x"]])).cuda()
    y = torch.from_numpy(np.stack([ref["y"], ref["x"], ref["x"][::-1].copy()])).cuda()
    module = getattr(shw, name)("cuda", p=p)
    pair = shw.emd_pair_costs(x, y, p=p, cost=kind)
    torch.testing.assert_close(module(x, y), pair.pow(1.0 / p).mean(), rtol=1e-6, atol=0)
    single = module(x[0], y[0])
    assert single.dim() == 0
    torch.testing.assert_close(single, pair[0].pow(1.0 / p), rtol=1e-6, atol=0)


def test_notebook_functions_equal_the_single_pair_modules(shw):
    ref = cases.reference(("cube", 1200, "lp", 2.0))
    x, y = torch.from_numpy(ref["x"].copy()).cuda(), torch.from_numpy(ref["y"].copy()).cuda()
    assert torch.equal(shw.wasserstein_distance(x, y, "cuda", p=2), shw.Cos_disimilarity_W("cuda", p=2)(x, y))
    assert torch.equal(shw.wasserstein_distance_geo(x, y, "cuda", p=2), shw.Geodesic_distance_W("cuda", p=2)(x, y))
    assert torch.equal(shw.wasserstein_distance(x[None], y[None], "cuda"), shw.wasserstein_distance(x, y, "cuda"))


def test_module_gradient_flows_through_the_root(shw):
    """loss = mean_b cost_b^(1/2): d loss / dx = (1 / (2 B sqrt(cost_b))) d cost_b / dx, the root taken by torch.pow"""
    x, y = cases.grad_inputs(65)
    xd = torch.from_numpy(x).cuda().requires_grad_(True)
    yd = torch.from_numpy(y).cuda()
    shw.Cos_disimilarity_W("cuda", p=2)(xd, yd).backward()
    xe = torch.from_numpy(x).cuda().requires_grad_(True)
    cost = shw.emd_pair_costs(xe, yd, p=2)
    (cost * (0.5 / (2 * cost.detach().sqrt()))).sum().backward()
    torch.testing.assert_close(xd.grad, xe.grad, rtol=1e-5, atol=0)


def test_phi_max_criterion_trains_with_the_exact_loss_in_the_csw_slot(shw):
    """train_W_COS.py:393-404: max_cos_disimilarity_wassersten_distance(phi, Cos_disimilarity_W(device, p=2), ...)"""
    torch.manual_seed(0)
    ref = cases.reference(("registration", 257, "lp", 2.0))
    x = torch.from_numpy(np.stack([ref["x"][:64], ref["x"][64:128]])).cuda().requires_grad_(True)
    y = torch.from_numpy(np.stack([ref["y"][:64], ref["y"][64:128]])).cuda()
    phi = torch.nn.Linear(3, 3).cuda()
    with torch.no_grad():
        phi.weight.copy_(torch.eye(3) + 0.01 * torch.randn(3, 3))
        phi.bias.zero_()
    before = phi.weight.detach().clone()
    phi_op = torch.optim.SGD(phi.parameters(), lr=0.01)
    criteria = shw.max_cos_disimilarity_wassersten_distance(phi, shw.Cos_disimilarity_W("cuda", p=2), "cuda", phi_op,
                                                            max_iter=2)
    loss, a, b = criteria(y, x, train_or_test="train")
    assert loss.dim() == 0 and torch.isfinite(loss) and loss.item() > 0
    assert a.shape == y.shape and b.shape == x.shape
    assert not torch.equal(phi.weight.detach(), before)            # the inner ascent moved phi
    loss.backward()
    assert x.grad is not None and torch.isfinite(x.grad).all() and x.grad.abs().max() > 0
