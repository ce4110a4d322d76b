"""GPU tests of the gradients through the Sinkhorn plan P and cost matrix C (`plan_grad=True`, dense cotangents:
sinkhorn_seed_plan_x_kernel, sinkhorn_seed_y_kernel<true>) and of the fused soft map (`sinkhorn_barycentric_map`:
sinkhorn_map_traj_kernel, sinkhorn_seed_map_x_kernel, sinkhorn_seed_y_kernel<false>), against float64 autograd through
oracle/sinkhorn_mirror.py at the shapes where the tiles go ragged.

Bounds are the rule of tests/helpers/sinkhorn_chamfer_cases.py (max(16 g, floor), g the float32 mirror's own gap to the
float64 run); inputs and cached mirror runs are in tests/helpers/sinkhorn_plan_cases.py, the conditions they rely on are
checked without a GPU in tests/test_sinkhorn_plan_cpu.py.  Every assertion prints (kernel gap) / g; the measured ratios
are in profiles/r16_sinkhorn_plan_gaps.txt."""
import pytest
import torch

from helpers import sinkhorn_chamfer_cases as cases
from helpers import sinkhorn_plan_cases as plan

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def shw():
    import shw_amd
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    shw_amd._lib.load()
    return shw_amd


def within(what, gap, g, k=cases.K):
    r = cases.ratio(gap, g)
    print(f"GAP {what}: kernel {gap:.3e} mirror {g:.3e} ratio {r:.2f}")
    assert gap < cases.bound(g, 1.0, k), f"{what}: kernel gap {gap:.3e} = {r:.1f} x the mirror's own gap {g:.3e} (bound {k})"


def check_grads(what, cost, gx, gy, ref, g, quantities=("cost", "gx", "gy")):
    got = cases.grad_gaps(cost.detach().cpu().numpy(), gx.cpu().numpy(), gy.cpu().numpy(), ref)
    for q in quantities:
        within(f"{what} {q}", got[q], g[q])


def plan_run(shw, x, y, eps, iters, w, WP, WC, use=("cost", "P", "C"), thresh=1e-9, transposed=False):
    """forward with plan_grad=True and backward of L restricted to `use`; returns cost, gx, gy"""
    xd, yd = x.cuda().requires_grad_(True), y.cuda().requires_grad_(True)
    cost, P, C = shw.sinkhorn_pair_costs(xd, yd, eps, iters, thresh=thresh, return_plan=True, plan_grad=True)
    assert P.requires_grad and C.requires_grad and cost.requires_grad
    loss = 0
    if "cost" in use:
        loss = loss + (cost * torch.as_tensor(w, dtype=torch.float32, device="cuda")).sum()
    if "P" in use:
        # transposed: the cotangent of P arrives as a non-contiguous (B, n, m) view of a (B, m, n) tensor
        loss = loss + ((WP.cuda().transpose(1, 2).contiguous() * P.transpose(1, 2)).sum() if transposed else (WP.cuda() * P).sum())
    if "C" in use:
        loss = loss + (WC.cuda() * C).sum()
    loss.backward()
    return cost.detach(), xd.grad, yd.grad


# --------------------------------------------------------------------------------------- 1. dense cotangents
@pytest.mark.parametrize("case", plan.PLAN_CASES, ids=plan.case_id)
def test_plan_and_cost_matrix_gradients_at_tile_edges(shw, case):
    """gx, gy of L = sum w cost + <WP, P> + <WC, C> against the float64 mirror.
    measured (kernel gap / mirror gap): gx 1.0 to 7.0 (7.0 at eps 0.005), gy 1.0 to 5.7; cost 0.3 to 7.6."""
    n, m, eps, iters = case
    x, y, WP, WC, ref, g = plan.plan_case(*case)
    cost, gx, gy = plan_run(shw, x, y, eps, iters, plan.W, WP, WC)
    check_grads(f"plan {n}x{m} eps {eps}", cost, gx, gy, ref, g)


@pytest.mark.parametrize("use,transposed", [(("P",), False), (("C",), False), (("cost", "P", "C"), True)],
                         ids=["only_P", "only_C", "noncontiguous_cotangent"])
def test_plan_gradients_with_unused_outputs_and_a_noncontiguous_cotangent(shw, use, transposed):
    """(257, 513): only P consumed (the cost unused: a null grad_cost), only C consumed (null grad_cost and grad_plan), and a
    cotangent of P that arrives non-contiguous from a loss on P.transpose(1, 2)."""
    case = (257, 513, 0.05, 30)
    x, y, WP, WC, ref, g = plan.plan_case(*case, use=use)
    cost, gx, gy = plan_run(shw, x, y, 0.05, 30, plan.W, WP, WC, use=use, transposed=transposed)
    check_grads(f"plan 257x513 use {'+'.join(use)} transposed {transposed}", cost, gx, gy, ref, g)


# --------------------------------------------------------------------------------------- 2. G17 through the classes
@pytest.mark.parametrize("tag", list(plan.G17))
def test_g17_through_the_classes_with_plan_grad(shw, golden, tag):
    """L2, L1 and the N = 2 class (C = C^N returned, the 1/N root outside the kernel) against the real classes' float64
    gradients; g is the real class's float32-vs-float64 gap stored in the fixture."""
    f = golden("g17_sinkhorn_plan.npz")
    kw = plan.G17[tag]
    if kw["cost_pow"] == 1:
        crit = shw.log_Sinkhorn_Distance_Loss(kw["eps"], kw["max_iter"], type_of_cost_norm=f"L{kw['norm_p']}", plan_grad=True)
    else:
        crit = shw.log_N_Sinkhorn_Distance_Loss(kw["eps"], kw["max_iter"], type_of_cost_norm=f"L{kw['norm_p']}",
                                                type_of_Wasserstein_N=str(kw["cost_pow"]), plan_grad=True)
    xd, yd = torch.from_numpy(f["x"]).cuda().requires_grad_(True), torch.from_numpy(f["y"]).cuda().requires_grad_(True)
    cost, P, C = crit(xd, yd, "cuda")
    w, WP, WC = (torch.from_numpy(f[k]).cuda() for k in ("w", "WP", "WC"))
    ((cost * w).sum() + (WP * P).sum() + (WC * C).sum()).backward()
    ref = {q: f[f"{q}_{tag}_f64"] for q in ("cost", "gx", "gy")}
    check_grads(f"G17 {tag}", cost, xd.grad, yd.grad, ref, {q: float(f[f"gap_{q}_{tag}"]) for q in ("cost", "gx", "gy")})


def test_g17_single_pair_call_carries_the_gradient_through_p0(shw, golden):
    """A 2-D (n, 3), (m, 3) call returns P[0], C[0] of the batched solve: views that carry the gradient."""
    f = golden("g17_sinkhorn_plan.npz")
    crit = shw.log_Sinkhorn_Distance_Loss(0.05, 60, plan_grad=True)
    xd, yd = torch.from_numpy(f["x"][0]).cuda().requires_grad_(True), torch.from_numpy(f["y"][0]).cuda().requires_grad_(True)
    cost, P, C = crit(xd, yd, "cuda")
    assert P.shape == (48, 40) and cost.dim() == 0
    (cost * float(f["w"][0]) + (torch.from_numpy(f["WP"][0]).cuda() * P).sum() + (torch.from_numpy(f["WC"][0]).cuda() * C).sum()).backward()
    # the fixture's pair 0 alone (pairs do not interact, and neither run stops early): g is the gap of its own two runs
    for q, got in (("gx", xd.grad), ("gy", yd.grad)):
        within(f"G17 single pair {q}", cases.of_largest(got.cpu().numpy(), f[f"{q}_L2_f64"][0]),
               cases.of_largest(f[f"{q}_L2_f32"][0], f[f"{q}_L2_f64"][0]))


# --------------------------------------------------------------------------------------- 3. early stop
def test_plan_gradients_after_an_early_stop(shw):
    """cases.STOP_CASES[0]: the stop at sweep 9 of 40.  The seeds read the last EXECUTED slot of the trajectory: gradients
    against the mirror stopped by the same threshold, and bit-identical to a run with max_iter = 9 that cannot stop."""
    x, y, w, thresh, WP, WC, ref, g = plan.stop_plan_case()
    runs = [plan_run(shw, x, y, 0.5, it, w, WP, WC, thresh=th) for it, th in ((40, thresh), (cases.STOP_T, 0.0))]
    check_grads("plan early stop", *runs[0], ref, g)
    for a, b in zip(*runs):
        assert torch.equal(a, b)


# --------------------------------------------------------------------------------------- 4. no sweep
def test_plan_gradients_with_no_sweep(shw):
    """max_iter = 0: duals zero, P = exp(-C / eps), only the seed kernels run."""
    x, y, WP, WC, ref, g = plan.no_sweep_plan_case()
    cost, gx, gy = plan_run(shw, x, y, 0.05, 0, cases.VARIANT_W, WP, WC)
    check_grads("plan no sweep", cost, gx, gy, ref, g)


# --------------------------------------------------------------------------------------- 5. nothing existing moved
def test_plan_grad_leaves_values_and_the_cost_only_gradient_bit_identical(shw):
    case = (257, 513, 0.05, 30)
    x, y, WP, WC = plan.plan_case(*case)[:4]
    wd = torch.tensor(plan.W, device="cuda")
    outs = []
    for flag in (False, True):
        xd, yd = x.cuda().requires_grad_(True), y.cuda().requires_grad_(True)
        cost, P, C = shw.sinkhorn_pair_costs(xd, yd, 0.05, 30, return_plan=True, plan_grad=flag)
        assert P.requires_grad == flag and C.requires_grad == flag
        (cost * wd).sum().backward()                     # only the cost consumed
        outs.append((cost.detach(), P.detach(), C.detach(), xd.grad, yd.grad))
    for a, b in zip(*outs):
        assert torch.equal(a, b)
    runs = [plan_run(shw, x, y, 0.05, 30, plan.W, WP, WC) for _ in range(2)]
    for a, b in zip(*runs):
        assert torch.equal(a, b)


# --------------------------------------------------------------------------------------- 6. the fused map
def map_entry(shw, x, y, eps, iters):
    """the C entry itself: T, r, cost"""
    lib = shw._lib.load()
    B, n, _ = x.shape
    m = y.shape[1]
    xd, yd = x.cuda().contiguous(), y.cuda().contiguous()
    ws = torch.empty(lib.shw_sinkhorn_train_workspace_bytes(B, n, m, iters), dtype=torch.uint8, device="cuda")
    cost, T, r = torch.empty(B, device="cuda"), torch.empty(B, n, 3, device="cuda"), torch.empty(B, n, device="cuda")
    shw._lib.check(lib.shw_sinkhorn_map_forward(xd.data_ptr(), yd.data_ptr(), B, n, m, eps, iters, 2, 1, 1e-9, ws.data_ptr(),
                                                cost.data_ptr(), T.data_ptr(), r.data_ptr(),
                                                torch.cuda.current_stream().cuda_stream), "shw_sinkhorn_map_forward")
    return T, r, cost


@pytest.mark.parametrize("case", plan.PLAN_CASES, ids=plan.case_id)
def test_barycentric_map_and_its_gradients_at_tile_edges(shw, case):
    """T and r against the float64 mirror, T against (P @ y) / P.sum(-1) of the dense path, gx, gy of
    sum ||T - x||^2 + sum w cost against the mirror, and the cost of return_cost=True bit for bit.
    measured (kernel gap / mirror gap): T 0.0 to 1.8 (0.0 to 1.2 against the dense path), r 0.0 to 3.4, gx 2.0 to 9.4,
    gy 1.1 to 9.4 (both 9.4 at 17 x 63)."""
    n, m, eps, iters = case
    x, y, ref, g = plan.map_case(*case)
    tag = f"map {n}x{m} eps {eps}"
    T_e, r_e, cost_e = map_entry(shw, x, y, eps, iters)
    xd, yd = x.cuda().requires_grad_(True), y.cuda().requires_grad_(True)
    T, cost = shw.sinkhorn_barycentric_map(xd, yd, eps, iters, return_cost=True)
    assert T.requires_grad and cost.requires_grad and torch.equal(T.detach(), T_e) and torch.equal(cost.detach(), cost_e)
    (((T - xd) ** 2).sum() + (cost * torch.tensor(plan.W, device="cuda")).sum()).backward()
    got = plan.map_gaps({"T": T.detach().cpu().numpy(), "r": r_e.cpu().numpy(), "cost": cost.detach().cpu().numpy(),
                         "gx": xd.grad.cpu().numpy(), "gy": yd.grad.cpu().numpy()}, ref)
    for q in ("T", "r", "cost", "gx", "gy"):
        within(f"{tag} {q}", got[q], g[q])
    with torch.no_grad():
        cost_p, P, _ = shw.sinkhorn_pair_costs(xd, yd, eps, iters, return_plan=True)
        T_v = shw.sinkhorn_barycentric_map(xd, yd, eps, iters)
    assert torch.equal(cost_p, cost.detach())
    assert torch.equal(T_v, T.detach()) and T_v.grad_fn is None
    dense = (P.double() @ yd.detach().double()) / P.double().sum(-1, keepdim=True)
    within(f"{tag} T vs dense", cases.of_largest(T.detach().cpu().numpy(), dense.cpu().numpy()), g["T"])


def test_barycentric_map_allocates_no_dense_tensor(shw):
    """B = 2, n = m = 1024, 5 iterations: a forward + backward raises the peak of allocated memory by less than one
    (B, n, m) float32 tensor (8 MB; what it needs is the 115 KB trajectory and a few (B, n, 3) tensors: 247 KB measured)."""
    Bm, n = 2, 1024
    g = torch.Generator().manual_seed(1024)
    x, y = cases.unit_cloud(g, Bm, n).cuda().requires_grad_(True), cases.unit_cloud(g, Bm, n).cuda().requires_grad_(True)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    T = shw.sinkhorn_barycentric_map(x, y, 0.05, 5)
    ((T - x) ** 2).sum().backward()
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated() - before
    print(f"peak rise {rise} bytes, one dense tensor {4 * Bm * n * n}")
    assert rise < 4 * Bm * n * n
    assert torch.isfinite(x.grad).all() and torch.isfinite(y.grad).all() and x.grad.abs().max() > 0


# --------------------------------------------------------------------------------------- 7. arguments
def test_plan_grad_arguments(shw):
    x, y = (t.cuda() for t in cases.forward_inputs(9, 7))
    with pytest.raises(ValueError, match="plan_grad"):
        shw.sinkhorn_pair_costs(x.clone().requires_grad_(True), y, 0.05, 5, return_plan=False, plan_grad=True)
    with torch.no_grad():
        cost, P, C = shw.sinkhorn_pair_costs(x.clone().requires_grad_(True), y, 0.05, 5, return_plan=True, plan_grad=True)
    assert cost.grad_fn is None and P.grad_fn is None and C.grad_fn is None
    cost, P, C = shw.sinkhorn_pair_costs(x, y, 0.05, 5, return_plan=True, plan_grad=True)      # no cloud requires grad
    assert cost.grad_fn is None and P.grad_fn is None and not P.requires_grad
    T = shw.sinkhorn_barycentric_map(x, y, 0.05, 5)
    assert T.grad_fn is None and T.shape == (3, 9, 3)
    with pytest.raises(TypeError, match="float32"):
        shw.sinkhorn_barycentric_map(x.half(), y.half(), 0.05, 5)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        shw.sinkhorn_barycentric_map(x.cpu(), y, 0.05, 5)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        shw.sinkhorn_pair_costs(x.cpu(), y, 0.05, 5, return_plan=True, plan_grad=True)
    with pytest.raises(ValueError, match="same B"):
        shw.sinkhorn_barycentric_map(x[:2], y, 0.05, 5)
