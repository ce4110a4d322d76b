"""GPU tests that anchor the two comparison metrics, log-domain Sinkhorn (csrc/shw_sinkhorn.hip, 9 kernels) and Chamfer
(csrc/shw_chamfer.hip, 3 kernels), to float64 at the sizes where their tiles and chunks are ragged.

Sinkhorn bounds are derived, not chosen: tests/helpers/sinkhorn_chamfer_cases.py runs oracle/sinkhorn_mirror.py in float64
(the reference value) and in float32 on the same inputs; the gap g of the two runs is the reference's own rounding noise
for the quantity, and the kernel must lie within max(16 g, 8 * 2^-24 relative) of the float64 run (the reasoning for 16
is in that module's header).  Every assertion message carries (kernel gap) / g.  The conditions these tests rely on
(enough ties, a stop that float32 cannot move by a sweep, ...) are checked without a GPU in
tests/test_sinkhorn_mirror_cpu.py.  Measured ratios: profiles/r09_sinkhorn_chamfer_gaps.txt and the docstrings below."""
import numpy as np
import pytest
import torch

from helpers import sinkhorn_chamfer_cases as cases

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def shw():
    import shw_amd
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    shw_amd._lib.load()
    return shw_amd


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda")


def rel(a, b):
    a = np.asarray(a, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    return float(np.max(np.abs(a - b) / np.maximum(np.abs(b), 1e-30)))


def within(what, gap, g, scale=1.0, k=cases.K):
    """the rule of the module header; prints the figure before it asserts"""
    r = cases.ratio(gap, g, scale)
    print(f"GAP {what}: kernel {gap:.3e} mirror {g:.3e} ratio {r:.2f}")
    assert gap < cases.bound(g, scale, k), f"{what}: kernel gap {gap:.3e} = {r:.1f} x the mirror's own gap {g:.3e} (bound {k})"


def check_grads(what, cost, gx, gy, ref, g, k_of=None):
    got = cases.grad_gaps(cost.detach().cpu().numpy(), gx.cpu().numpy(), gy.cpu().numpy(), ref)
    for q in ("cost", "gx", "gy"):
        within(f"{what} {q}", got[q], g[q], k=(k_of or {}).get(q, cases.K))


# --------------------------------------------------------------------- Sinkhorn forward: duals, plan, marginals (2)
@pytest.mark.parametrize("n,m,eps,iters", cases.FORWARD_CASES)
def test_sinkhorn_plan_and_cost_at_tile_and_chunk_edges(shw, n, m, eps, iters):
    """Candidate counts 1, 7, 9 (a chunk of 8 + 1), 255, 513 (one past the 512 tile), 520 (tile + a full chunk), 1025;
    row counts 1, 257, 513 (one live thread in the last block).  Value-only and training entry paths.  Cost, log P entry
    by entry (that is the duals: log P_ij = (u_i + v_j - C_ij) / eps), column sums against the marginal a v-pass makes
    exact, row sums against float64, all within 16 x the mirror's float32-vs-float64 gap; C to 1e-6; P and C of the two
    entry paths bit-identical.  The last case, eps = 0.005 (exponent scale 288), underflows 90 % of the plan.
    measured (kernel gap / mirror gap; the two paths give the same bits): cost 1.7 to 9.9 (9.9 at 513 x 1025, the
    sequential fmaf over 1025 candidates of the cost kernel), log P 0.85 to 1.22, column sums 0.3 to 4.4 (4.4 at 9 x 7),
    row sums 1.0 to 1.9."""
    x, y, ref, g = cases.forward_case(n, m, eps, iters)
    xd, yd = x.cuda(), y.cuda()
    with torch.no_grad():
        cost_v, P_v, C_v = shw.sinkhorn_pair_costs(xd, yd, eps, iters, return_plan=True)
    cost_t, P_t, C_t = shw.sinkhorn_pair_costs(xd.clone().requires_grad_(True), yd, eps, iters, return_plan=True)
    assert cost_t.requires_grad and not cost_v.requires_grad
    assert torch.equal(P_v, P_t) and torch.equal(C_v, C_t)
    assert torch.equal(cost_v, cost_t.detach())
    assert np.allclose(C_v.cpu().numpy(), ref["C"], rtol=1e-6)
    got = cases.plan_gaps(P_v.cpu().numpy(), cost_v.cpu().numpy(), ref)
    tag = f"forward {n}x{m} eps {eps}"
    within(f"{tag} cost", got["cost"], g["cost"])
    within(f"{tag} logP", got["logP"], g["logP"], ref["logP_scale"])
    within(f"{tag} colsum", got["col"], g["col"])
    within(f"{tag} rowsum", got["row"], g["row"])


# -------------------------------------------------------------------------------- cost variants at a ragged shape (3)
@pytest.mark.parametrize("tag", list(cases.VARIANTS))
def test_sinkhorn_cost_variants_at_a_ragged_shape(shw, tag):
    """(257, 513), through the classes: L1, L3 (the powf branch of pair_cost / pair_cost_grad), L2 with N = 2 and 3, L1
    with N = 2.  Value and both gradients of (cost * [1, -0.7]).sum() against float64 autograd of the mirror.
    measured (kernel gap / mirror gap): cost 0.4 to 3.6, gx 2.4 to 3.9, gy 2.3 to 3.2."""
    x, y, ref, g = cases.variant_case(tag)
    norm_p, cost_pow = cases.VARIANTS[tag]
    if cost_pow == 1:
        crit = shw.log_Sinkhorn_Distance_Loss(0.05, 25, batch_reduction="none", type_of_cost_norm=f"L{norm_p}")
    else:
        crit = shw.log_N_Sinkhorn_Distance_Loss(0.05, 25, batch_reduction="none", type_of_cost_norm=f"L{norm_p}",
                                                type_of_Wasserstein_N=str(cost_pow))
    xd, yd = x.cuda().requires_grad_(True), y.cuda().requires_grad_(True)
    cost, P, C = crit(xd, yd, "cuda")
    (cost * torch.tensor(cases.VARIANT_W, device="cuda")).sum().backward()
    assert tuple(P.shape) == (2,) + cases.VARIANT_SHAPE
    check_grads(f"variant {tag}", cost, xd.grad, yd.grad, ref, g)


def test_sinkhorn_l1_subgradient_at_zero_difference(shw):
    """Lattice clouds (coordinates k / 8): 6 % of the coordinate differences are exactly 0, where the kernel's choice of
    sign(0) must be torch's (0) -- a +1 or -1 there moves thousands of terms.  measured (kernel gap / mirror gap): cost 0.8, gx 7.3, gy 5.4."""
    x, y, ref, g = cases.l1_lattice_case()
    xd, yd = x.cuda().requires_grad_(True), y.cuda().requires_grad_(True)
    cost, _, _ = shw.log_Sinkhorn_Distance_Loss(0.05, 25, batch_reduction="none", type_of_cost_norm="L1")(xd, yd, "cuda")
    (cost * torch.tensor(cases.VARIANT_W, device="cuda")).sum().backward()
    check_grads("L1 lattice", cost, xd.grad, yd.grad, ref, g)


# ------------------------------------------------------------------------- early stop in training, with backward (4)
@pytest.mark.parametrize("B,n,m,own_copy", cases.STOP_CASES)
def test_sinkhorn_early_stop_in_training_with_backward(shw, B, n, m, own_copy):
    """The device-side flag in training: the value comes from the last EXECUTED slot of the trajectory and the backward
    skips the sweeps that never ran.  The threshold sits (geometrically) half way between the statistic after sweeps 8 and
    9, so the stop is at T = 9 of max_iter = 40.  Value and gradients against the mirror stopped by the same threshold, and
    bit-identical to a run with max_iter = 9 that cannot stop; the value-only path gives the same bits.  own_copy: pair 0
    holds a copy of its own source cloud, so its statistic differs from the others' -- the stop is decided on the batch
    mean.  B = 70: the second trip of the check kernel's `b += 64` loop -- the first 64 pairs are small clouds that
    converge within three sweeps, so a check that saw only them would stop at sweep 3.
    measured (kernel gap / mirror gap; plain, own_copy, B = 70): cost 9.9, 10.4, 2.5; gx 4.3, 3.5, 3.2; gy 1.9, 2.4, 3.2."""
    x, y, w, thresh, free, ref, g = cases.stop_case(B, n, m, own_copy)
    wd = torch.tensor(w, device="cuda")
    runs = []
    for max_iter, th in ((40, thresh), (cases.STOP_T, 0.0)):
        xd, yd = x.cuda().requires_grad_(True), y.cuda().requires_grad_(True)
        cost, _, _ = shw.sinkhorn_pair_costs(xd, yd, 0.5, max_iter, thresh=th)
        (cost * wd).sum().backward()
        runs.append((cost.detach(), xd.grad, yd.grad))
    check_grads(f"early stop B {B} {n}x{m} copy {own_copy}", *runs[0], ref, g)
    for a, b in zip(*runs):
        assert torch.equal(a, b)
    with torch.no_grad():
        plain, _, _ = shw.sinkhorn_pair_costs(x.cuda(), y.cuda(), 0.5, 40, thresh=thresh)
    assert torch.equal(plain, runs[0][0])


# ------------------------------------------------------------------------- determinism and edge arguments (5)
def test_sinkhorn_training_is_bit_identical_from_run_to_run(shw):
    """"no atomics, deterministic": two training runs at (257, 513) return the same bits, cost and both gradients."""
    x, y = cases.variant_inputs()
    runs = []
    for _ in range(2):
        xd, yd = x.cuda().requires_grad_(True), y.cuda().requires_grad_(True)
        cost, _, _ = shw.sinkhorn_pair_costs(xd, yd, 0.05, 25)
        (cost * torch.tensor(cases.VARIANT_W, device="cuda")).sum().backward()
        runs.append((cost.detach(), xd.grad, yd.grad))
    for a, b in zip(*runs):
        assert torch.equal(a, b)


def test_sinkhorn_backward_with_no_sweep(shw):
    """max_iter = 0: the cost of the plan exp(-C / eps) and the backward that has only the cost kernels to run.
    measured (kernel gap / mirror gap): cost 3.6, gx 3.5, gy 1.2."""
    x, y = cases.variant_inputs()
    ref, g = cases.grad_reference(x, y, 0.05, 0, cases.VARIANT_W)
    xd, yd = x.cuda().requires_grad_(True), y.cuda().requires_grad_(True)
    cost, _, _ = shw.sinkhorn_pair_costs(xd, yd, 0.05, 0)
    (cost * torch.tensor(cases.VARIANT_W, device="cuda")).sum().backward()
    check_grads("no sweep", cost, xd.grad, yd.grad, ref, g)


def test_sinkhorn_noncontiguous_input_and_a_zero_upstream_gradient(shw):
    """x is a transposed view of a (B, 3, n) leaf; pair 1 gets an upstream gradient of exactly 0: its gradient rows are
    exactly 0 (not the rounding residue of a product), the others match the mirror.
    Shape (9, 7), the one place where a gradient misses 16 g -- measured gx 15.6 g, gy 30.8 g (2.0e-5 and 3.1e-5 of the
    largest entry; the float32 mirror under 30 random reorderings of the points: 0.8e-6 to 4.7e-6).  The rounding is the
    float32 STORAGE of the duals, amplified by 1 / eps in the weights the backward recomputes: w_ij = exp(M_ij(u_t, v_t)) /
    (b + 1e-8) sums to 1 over i only to ulp(v) / eps ~ 2.4e-6, coherently along the column, where autograd's softmax is
    normalised to 1 ulp; over 30 sweeps and with 7 to 9 entries to average over this does not cancel.  Evaluating the
    kernels' formulas in float64 on a trajectory rounded to float32 reproduces it (3.2e-5 / 2.3e-5), and normalising w, w'
    before use removes it (9e-7 / 6e-7); at 40 x 30 the same experiment gives 1.4e-6 / 2.2e-6.  So these two bounds are
    the next powers of two with a factor 2 of headroom, 32 g (gx) and 64 g (gy); the cost keeps 16 g (measured 4.6)."""
    x, y = cases.forward_inputs(9, 7)
    w = (1.0, 0.0, 0.4)
    ref, g = cases.grad_reference(x, y, 0.05, 30, w)
    leaf = x.transpose(1, 2).contiguous().cuda().requires_grad_(True)
    xv = leaf.transpose(1, 2)
    assert not xv.is_contiguous()
    yd = y.cuda().requires_grad_(True)
    cost, _, _ = shw.sinkhorn_pair_costs(xv, yd, 0.05, 30)
    (cost * torch.tensor(w, device="cuda")).sum().backward()
    gx = leaf.grad.transpose(1, 2)
    assert not gx[1].any() and not yd.grad[1].any()
    assert gx[0].abs().max() > 0 and gx[2].abs().max() > 0
    check_grads("non-contiguous", cost, gx, yd.grad, ref, g, k_of={"gx": 32, "gy": 64})


# --------------------------------------------------------------------------------------------------- Chamfer (6)
def chamfer_forward(shw, x, y):
    """the C entry point itself: min_xy, nn_xy, min_yx, nn_yx, pair_loss"""
    lib = shw._lib.load()
    B, n, _ = x.shape
    m = y.shape[1]
    xd, yd = x.cuda().contiguous(), y.cuda().contiguous()
    min_xy, min_yx = torch.empty(B, n, device="cuda"), torch.empty(B, m, device="cuda")
    nn_xy = torch.full((B, n), -1, dtype=torch.int32, device="cuda")
    nn_yx = torch.full((B, m), -1, dtype=torch.int32, device="cuda")
    pair = torch.empty(B, device="cuda")
    shw._lib.check(lib.shw_chamfer_forward(xd.data_ptr(), yd.data_ptr(), B, n, m, min_xy.data_ptr(), nn_xy.data_ptr(),
                                           min_yx.data_ptr(), nn_yx.data_ptr(), pair.data_ptr(),
                                           torch.cuda.current_stream().cuda_stream), "shw_chamfer_forward")
    return [t.cpu().numpy() for t in (min_xy, nn_xy, min_yx, nn_yx, pair)]


@pytest.mark.parametrize("n,m", cases.CHAMFER_SHAPES)
def test_chamfer_first_minimum_wins_on_lattice_clouds(shw, n, m):
    """Coordinates k / 8: float32 is exact, half of the queries have a tied minimum, and the tied candidates sit in
    different groups of four and different 1024-candidate tiles hundreds of times (counted in the CPU test).  Candidate
    counts 1027 (a 3-candidate tail-only tile after a full one), 2049 and 1029 (second tile boundary; one group + one
    tail), 5, 3 and 1.  The indices ARE numpy's argmin (first minimum), the minima are bit-equal, the pair loss is within
    4 ulp of the float64 value."""
    x, y, ref = cases.chamfer_case("lattice", n, m)
    min_xy, nn_xy, min_yx, nn_yx, pair = chamfer_forward(shw, x, y)
    assert np.array_equal(nn_xy, ref["nn_xy"]) and np.array_equal(nn_yx, ref["nn_yx"])
    assert np.array_equal(min_xy.astype(np.float64), ref["min_xy"])
    assert np.array_equal(min_yx.astype(np.float64), ref["min_yx"])
    ulp = np.spacing(ref["pair"].astype(np.float32)).astype(np.float64)
    assert np.all(np.abs(pair.astype(np.float64) - ref["pair"]) <= 4 * ulp), (pair, ref["pair"])


@pytest.mark.parametrize("n,m", cases.CHAMFER_SHAPES)
def test_chamfer_indices_on_random_clouds(shw, n, m):
    """Random float clouds have no exact ties, but float32 may order two near-equal distances differently from float64:
    where the kernel's index differs from the float64 argmin the distance at the kernel's index is within 1e-6 relative
    of the minimum, and that happens for at most 0.5 % of the queries.  measured: no index differs at any of the shapes."""
    x, y, ref = cases.chamfer_case("random", n, m)
    min_xy, nn_xy, min_yx, nn_yx, pair = chamfer_forward(shw, x, y)
    for axis, idx, mins, key in ((2, nn_xy, min_xy, "nn_xy"), (1, nn_yx, min_yx, "nn_yx")):
        assert idx.min() >= 0 and idx.max() < ref["d"].shape[axis]
        best = ref["d"].min(axis)
        at = np.take_along_axis(ref["d"], np.expand_dims(idx.astype(np.int64), axis), axis).squeeze(axis)
        differ = idx != ref[key]
        print(f"GAP chamfer random {n}x{m} {key}: {int(differ.sum())} of {differ.size} indices differ")
        assert differ.mean() <= 0.005
        assert np.all(at - best <= 1e-6 * best)
        assert rel(mins, best) < 1e-6
    assert rel(pair, ref["pair"]) < 1e-6


@pytest.mark.parametrize("kind,n,m", [("lattice",) + s for s in cases.CHAMFER_SHAPES] + [("clustered",) + cases.CLUSTERED_SHAPE])
def test_chamfer_gradients_against_float64_autograd(shw, kind, n, m):
    """Gradients of (pair_loss * [1, -0.5]).sum() against float64 autograd of the definition, within 16 x the gap of the
    float32 torch evaluation of that same definition (1e-4, the bound of test_chamfer_against_numpy_oracle, as ceiling).
    On the lattice the owner scan must agree with the tie-breaking of the forward; in the clustered case one y point is
    the nearest neighbour of all 1029 x points and its thread adds 1030 terms.
    measured (kernel gap / float32 torch gap): 0.7 to 1.4 on the lattice, 1.0 clustered (all below 3e-7 of the largest entry)."""
    x, y, ref, (gx, gy), (fx, fy) = cases.chamfer_grad_case(kind, n, m)
    xd, yd = x.cuda().requires_grad_(True), y.cuda().requires_grad_(True)
    pair = shw.chamfer_pair_losses(xd, yd)
    (pair * torch.tensor(cases.CHAMFER_W, device="cuda")).sum().backward()
    assert rel(pair.detach().cpu().numpy(), ref["pair"]) < 1e-6
    for name, got, want, g in (("gx", xd.grad, gx, fx), ("gy", yd.grad, gy, fy)):
        gap = cases.of_largest(got.cpu().numpy(), want)
        r = cases.ratio(gap, g)
        print(f"GAP chamfer {kind} {n}x{m} {name}: kernel {gap:.3e} torch-f32 {g:.3e} ratio {r:.2f}")
        assert gap < min(cases.bound(g), 1e-4), f"{name}: kernel gap {gap:.3e} = {r:.1f} x the float32 gap {g:.3e}"
