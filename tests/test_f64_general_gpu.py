"""General float64 circular OT (`-m gpu`, MI355X): weighted and / or unequal-size double clouds, any p >= 1.

Two yardsticks, as for the equal-size float64 path (test_f64_gpu.py):

* THE DEFINITION, tests/helpers/circle_general_exact.py: min over the cut theta in [-1, 1] of the reference's `Cost`,
  evaluated only through `oracle.ref_mirror.cut_cost` / `cut_slopes` (code the kernel shares nothing with), by
  exhaustive evaluation at every kink up to n * m = 3100 and by the certificate search above; p = 1 at the sliced level
  and emd1D_circle: `ref_mirror.circular_w1_level_median`.  A per-slice cost must be within
  max(1e-12 * cost + 1e-14, 10 * S) of it: the first term is `cost_bound` of test_f64_gpu.py, S the rounding spread of
  helpers/f64_general_cases.py (the kernel sums its CDFs in a third order).  Gradients up to 200 x 256: every entry within
  1e-10 of the largest, on slices whose minimiser is isolated (the CPU file asserts that the cases leave out none).
* THE REAL REFERENCE, fixture G14 (tools/make_golden_f64_general.py): values and per-slice costs within 1e-9 absolute and
  never above the reference by more than the bound above (a minimum cannot exceed what a bisection returns); gradients
  for p != 1 within ten times the worst gap between the definition's gradient and the fixture's, measured on the CPU
  when the fixture was made (1.395e-06: the reference's bisection ends off the kink) and recomputed by
  test_f64_general_cpu.py; p = 1 has no bisection: 1e-10 of the largest entry.

The path is its own opt-in on top of `enable_float64()` (the module fixture turns both on and restores them).  Every
test here fails on a library without `enable_float64_general`.
"""
import numpy as np
import pytest
import torch

from helpers import circle_general_exact as exact
from helpers import f64_general_cases as cases
from helpers.compare import grad_close

pytestmark = pytest.mark.gpu

F64 = torch.float64
G14_GRAD_BOUND = 1.396e-05
G14_SLICED = (("n256_m200_L16w", True, (1, 2, 3), True), ("n256_m200_L8u", False, (1, 2), False),
              ("n1200_m1000_L4w", True, (2,), False))


@pytest.fixture(scope="module")
def shw():
    import shw_amd
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    shw_amd._lib.load()
    previous = shw_amd.enable_float64(True)
    previous_general = shw_amd.enable_float64_general(True)
    yield shw_amd
    shw_amd.enable_float64_general(previous_general)
    shw_amd.enable_float64(previous)


def cost_bound(c):
    return np.maximum(1e-12 * np.abs(c) + 1e-14, 10 * cases.ROUNDING_SPREAD)


def cuda(t):
    return None if t is None else t.cuda()


def run_case(shw, x, y, U, wu, wv, p, grads):
    xs, ys = x.cuda().requires_grad_(grads), y.cuda().requires_grad_(grads)
    pair, cost, shift = shw.ssw_pair_losses(xs, ys, U.cuda(), p=p, return_slices=True, u_weights=cuda(wu),
                                            v_weights=cuda(wv))
    assert pair.dtype == F64 and cost.dtype == F64 and shift.dtype == torch.int32 and not bool(shift.any())
    if grads:
        pair.sum().backward()
        assert xs.grad.dtype == F64 and ys.grad.dtype == F64
    return pair.detach().cpu().numpy(), cost.cpu().numpy(), (xs.grad.cpu().numpy(), ys.grad.cpu().numpy()) if grads else None


def against_definition(shw, n, m, p, mode, many=False, grads=False):
    x, y, U, wu, wv = cases.case(n, m, p, mode, many)
    pair, cost, got = run_case(shw, x, y, U, wu, wv, p, grads)
    xe, ye = x.clone().requires_grad_(grads), y.clone().requires_grad_(grads)
    want, iso = exact.batch_slice_costs(xe, ye, U, p, wu, wv)
    w = want.detach().numpy()
    diff = np.abs(cost - w)
    print(f"n={n} m={m} p={p} weights={mode} problems={cost.size}: cost diff max {diff.max():.2e} "
          f"(bound {cost_bound(w).min():.1e}), not isolated {int((~iso).sum())}")
    assert (diff <= cost_bound(w)).all(), (n, m, p, mode, diff.max())
    assert np.abs(pair - cost.mean(axis=1)).max() <= 1e-15
    if grads:
        left_out = int((~iso).sum())
        assert left_out <= 0.01 * iso.numel()
        if left_out == 0:                       # (the CPU file asserts that no case leaves a slice out)
            want.mean(1).sum().backward()
            for b in range(x.shape[0]):
                grad_close(got[0][b], xe.grad[b].numpy(), strict=1e-10, exact=True)
                grad_close(got[1][b], ye.grad[b].numpy(), strict=1e-10, exact=True)


# ------------------------------------------------------------------------------------------------ the definition
@pytest.mark.parametrize("p", cases.POWERS)
@pytest.mark.parametrize("n,m", cases.SHAPES)
def test_slice_costs_and_gradients_against_the_definition(shw, n, m, p):
    for mode in cases.modes_for(n, m):
        against_definition(shw, n, m, p, mode, grads=(n, m) in cases.GRAD_SHAPES)


@pytest.mark.parametrize("p", cases.POWERS)
@pytest.mark.parametrize("n,m", cases.MANY)
def test_more_than_1024_problems_against_the_definition(shw, n, m, p):
    for mode in cases.modes_for(n, m):
        against_definition(shw, n, m, p, mode, many=True)


@pytest.mark.parametrize("p", cases.POWERS)
def test_the_limit_against_the_definition(shw, p):
    limit = shw.max_points_f64_general()
    assert limit >= 2048
    g = torch.Generator().manual_seed(14200 + int(10 * p))
    x, y, U = cases.unit_cloud(g, 1, limit), cases.unit_cloud(g, 1, limit - 1), cases.frames(g, 2)
    wu = cases.weights(g, limit)
    for a, b, wa in ((x, y, wu), (y, x, None)):              # the limit as the source and as the target
        pair, cost, got = run_case(shw, a, b, U, wa, None, p, True)
        want, _ = exact.batch_slice_costs(a, b, U, p, wa, None)
        print(f"limit p={p}: cost diff max {np.abs(cost - want.numpy()).max():.2e}")
        assert (np.abs(cost - want.numpy()) <= cost_bound(want.numpy())).all()
        assert np.isfinite(got[0]).all() and np.isfinite(got[1]).all()


@pytest.mark.parametrize("p", cases.POWERS)
def test_zero_weights_and_duplicated_points(shw, p):
    """Three exactly-zero weights and two duplicated points: equal CDF levels and zero-width segments (values only)."""
    g = torch.Generator().manual_seed(14300)
    n, m = 40, 33
    x, y, U = cases.unit_cloud(g, 2, n), cases.unit_cloud(g, 2, m), cases.frames(g, 3)
    x[:, 7] = x[:, 3]
    y[:, m - 1] = y[:, 0]
    wu, wv = cases.weights(g, n), cases.weights(g, m)
    wu[0] = wu[n - 1] = 0.0
    wv[5] = 0.0
    wu, wv = wu / wu.sum(), wv / wv.sum()
    _, cost, _ = run_case(shw, x, y, U, wu, wv, p, False)
    want, _ = exact.batch_slice_costs(x, y, U, p, wu, wv)
    print(f"zero weights p={p}: cost diff max {np.abs(cost - want.numpy()).max():.2e}")
    assert (np.abs(cost - want.numpy()) <= cost_bound(want.numpy())).all()


# ------------------------------------------------------------------------------------------------ the real reference
@pytest.mark.parametrize("tag,weighted,powers,with_gy", G14_SLICED)
def test_g14_reference_in_double(shw, golden, tag, weighted, powers, with_gy):
    g = golden("g14_f64_general.npz")
    assert 10 * float(g["grad_gap_worst"]) <= G14_GRAD_BOUND
    x, y, U = (torch.from_numpy(g[f"{k}_{tag}"]).cuda() for k in ("x", "y", "U"))
    wu = torch.from_numpy(g[f"wu_{tag}"]).cuda() if weighted else None
    wv = torch.from_numpy(g[f"wv_{tag}"]).cuda() if weighted else None
    for p in powers:
        xs, ys = x.clone().requires_grad_(True), y.clone().requires_grad_(True)
        val = shw.sliced_cost(xs, ys, U, p=p, u_weights=wu, v_weights=wv)
        assert val.dtype == F64 and val.dim() == 0
        val.backward()
        _, cost, _ = shw.ssw_pair_losses(x[None], y[None], U, p=p, return_slices=True, u_weights=wu, v_weights=wv)
        cost = cost[0].cpu().numpy()
        want, want_val = g[f"slices_{tag}_p{p}"], float(g[f"val_{tag}_p{p}"])
        print(f"G14 {tag} p={p}: value diff {val.item() - want_val:.3e}, slice diff in "
              f"[{(cost - want).min():.3e}, {(cost - want).max():.3e}]")
        assert np.abs(cost - want).max() <= 1e-9
        assert abs(val.item() - want_val) <= 1e-9
        assert (cost - want <= cost_bound(want)).all()
        assert val.item() - want_val <= cost_bound(want_val)
        bound = 1e-10 if p == 1 else G14_GRAD_BOUND
        grad_close(xs.grad.cpu().numpy(), g[f"gx_{tag}_p{p}"], strict=bound, exact=True)
        if with_gy:
            grad_close(ys.grad.cpu().numpy(), g[f"gy_{tag}_p{p}"], strict=bound, exact=True)


@pytest.mark.parametrize("tag", ["rows_w", "rows_u"])
def test_g14_circle_rows(shw, golden, tag):
    g = golden("g14_f64_general.npz")
    u, v = torch.from_numpy(g["u_rows"]).cuda(), torch.from_numpy(g["v_rows"]).cuda()
    wu = torch.from_numpy(g["wu_rows"]).cuda() if tag == "rows_w" else None
    wv = torch.from_numpy(g["wv_rows"]).cuda() if tag == "rows_w" else None
    for p in (1, 2, 3):
        got = shw.binary_search_circle(u, v, u_weights=wu, v_weights=wv, p=p).cpu().numpy()
        want = g[f"bsc_p{p}_{tag}"]
        print(f"G14 {tag} bsc p={p}: diff in [{(got - want).min():.3e}, {(got - want).max():.3e}]")
        assert got.dtype == np.float64 and np.abs(got - want).max() <= 1e-9
        assert (got - want <= cost_bound(want)).all()
    got = shw.emd1D_circle(u, v, u_weights=wu, v_weights=wv).cpu().numpy()
    want = g[f"emd1_{tag}"]
    print(f"G14 {tag} emd1: diff max {np.abs(got - want).max():.3e}")
    assert np.abs(got - want).max() <= 1e-9 and (got - want <= cost_bound(want)).all()


# ------------------------------------------------------------------------------------------------ gradcheck
@pytest.mark.parametrize("p", [1, 2, 3])
def test_gradcheck_sliced_cost(shw, p):
    """torch.autograd.gradcheck, default tolerances, (12, 9) weighted, L = 3.  The seed is one for which the CPU helper
    shows an isolated minimiser on every slice and merged coordinates more than 1e-5 apart (asserted here and in the CPU
    file), so a finite-difference step of 1e-6 does not cross a kink."""
    x, y, U, wu, wv = cases.gradcheck_clouds(cases.GRADCHECK_SEED)
    assert cases.gradcheck_margins_ok(x, y, U, wu, wv, p)
    Ud, wud, wvd = U.cuda(), wu.cuda(), wv.cuda()
    xs, ys = x[0].cuda().requires_grad_(True), y[0].cuda().requires_grad_(True)
    assert torch.autograd.gradcheck(lambda a, b: shw.sliced_cost(a, b, Ud[0], p=p, u_weights=wud, v_weights=wvd), (xs, ys))
    xb, yb = x.cuda().requires_grad_(True), y.cuda().requires_grad_(True)
    assert torch.autograd.gradcheck(lambda a, b: shw.sliced_cost(a, b, Ud, p=p, u_weights=wud, v_weights=wvd), (xb, yb))


@pytest.mark.parametrize("fn", ["binary_search_circle", "emd1D_circle"])
def test_gradcheck_circle_rows(shw, fn):
    u, v, wu, wv = cases.gradcheck_rows(cases.GRADCHECK_ROWS_SEED)
    assert cases.gradcheck_rows_margins_ok(u, v, wu, wv, 2 if fn == "binary_search_circle" else 1)
    us, vs = u.cuda().requires_grad_(True), v.cuda().requires_grad_(True)
    wud, wvd = wu.cuda(), wv.cuda()
    if fn == "binary_search_circle":
        assert torch.autograd.gradcheck(lambda a, b: shw.binary_search_circle(a, b, wud, wvd, p=2), (us, vs))
    else:
        assert torch.autograd.gradcheck(lambda a, b: shw.emd1D_circle(a, b, wud, wvd), (us, vs))


# ------------------------------------------------------------------------------------------------ determinism, float32
def test_two_runs_are_bit_identical(shw):
    g = torch.Generator().manual_seed(14600)
    n, m, B, L = 200, 256, 5, 210                           # 1050 > 1024 problems
    x, y, U = cases.unit_cloud(g, B, n).cuda(), cases.unit_cloud(g, B, m).cuda(), cases.frames(g, B, L).cuda()
    wu, wv = cases.weights(g, B, n).cuda(), cases.weights(g, m).cuda()
    for p in (2, 1):
        runs = []
        for _ in range(2):
            a, b = x.clone().requires_grad_(True), y.clone().requires_grad_(True)
            pair, cost, _ = shw.ssw_pair_losses(a, b, U, p=p, return_slices=True, u_weights=wu, v_weights=wv)
            pair.sum().backward()
            runs.append((pair.detach(), cost, a.grad, b.grad))
        for a, b in zip(*runs):
            assert torch.equal(a, b)


def test_float32_calls_are_untouched_by_general_float64_calls(shw):
    g = torch.Generator().manual_seed(14700)
    B, n, m, L = 3, 300, 256, 16
    x = cases.unit_cloud(g, B, n).float().cuda()
    y = cases.unit_cloud(g, B, m).float().cuda()
    U = cases.frames(g, B, L).float().cuda()
    w = cases.weights(g, n).float().cuda()

    def run(a, b, D, wa):
        a, b = a.clone().requires_grad_(True), b.clone().requires_grad_(True)
        pair, cost, _ = shw.ssw_pair_losses(a, b, D, p=2, return_slices=True, u_weights=wa)
        pair.sum().backward()
        return pair.detach().clone(), cost.clone(), a.grad.clone(), b.grad.clone()

    first = run(x, y, U, w)
    middle = run(x.double(), y.double(), U.double(), w.double())
    third = run(x, y, U, w)
    assert middle[0].dtype == F64 and middle[2].dtype == F64 and first[0].dtype == torch.float32
    for a, b in zip(first, third):
        assert a.dtype == b.dtype and torch.equal(a, b)


@pytest.mark.parametrize("n,m", [(200, 256), (1200, 1000)])
def test_consistent_with_the_float32_general_kernels(shw, n, m):
    """On float32-representable clouds and weights the double per-slice costs agree with `shw_ssw_forward_general`'s at
    the tolerance test_ssw_gpu.py uses for that path against its oracle (rtol 5e-5, atol 1e-9)."""
    g = torch.Generator().manual_seed(14800 + n)
    B, L = 2, 8
    x, y, U = cases.unit_cloud(g, B, n).float(), cases.unit_cloud(g, B, m).float(), cases.frames(g, B, L).float()
    wu, wv = cases.weights(g, n).float(), cases.weights(g, m).float()
    for p in (2, 3):
        _, c32, _ = shw.ssw_pair_losses(x.cuda(), y.cuda(), U.cuda(), p=p, return_slices=True, u_weights=wu.cuda(),
                                        v_weights=wv.cuda())
        _, c64, _ = shw.ssw_pair_losses(x.double().cuda(), y.double().cuda(), U.double().cuda(), p=p, return_slices=True,
                                        u_weights=wu.double().cuda(), v_weights=wv.double().cuda())
        assert c32.dtype == torch.float32 and c64.dtype == F64
        print(f"float32 vs float64 general n={n} m={m} p={p}: max rel {((c32.double() - c64).abs() / c64).max().item():.2e}")
        assert np.allclose(c32.cpu().numpy(), c64.cpu().numpy(), rtol=5e-5, atol=1e-9)


# ------------------------------------------------------------------------------------------------ errors, call shapes
def test_errors(shw):
    g = torch.Generator().manual_seed(14900)
    x, y, U = cases.unit_cloud(g, 2, 32).cuda(), cases.unit_cloud(g, 2, 24).cuda(), cases.frames(g, 2, 4).cuda()
    wts = cases.weights(g, 32).cuda()
    u = torch.rand(2, 8, dtype=F64, device="cuda")
    assert shw.enable_float64_general(False) is True and not shw.float64_general_enabled()
    try:                                                    # the switch off: the ValueError of before
        with pytest.raises(ValueError, match="float64"):
            shw.ssw_pair_losses(x, y, U, p=2)
        with pytest.raises(ValueError, match="enable_float64_general"):
            shw.ssw_pair_losses(x, x, U, p=2, u_weights=wts)
        with pytest.raises(ValueError, match="float64"):
            shw.binary_search_circle(u, u[:, :6].contiguous(), p=2)
        with pytest.raises(ValueError, match="float64"):
            shw.emd1D_circle(u, u, u_weights=torch.full((8,), 0.125, dtype=F64, device="cuda"))
    finally:
        assert shw.enable_float64_general(True) is False
    limit = shw.max_points_f64_general()
    big = cases.unit_cloud(g, 1, limit + 1).cuda()
    with pytest.raises(ValueError, match=str(limit)):
        shw.ssw_pair_losses(big, x[:1], U[0], p=2)
    with pytest.raises(ValueError, match=str(limit)):
        shw.ssw_pair_losses(x[:1], big, U[0], p=1)
    with pytest.raises(ValueError, match=str(limit)):
        shw.binary_search_circle(torch.rand(1, limit + 1, dtype=F64, device="cuda"), u[:1], p=2)
    with pytest.raises(ValueError, match=str(limit)):
        shw.emd1D_circle(u[:1], torch.rand(1, limit + 1, dtype=F64, device="cuda"))
    with pytest.raises(TypeError):                          # weights of the other dtype
        shw.ssw_pair_losses(x, y, U, p=2, u_weights=wts.float())
    with pytest.raises(TypeError):
        shw.ssw_pair_losses(x.float(), y.float(), U.float(), p=2, u_weights=wts)
    with pytest.raises(TypeError):
        shw.binary_search_circle(u, u, u_weights=torch.full((8,), 0.125, device="cuda"), p=2)
    with pytest.raises(ValueError):
        shw.emd1D_circle(u, u[:, :6].contiguous(), p=2)


def test_call_shapes_dtypes_and_upstream_weights(shw):
    g = torch.Generator().manual_seed(15000)
    B, n, m, L = 3, 40, 28, 5
    x, y, U = cases.unit_cloud(g, B, n), cases.unit_cloud(g, B, m), cases.frames(g, B, L)
    wu, wv = cases.weights(g, n), cases.weights(g, B, m)
    w = torch.tensor([0.5, -2.0, 3.25], dtype=F64)
    xe, ye = x.clone().requires_grad_(True), y.clone().requires_grad_(True)
    want, iso = exact.batch_slice_costs(xe, ye, U, 2, wu, wv)
    assert bool(iso.all())
    vals = want.mean(1)

    def definition_grads(weights_of_pairs):
        gx, gy = torch.autograd.grad((vals * weights_of_pairs).sum(), (xe, ye), retain_graph=True)
        return gx.numpy(), gy.numpy()

    xd, yd, Ud, kw = x.cuda(), y.cuda(), U.cuda(), dict(u_weights=wu.cuda(), v_weights=wv.cuda())
    # pair.sum()
    xs, ys = xd.clone().requires_grad_(True), yd.clone().requires_grad_(True)
    pair = shw.ssw_pair_losses(xs, ys, Ud, p=2, **kw)
    assert pair.dtype == F64 and np.abs(pair.detach().cpu().numpy() - vals.detach().numpy()).max() <= 1e-12
    pair.sum().backward()
    gx, gy = definition_grads(torch.ones(B, dtype=F64))
    assert xs.grad.dtype == F64 and ys.grad.dtype == F64
    grad_close(xs.grad.cpu().numpy(), gx, strict=1e-10, exact=True)
    grad_close(ys.grad.cpu().numpy(), gy, strict=1e-10, exact=True)
    # a weighted sum of pairs, with the total
    xs, ys = xd.clone().requires_grad_(True), yd.clone().requires_grad_(True)
    pair, total = shw.ssw_pair_losses(xs, ys, Ud, p=2, return_total=True, **kw)
    assert total.dtype == F64 and total.shape == (1,) and abs(total.item() - vals.sum().item()) <= 1e-12
    ((pair * w.cuda()).sum() + 1.5 * total.sum()).backward()
    gx, gy = definition_grads(w + 1.5)
    grad_close(xs.grad.cpu().numpy(), gx, strict=1e-10, exact=True)
    grad_close(ys.grad.cpu().numpy(), gy, strict=1e-10, exact=True)
    # the batched total of the reference's call shape, and the per-pair one
    xs = xd.clone().requires_grad_(True)
    tot = shw.sliced_cost(xs, yd, Ud, p=2, **kw)
    assert tot.dtype == F64 and tot.shape == (1,)
    tot.backward()
    grad_close(xs.grad.cpu().numpy(), definition_grads(torch.ones(B, dtype=F64))[0], strict=1e-10, exact=True)
    one = shw.sliced_cost(xd[1], yd[1], Ud[1], p=2, u_weights=wu.cuda(), v_weights=wv[1].cuda())
    assert one.dim() == 0 and one.dtype == F64 and abs(one.item() - vals[1].item()) <= 1e-12
    # 1-D coordinate rows
    u, v = torch.rand(9, generator=g, dtype=F64), torch.rand(7, generator=g, dtype=F64)
    got = shw.binary_search_circle(u.cuda(), v.cuda(), p=2)
    ref, _, _ = exact.circle_min(u[None], v[None], 2)
    assert got.shape == (1,) and got.dtype == F64 and abs(got.item() - ref.item()) <= cost_bound(ref.item())
    got = shw.emd1D_circle(u.cuda(), v.cuda())
    assert got.shape == (1,) and abs(got.item() - exact.circle_level_median(u[None], v[None]).item()) <= cost_bound(got.item())


@pytest.mark.parametrize("p", [1, 2])
def test_all_zero_target_cloud(shw, p):
    """Every coordinate of the target 0 (projection (0, 0), circle coordinate 0 as in the reference), n != m."""
    g = torch.Generator().manual_seed(15100)
    x, U = cases.unit_cloud(g, 1, 50), cases.frames(g, 4)
    y = torch.zeros(1, 37, 3, dtype=F64)
    pair, cost, got = run_case(shw, x, y, U, None, None, p, True)
    want, _ = exact.batch_slice_costs(x, y, U, p)
    print(f"zero target p={p}: cost diff max {np.abs(cost - want.numpy()).max():.2e}")
    assert np.isfinite(cost).all() and np.isfinite(got[0]).all() and np.isfinite(got[1]).all()
    assert (np.abs(cost - want.numpy()) <= cost_bound(want.numpy())).all()
