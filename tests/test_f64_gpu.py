"""Float64 path of the spherical sliced-Wasserstein loss (`-m gpu`, MI355X): equal sizes, uniform weights, any p >= 1.

Two yardsticks, because the reference's bisection is not exact even in double:

* THE DEFINITION, `oracle/exact_shift.py` (float64 numpy, shares no code with the kernels).  The kernels implement
  min_k c(k), so a per-slice cost must be within 1e-12 * cost + 1e-14 of the exhaustive minimum (a sequential sum of n
  terms loses at most n * 2^-53 = 4.5e-13 relative at n = 4096; device and host atan2 may differ by an ulp of a
  coordinate, about 1e-16 absolute), the shift must be the exhaustive argmin on every slice whose second-best cost is
  more than 1e-9 relative above the best (at most 1 % of the slices may be left out by that rule), and every gradient
  entry must be within 1e-10 of the largest entry of `exact_shift.ssw_pair_grad`.  p = 1: `exact_shift.w1_level_median`
  at the same cost bound, gradients against double autograd of `ref_mirror.circular_w1_level_median`.
* THE REAL REFERENCE, fixture G12 (tools/make_golden_f64.py) and the `_f64` rows of G3 / G3b.  Circle rows within 1e-12
  relative; G12 values and per-slice costs within 1e-9 absolute and never above the reference by more than
  1e-12 * cost + 1e-14 (a minimum cannot exceed what a bisection returns); G12 gradients within G12_GRAD_BOUND of the
  largest entry: ten times the worst gap between `exact_shift.ssw_pair_grad` and the fixture's gradients, measured on the
  CPU when the fixture was made (2.54e-14: on the fixture's cases the bisection ends on the kink) and recomputed by
  tests/test_f64_cpu.py.  p = 1 has no bisection: 1e-10 of the largest entry, the bound used against the definition.

float64 is opt-in (`shw.enable_float64()`, the module fixture below): by default double input keeps raising TypeError.
Every test here fails on a library without the float64 path (no `enable_float64`; TypeError "must be float32").
"""
import numpy as np
import pytest
import torch

from helpers.compare import grad_close

pytestmark = pytest.mark.gpu

G12_GRAD_BOUND = 2.54e-13
G12_CASES = (("n256_L32", (1, 2, 3), True), ("n1200_L8", (1, 2), False))
GRADCHECK_SEED, GRADCHECK_ROWS_SEED = 7008, 7102
F64 = torch.float64


@pytest.fixture(scope="module")
def shw():
    import shw_amd
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    shw_amd._lib.load()
    previous = shw_amd.enable_float64(True)         # float64 is opt-in; the other test modules see the default again
    yield shw_amd
    shw_amd.enable_float64(previous)


def unit_cloud(gen, *shape):
    return torch.nn.functional.normalize(torch.randn(*shape, 3, generator=gen, dtype=F64), dim=-1)


def frames(gen, *shape):
    return torch.linalg.qr(torch.randn(*shape, 3, 2, generator=gen, dtype=F64))[0]


def cost_bound(c):
    return 1e-12 * np.abs(c) + 1e-14


def slice_oracle(x, y, U, p):
    """One slice: x, y (n,3), U (3,2) numpy -> exhaustive (cost, k*, relative margin of the second-best shift)."""
    from oracle import exact_shift
    cu = exact_shift.circle_coords(x, U[None])[0]
    cv = exact_shift.circle_coords(y, U[None])[0]
    if p == 1:
        return exact_shift.w1_level_median(cu, cv), None, None
    ks, c = exact_shift.shift_costs(np.sort(cu), np.sort(cv), p)
    j = int(np.argmin(c))
    second = np.partition(c, 1)[1] if c.size > 1 else np.inf
    margin = (second - c[j]) / c[j] if c[j] > 0 else np.inf
    return c[j], int(ks[j]), margin


def check_slices(cost, shift, x, y, U, p, which):
    """cost, shift (B,L) from the kernel against the definition on the (b, l) in `which`; U (B,L,3,2) or shared (L,3,2)."""
    left_out = 0
    for b, l in which:
        Ul = U[l] if U.ndim == 3 else U[b, l]
        c, k, margin = slice_oracle(x[b], y[b], Ul, p)
        print(f"slice b={b} l={l} p={p} n={x.shape[1]}: kernel {cost[b, l]:.17e} oracle {c:.17e} "
              f"diff {cost[b, l] - c:.2e} margin {margin}")
        assert abs(cost[b, l] - c) <= cost_bound(c), (b, l, cost[b, l], c)
        if p != 1:
            if margin > 1e-9:
                assert int(shift[b, l]) == k, (b, l, int(shift[b, l]), k)
            else:
                left_out += 1
    assert left_out <= 0.01 * len(which), (left_out, len(which))


# ------------------------------------------------------------------------------------------------ the definition
@pytest.mark.parametrize("p", [1, 1.5, 2, 3])
@pytest.mark.parametrize("n,L", [(64, 16), (1200, 8), (2048, 6)])
def test_slice_costs_shifts_and_gradients_against_the_definition(shw, n, L, p):
    from oracle import exact_shift, ref_mirror
    B = 2
    g = torch.Generator().manual_seed(12100 + n + int(10 * p))
    x, y, U = unit_cloud(g, B, n), unit_cloud(g, B, n), frames(g, B, L)
    xs, ys = x.cuda().requires_grad_(True), y.cuda().requires_grad_(True)
    pair, cost, shift = shw.ssw_pair_losses(xs, ys, U.cuda(), p=p, return_slices=True)
    assert pair.dtype == F64 and cost.dtype == F64 and shift.dtype == torch.int32
    pair.sum().backward()
    assert xs.grad.dtype == F64 and ys.grad.dtype == F64
    check_slices(cost.cpu().numpy(), shift.cpu().numpy(), x.numpy(), y.numpy(), U.numpy(), p,
                 [(b, l) for b in range(B) for l in range(L)])
    assert np.abs(pair.detach().cpu().numpy() - cost.cpu().numpy().mean(axis=1)).max() <= 1e-15
    if n > 1200 or p == 1.5:                 # the O(L n^2) gradient oracle: the two smaller shapes, integer p
        return
    for b in range(B):
        if p == 1:
            xr, yr = x[b].clone().requires_grad_(True), y[b].clone().requires_grad_(True)
            ref_mirror.sliced_cost(xr, yr, U[b], p=1).backward()
            gx, gy = xr.grad.numpy(), yr.grad.numpy()
        else:
            gx, gy = exact_shift.ssw_pair_grad(x[b].numpy(), y[b].numpy(), U[b].numpy(), p)
        grad_close(xs.grad[b].cpu().numpy(), gx, strict=1e-10, exact=True)
        grad_close(ys.grad[b].cpu().numpy(), gy, strict=1e-10, exact=True)


def test_sizes_up_to_the_limit_shared_and_per_pair_directions(shw):
    """n = m from 1 to the limit; B * L below and above 1024 problems; shared and per-pair directions; a sample of slices
    against the definition.  limit + 1 raises a ValueError that names the limit."""
    limit = shw.ssw.max_points_f64()
    assert limit >= 4096
    sizes = sorted({1, 2, 63, 64, 65, 200, 1000, 1200, 2000, 2048, 3000, 4096, limit})
    for n in sizes:
        g = torch.Generator().manual_seed(12200 + n)
        big = n <= 200                                   # many problems at the small sizes, few at the large ones
        B, L = (5, 250) if big else (2, 3)               # 1250 > 1024 problems / 6
        shared = n % 2 == 0
        x, y = unit_cloud(g, B, n), unit_cloud(g, B, n)
        U = frames(g, L) if shared else frames(g, B, L)
        xs = x.cuda().requires_grad_(True)
        for p in (2, 1):
            pair, cost, shift = shw.ssw_pair_losses(xs, y.cuda(), U.cuda(), p=p, return_slices=True)
            which = [(0, 0), (B - 1, L - 1)] + ([(2, 131), (3, 7)] if big else [])
            check_slices(cost.cpu().numpy(), shift.cpu().numpy(), x.numpy(), y.numpy(), U.numpy(), p, which)
            assert bool(torch.isfinite(cost).all())
            (gx,) = torch.autograd.grad(pair.sum(), xs)
            assert gx.shape == xs.shape and bool(torch.isfinite(gx).all())
    n = limit + 1
    g = torch.Generator().manual_seed(1)
    x = unit_cloud(g, 1, n).cuda()
    with pytest.raises(ValueError, match=str(limit)):
        shw.ssw_pair_losses(x, x, frames(g, 2).cuda(), p=2)
    with pytest.raises(ValueError, match=str(limit)):
        shw.binary_search_circle(torch.rand(1, n, dtype=F64, device="cuda"), torch.rand(1, n, dtype=F64, device="cuda"), p=2)


# ------------------------------------------------------------------------------------------------ the real reference
@pytest.mark.parametrize("tag,powers,with_gy", G12_CASES)
def test_g12_reference_in_double(shw, golden, tag, powers, with_gy):
    g = golden("g12_f64.npz")
    x, y, U = (torch.from_numpy(g[f"{k}_{tag}"]).cuda() for k in ("x", "y", "U"))
    for p in powers:
        xs, ys = x.clone().requires_grad_(True), y.clone().requires_grad_(True)
        val = shw.sliced_cost(xs, ys, U, p=p)
        assert val.dtype == F64 and val.dim() == 0
        val.backward()
        _, cost, _ = shw.ssw_pair_losses(x[None], y[None], U, p=p, return_slices=True)
        cost = cost[0].cpu().numpy()
        want, want_val = g[f"slices_{tag}_p{p}"], float(g[f"val_{tag}_p{p}"])
        print(f"G12 {tag} p={p}: value diff {val.item() - want_val:.3e}, slice diff in "
              f"[{(cost - want).min():.3e}, {(cost - want).max():.3e}]")
        assert np.abs(cost - want).max() <= 1e-9
        assert abs(val.item() - want_val) <= 1e-9
        assert (cost - want <= cost_bound(want)).all()
        assert val.item() - want_val <= cost_bound(want_val)
        bound = 1e-10 if p == 1 else G12_GRAD_BOUND
        grad_close(xs.grad.cpu().numpy(), g[f"gx_{tag}_p{p}"], strict=bound, exact=True)
        if with_gy:
            grad_close(ys.grad.cpu().numpy(), g[f"gy_{tag}_p{p}"], strict=bound, exact=True)


def test_circle_rows_against_the_reference_f64_rows(shw, golden):
    g3, g3b = golden("g3_circle.npz"), golden("g3b_bisection_p1.npz")

    def rows(fix, tag):
        return (torch.from_numpy(fix[f"{k}_{tag}"].astype(np.float64)).cuda() for k in ("u", "v"))

    def close(got, want, what):
        got = got.cpu().numpy()
        rel = np.abs(got - want).max() / np.abs(want).max()
        print(f"{what}: rel {rel:.2e}")
        assert got.dtype == np.float64
        assert (np.abs(got - want) <= 1e-12 * np.abs(want)).all(), what

    for tag in ("64x64", "100x100", "256x256"):
        u, v = rows(g3, tag)
        close(shw.binary_search_circle(u, v, p=2), g3[f"bsc_p2_{tag}_f64"], f"bsc_p2_{tag}")
        close(shw.binary_search_circle(u, v, p=3), g3[f"bsc_p3_{tag}_f64"], f"bsc_p3_{tag}")
        close(shw.emd1D_circle(u, v), g3[f"emd1_{tag}_f64"], f"emd1_{tag}")
        close(shw.binary_search_circle(u, v, p=1), g3b[f"bsc_p1_{tag}_f64"], f"bsc_p1_{tag}")
        close(shw.binary_search_circle(u, v), g3b[f"bsc_p1_{tag}_f64"], f"bsc_default_{tag}")      # p = 1 is the default
    for tag in ("96x96", "1200x1200"):
        u, v = rows(g3b, tag)
        close(shw.binary_search_circle(u, v, p=1), g3b[f"bsc_p1_{tag}_f64"], f"bsc_p1_{tag}")
    u, v = rows(g3, "64x64")                                                                  # 1-D input -> one row
    assert shw.binary_search_circle(u[0], v[0], p=2).shape == (1,)
    with pytest.raises(ValueError):
        shw.emd1D_circle(u, v, p=2)


# ------------------------------------------------------------------------------------------------ gradcheck
def shift_margin(cu, cv, p):
    """Smallest relative lead of the best shift over the second, and smallest distance between two merged coordinates."""
    from oracle import exact_shift
    lead, gap = np.inf, np.inf
    for a, b in zip(cu, cv):
        _, c = exact_shift.shift_costs(np.sort(a), np.sort(b), p)
        s = np.sort(c)
        lead = min(lead, (s[1] - s[0]) / s[0])
        gap = min(gap, np.diff(np.sort(np.concatenate([a, b]))).min())
    return lead, gap


def median_margin(cu, cv):
    """p = 1 level median: how far the cumulated gap weights stay from the 0.5 threshold (the median level jumps there)."""
    far = np.inf
    for a, b in zip(cu, cv):
        n = a.shape[0]
        vals = np.concatenate([np.sort(a), np.sort(b)])
        sign = np.concatenate([np.full(n, 1.0 / n), np.full(n, -1.0 / n)])
        order = np.argsort(vals, kind="stable")
        vals, level = vals[order], np.cumsum(sign[order])
        gaps = np.diff(np.concatenate([vals, [1.0]]))
        acc = np.cumsum(gaps[np.argsort(level, kind="stable")])
        far = min(far, np.abs(acc - 0.5).min())
    return far


@pytest.mark.parametrize("p", [1, 2, 3])
def test_gradcheck_sliced_cost(shw, p):
    """torch.autograd.gradcheck, default tolerances.  The seed is one for which the CPU oracle shows the best shift ahead
    of the second by more than 1e-4 relative on every slice (asserted), coordinates more than 1e-5 apart and, for p = 1,
    the median threshold more than 1e-4 away, so a finite-difference step of 1e-6 cannot cross a kink."""
    from oracle import exact_shift
    g = torch.Generator().manual_seed(GRADCHECK_SEED)
    x, y, U = unit_cloud(g, 2, 24), unit_cloud(g, 2, 24), frames(g, 2, 4)
    for b in range(2):
        cu = exact_shift.circle_coords(x[b].numpy(), U[b].numpy())
        cv = exact_shift.circle_coords(y[b].numpy(), U[b].numpy())
        lead, gap = shift_margin(cu, cv, p)
        assert gap > 1e-5
        if p == 1:
            assert median_margin(cu, cv) > 1e-4
        else:
            assert lead > 1e-4
    Ud = U.cuda()
    xs, ys = x[0].cuda().requires_grad_(True), y[0].cuda().requires_grad_(True)
    assert torch.autograd.gradcheck(lambda a, b: shw.sliced_cost(a, b, Ud[0], p=p), (xs, ys))
    xb, yb = x.cuda().requires_grad_(True), y.cuda().requires_grad_(True)
    assert torch.autograd.gradcheck(lambda a, b: shw.sliced_cost(a, b, Ud, p=p), (xb, yb))


@pytest.mark.parametrize("p", [1, 2])
def test_gradcheck_binary_search_circle(shw, p):
    g = torch.Generator().manual_seed(GRADCHECK_ROWS_SEED)
    u = torch.rand(3, 32, generator=g, dtype=F64)
    v = torch.rand(3, 32, generator=g, dtype=F64)
    lead, gap = shift_margin(u.numpy(), v.numpy(), p)
    assert lead > 1e-4 and gap > 1e-5
    us, vs = u.cuda().requires_grad_(True), v.cuda().requires_grad_(True)
    assert torch.autograd.gradcheck(lambda a, b: shw.binary_search_circle(a, b, p=p), (us, vs))


def test_gradcheck_emd1d_circle(shw):
    g = torch.Generator().manual_seed(GRADCHECK_ROWS_SEED)
    u = torch.rand(3, 32, generator=g, dtype=F64)
    v = torch.rand(3, 32, generator=g, dtype=F64)
    assert shift_margin(u.numpy(), v.numpy(), 1)[1] > 1e-5 and median_margin(u.numpy(), v.numpy()) > 1e-4
    us, vs = u.cuda().requires_grad_(True), v.cuda().requires_grad_(True)
    assert torch.autograd.gradcheck(lambda a, b: shw.emd1D_circle(a, b), (us, vs))


# ------------------------------------------------------------------------------------------------ float32 beside float64
@pytest.mark.parametrize("n,p", [(2048, 2), (2000, 3), (1200, 1.5), (256, 2)])
def test_consistent_with_the_float32_kernels(shw, n, p):
    """On float32-representable inputs the double per-slice costs agree with the float32 kernels' at the tolerances
    test_shift_search_gpu.py uses for float32 against the exhaustive float64 minimum (2e-5 at p = 2, 4e-5 otherwise)."""
    g = torch.Generator().manual_seed(12300 + n)
    B, L = 3, 64
    x = torch.nn.functional.normalize(torch.randn(B, n, 3, generator=g), dim=-1)
    y = torch.nn.functional.normalize(torch.randn(B, n, 3, generator=g), dim=-1)
    U = torch.linalg.qr(torch.randn(B, L, 3, 2, generator=g))[0]
    _, c32, _ = shw.ssw_pair_losses(x.cuda(), y.cuda(), U.cuda(), p=p, return_slices=True)
    _, c64, _ = shw.ssw_pair_losses(x.double().cuda(), y.double().cuda(), U.double().cuda(), p=p, return_slices=True)
    assert c32.dtype == torch.float32 and c64.dtype == F64
    tol = 2e-5 if p == 2 else 4e-5
    rel = ((c32.double() - c64).abs() / c64).max().item()
    print(f"float32 vs float64 n={n} p={p}: max rel {rel:.2e}")
    assert rel <= tol


def test_float32_calls_are_untouched_by_float64_calls(shw):
    g = torch.Generator().manual_seed(12400)
    B, n, L = 4, 512, 32
    x = torch.nn.functional.normalize(torch.randn(B, n, 3, generator=g), dim=-1).cuda()
    y = torch.nn.functional.normalize(torch.randn(B, n, 3, generator=g), dim=-1).cuda()
    U = torch.linalg.qr(torch.randn(B, L, 3, 2, generator=g))[0].cuda()

    def run(a, b, D):
        a = a.clone().requires_grad_(True)
        b = b.clone().requires_grad_(True)
        pair, cost, shift = shw.ssw_pair_losses(a, b, D, p=2, return_slices=True)
        pair.sum().backward()
        return pair.detach().clone(), cost.clone(), shift.clone(), a.grad.clone(), b.grad.clone()

    first = run(x, y, U)
    middle = run(x.double(), y.double(), U.double())
    third = run(x, y, U)
    assert middle[0].dtype == F64 and middle[3].dtype == F64
    for a, b in zip(first, third):
        assert a.dtype == b.dtype and torch.equal(a, b)
    assert first[0].dtype == torch.float32 and first[3].dtype == torch.float32
    # the pools of the two precisions are separate
    keys = list(shw.ssw.SSWWorkspace._pools)
    assert any(torch.float64 in k for k in keys) and any(torch.float32 in k for k in keys)


def test_two_runs_are_bit_identical(shw):
    g = torch.Generator().manual_seed(12500)
    for n, p in ((1200, 2), (300, 1), (777, 2.5)):
        x, y, U = unit_cloud(g, 3, n).cuda(), unit_cloud(g, 3, n).cuda(), frames(g, 3, 40).cuda()
        runs = []
        for _ in range(2):
            a, b = x.clone().requires_grad_(True), y.clone().requires_grad_(True)
            pair, cost, shift = shw.ssw_pair_losses(a, b, U, p=p, return_slices=True)
            pair.sum().backward()
            runs.append((pair.detach(), cost, shift, a.grad, b.grad))
        for a, b in zip(*runs):
            assert torch.equal(a, b)


# ------------------------------------------------------------------------------------------------ call shapes
def test_outputs_call_shapes_and_upstream_weights(shw):
    from oracle import exact_shift
    g = torch.Generator().manual_seed(12600)
    B, n, L = 3, 96, 12
    x, y, U = unit_cloud(g, B, n), unit_cloud(g, B, n), frames(g, B, L)
    w = torch.tensor([0.5, -2.0, 3.25], dtype=F64)
    grads = [exact_shift.ssw_pair_grad(x[b].numpy(), y[b].numpy(), U[b].numpy(), 2) for b in range(B)]
    vals = np.array([exact_shift.ssw_pair(x[b].numpy(), y[b].numpy(), U[b].numpy(), 2) for b in range(B)])
    xd, yd, Ud = x.cuda(), y.cuda(), U.cuda()
    # per-pair upstream weights
    xs, ys = xd.clone().requires_grad_(True), yd.clone().requires_grad_(True)
    pair = shw.ssw_pair_losses(xs, ys, Ud, p=2)
    assert pair.dtype == F64 and np.abs(pair.detach().cpu().numpy() - vals).max() <= 1e-12 * vals.max()
    (pair * w.cuda()).sum().backward()
    for b in range(B):
        grad_close(xs.grad[b].cpu().numpy(), w[b].item() * grads[b][0], strict=1e-10, exact=True)
        grad_close(ys.grad[b].cpu().numpy(), w[b].item() * grads[b][1], strict=1e-10, exact=True)
    # return_total, and pair and total used together
    xs = xd.clone().requires_grad_(True)
    pair, total = shw.ssw_pair_losses(xs, yd, Ud, p=2, return_total=True)
    assert total.dtype == F64 and total.shape == (1,) and abs(total.item() - vals.sum()) <= 1e-12 * vals.sum()
    ((pair * w.cuda()).sum() + 1.5 * total.sum()).backward()
    for b in range(B):
        grad_close(xs.grad[b].cpu().numpy(), (w[b].item() + 1.5) * grads[b][0], strict=1e-10, exact=True)
    # the batched reference shape: shape-[1] total in the INPUT's dtype
    xs = xd.clone().requires_grad_(True)
    tot = shw.sliced_cost(xs, yd, Ud, p=2)
    assert tot.dtype == F64 and tot.shape == (1,)
    tot.backward()
    grad_close(xs.grad[1].cpu().numpy(), grads[1][0], strict=1e-10, exact=True)
    # the per-pair reference shape and return_first
    one = shw.sliced_cost(xd[0], yd[0], Ud[0], p=2)
    assert one.dim() == 0 and one.dtype == F64 and abs(one.item() - vals[0]) <= 1e-12 * vals[0]
    # shared directions
    pair_sh = shw.ssw_pair_losses(xd, yd, Ud[0], p=2)
    assert abs(pair_sh[0].item() - vals[0]) <= 1e-12 * vals[0]
    # evaluation under no_grad: no graph, the loss-only bits
    xs = xd.clone().requires_grad_(True)
    with torch.no_grad():
        quiet = shw.ssw_pair_losses(xs, yd, Ud, p=2)
    assert not quiet.requires_grad and torch.equal(quiet, pair.detach())
    # the drawing call shapes follow the clouds' dtype and consume the generator like a double randn
    torch.manual_seed(77)
    a = shw.sliced_wasserstein_sphere(xd[0], yd[0], 10, "cuda", p=2)
    torch.manual_seed(77)
    D = shw.stiefel_frames(torch.randn(10, 3, 2, device="cuda", dtype=F64))
    assert a.dtype == F64 and torch.equal(a, shw.sliced_cost(xd[0], yd[0], D, p=2))
    torch.manual_seed(78)
    bt = shw.sliced_wasserstein_sphere_fast(xd, yd, 10, "cuda", p=2)
    torch.manual_seed(78)
    D = shw.stiefel_frames(torch.randn(B, 10, 3, 2, device="cuda", dtype=F64))
    assert bt.dtype == F64 and torch.equal(bt, shw.sliced_cost(xd, yd, D, p=2))


def test_float64_is_opt_in(shw):
    """Without enable_float64() double input raises the TypeError it always raised (the message says how to opt in);
    float32 calls do not depend on the switch."""
    g = torch.Generator().manual_seed(12650)
    x, y, U = unit_cloud(g, 2, 32).cuda(), unit_cloud(g, 2, 32).cuda(), frames(g, 2, 4).cuda()
    on = shw.ssw_pair_losses(x, y, U, p=2)
    f32_on = shw.ssw_pair_losses(x.float(), y.float(), U.float(), p=2)
    assert shw.enable_float64(False) is True and not shw.float64_enabled()
    try:
        with pytest.raises(TypeError, match="enable_float64"):
            shw.ssw_pair_losses(x, y, U, p=2)
        with pytest.raises(TypeError, match="enable_float64"):
            shw.sliced_cost(x[0], y[0], U[0], p=2)
        with pytest.raises(TypeError, match="enable_float64"):
            shw.binary_search_circle(torch.rand(2, 8, dtype=F64, device="cuda"), torch.rand(2, 8, dtype=F64, device="cuda"))
        assert torch.equal(shw.ssw_pair_losses(x.float(), y.float(), U.float(), p=2), f32_on)
    finally:
        assert shw.enable_float64(True) is False
    assert torch.equal(shw.ssw_pair_losses(x, y, U, p=2), on)


def test_errors(shw):
    g = torch.Generator().manual_seed(12700)
    x, y, U = unit_cloud(g, 2, 32).cuda(), unit_cloud(g, 2, 32).cuda(), frames(g, 2, 4).cuda()
    with pytest.raises(TypeError):
        shw.ssw_pair_losses(x, y.float(), U, p=2)
    with pytest.raises(TypeError):
        shw.ssw_pair_losses(x, y, U.float(), p=2)
    with pytest.raises(TypeError):
        shw.ssw_pair_losses(x.float(), y.float(), U, p=2)
    with pytest.raises(TypeError):
        shw.binary_search_circle(torch.rand(2, 8, dtype=F64, device="cuda"), torch.rand(2, 8, device="cuda"), p=2)
    wts = torch.full((32,), 1 / 32, dtype=F64, device="cuda")
    with pytest.raises(ValueError, match="float64"):
        shw.ssw_pair_losses(x, y, U, p=2, u_weights=wts)
    with pytest.raises(ValueError, match="float64"):
        shw.sliced_cost(x, y, U, p=2, v_weights=wts.float())
    with pytest.raises(ValueError, match="float64"):
        shw.ssw_pair_losses(x, y[:, :24].contiguous(), U, p=2)
    with pytest.raises(ValueError, match="float64"):
        shw.ssw_pair_losses(x, y[:, :24].contiguous(), U, p=1)
    u = torch.rand(2, 8, dtype=F64, device="cuda")
    with pytest.raises(ValueError, match="float64"):
        shw.binary_search_circle(u, u[:, :6].contiguous(), p=2)
    with pytest.raises(ValueError, match="float64"):
        shw.emd1D_circle(u, u, u_weights=torch.full((8,), 0.125, dtype=F64, device="cuda"))
    with pytest.raises(TypeError):
        shw.stiefel_frames(torch.randn(4, 3, 2, device="cuda").half())


# ------------------------------------------------------------------------------------------------ degenerate inputs
def test_degenerate_inputs(shw):
    from oracle import exact_shift, ref_mirror
    g = torch.Generator().manual_seed(12800)
    n, L = 256, 16
    x, U = unit_cloud(g, n), frames(g, L)
    y = unit_cloud(g, n)
    # identical clouds: c(0) is a sum of exact zeros
    for p in (2, 3, 1.5):
        xs = x.cuda().requires_grad_(True)
        _, cost, shift = shw.ssw_pair_losses(xs[None], x.cuda()[None], U.cuda(), p=p, return_slices=True)
        assert bool((cost == 0).all()) and bool((shift == 0).all())
        val = shw.sliced_cost(xs, x.cuda(), U.cuda(), p=p)
        val.backward()
        assert val.item() == 0.0 and bool(torch.isfinite(xs.grad).all())
    xs = x.cuda().requires_grad_(True)
    val = shw.sliced_cost(xs, x.cuda(), U.cuda(), p=1)
    val.backward()
    cu = exact_shift.circle_coords(x.numpy(), U.numpy())
    want = np.mean([exact_shift.w1_level_median(c, c) for c in cu])
    assert abs(val.item() - want) <= cost_bound(want) and bool(torch.isfinite(xs.grad).all())
    # 32-fold duplicate points, and an all-zero cloud: ref_mirror in double
    dup = unit_cloud(g, n // 32).repeat_interleave(32, dim=0)
    dup8 = unit_cloud(g, n // 8).repeat_interleave(8, dim=0)      # few enough per bin for the distribution sort
    zero = torch.zeros(n, 3, dtype=F64)
    for name, a, b in (("dup", x, dup), ("dup8", dup8, y), ("dup8 both", dup8, dup8.flip(0)), ("dup both", dup, dup.flip(0)), ("zero target", x, zero), ("zero source", zero, y)):
        for p in (2, 1):
            want = ref_mirror.per_slice_costs(a, b, U, p).numpy()
            a_d = a.cuda().requires_grad_(True)
            pair, cost, _ = shw.ssw_pair_losses(a_d[None], b.cuda()[None], U.cuda(), p=p, return_slices=True)
            cost = cost[0].cpu().numpy()
            print(f"{name} p={p}: max diff {np.abs(cost - want).max():.3e}")
            # the mirror bisects: 1e-9 absolute as for G12, and the minimum is never above it
            assert np.abs(cost - want).max() <= 1e-9, (name, p)
            assert (cost - want <= cost_bound(want)).all(), (name, p)
            pair.sum().backward()
            assert bool(torch.isfinite(a_d.grad).all()), (name, p)


# ------------------------------------------------------------------------------------------------ direction frames
def test_stiefel_frames_and_draw_directions_in_double(shw):
    g = torch.Generator().manual_seed(12900)
    Z = torch.randn(5, 300, 3, 2, generator=g, dtype=F64)
    Q = shw.stiefel_frames(Z.cuda())
    assert Q.dtype == F64 and Q.shape == Z.shape
    ref = torch.linalg.qr(Z)[0]
    err = (Q.cpu() - ref).abs().max().item()
    print(f"stiefel_frames f64 vs LAPACK: {err:.2e}")
    assert err <= 1e-13
    torch.manual_seed(4242)
    D = shw.draw_directions(50, "cuda", dtype=torch.float64)
    torch.manual_seed(4242)
    want = shw.stiefel_frames(torch.randn(50, 3, 2, device="cuda", dtype=torch.float64))
    assert D.dtype == F64 and torch.equal(D, want)
    torch.manual_seed(4242)
    Db = shw.draw_directions(7, "cuda", batch=3, dtype=torch.float64)
    torch.manual_seed(4242)
    assert torch.equal(Db, shw.stiefel_frames(torch.randn(3, 7, 3, 2, device="cuda", dtype=torch.float64)))
    torch.manual_seed(4242)
    assert shw.draw_directions(7, "cuda").dtype == torch.float32
