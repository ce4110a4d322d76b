"""GPU tests (`-m gpu`, MI355X) of the generalised sliced-W family: the rows primitive `sorted_row_sums`, the fused
circular defining function `gsw_circular_slice_sums` (csrc/shw_gsw.hip), the polynomial defining function on the
Euclidean kernels, and the notebook cell's call shapes (GSWD_circular, max_GSWD_circular, GSWD_polynomial,
max_GSWD_polynomial_3 / _5, gsw_nn_1, max_gsw_nn_1, distributional_sliced_wasserstein_distance).

  both primitives against the float64 restatement (tests/helpers/gsw_restatement.py): sums and every gradient;
  the fused circular call against the rows primitive fed by torch-computed keys;
  a point exactly at r theta: finite sums and gradients;
  the limits' named errors;
  fixture G16 (tests/golden/g16_notebook_gsw.npz, tools/make_golden_gsw.py: the notebook cell exec'd on the CPU);
  the generator streams; bit-identical gradients from run to run.

Tolerances.  The arithmetic is that of the Euclidean sliced-W kernels (a D-term fp32 key, the same sort, the same
fixed-order sums), so the bounds are theirs (tests/test_esw_dim_gpu.py): slice sums 2e-5 relative plus 1e-6 of the
largest sum; cloud gradients within 5e-4 of the largest entry with grad_close's near-tie allowance; direction
gradients 1e-3 of the largest entry, the same way.  One of them does not hold as it stands and is set from the
restatement's float32 / float64 gap instead: the direction gradient of one point per cloud in R^1, which cancels to
rounding residue -- 9.6e-7 absolute = 4 x the 2.4e-7 the float32 restatement deviates by on the CPU
(one_point_on_a_line_dirs_close).  Fixture cases with an ascent loop are
held to 8 x the fixture's `<case>_*_f32_gap` (the notebook cell's own float32 run against its float64 run: what float32
rounding amplified through ten Adam steps does to the reference itself), never below the single-evaluation bound."""

import numpy as np
import pytest
import torch

from helpers import gsw_restatement as R
from helpers.compare import grad_close

pytestmark = pytest.mark.gpu

SUM_RTOL, SUM_ATOL_OF_MAX = 2e-5, 1e-6
CLOUD_STRICT, DIRS_STRICT = 5e-4, 1e-3
PARAM_ABS = 1e-4      # a parameter after ten Adam steps at lr 0.005: lr * (relative gradient difference <= 1e-3) * 10 = 5e-5
                      # (the reasoning of the G11 test, tests/test_esw_dim_gpu.py), rounded up


@pytest.fixture(scope="module")
def shw():
    import shw_amd
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    shw_amd._lib.load()
    return shw_amd


@pytest.fixture(scope="module")
def g16(golden):
    g = golden("g16_notebook_gsw.npz")
    return {k: g[k] for k in g.files}


@pytest.fixture(scope="module")
def g10_clouds(golden):
    g = golden("g10_notebook_flow.npz")
    return np.ascontiguousarray(g["source"]), np.ascontiguousarray(g["target"])


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda")


def rel(a, b):
    a = np.asarray(a, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    return float(np.max(np.abs(a - b) / np.maximum(np.abs(b), 1e-30)))


def sums_close(got, want):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert np.allclose(got, want, rtol=SUM_RTOL, atol=SUM_ATOL_OF_MAX * np.abs(want).max() + 1e-12), rel(got, want)


def clouds(gen, B, n, D):
    return torch.randn(B, n, D, generator=gen), torch.randn(B, n, D, generator=gen) * 0.7 + 0.2


def directions(shw, B, L, D, per_pair):
    if per_pair:
        return torch.stack([shw.rand_projections(D, L) for _ in range(B)])
    return shw.rand_projections(D, L)


def smallest_key(a, b, th, r):
    keys = [R.circular_keys(x[k].double(), (th[k] if th.dim() == 3 else th).double(), r)
            for x in (a, b) for k in range(a.shape[0])]
    return torch.stack(keys)


def clouds_off_the_singular_points(gen, shw, B, n, D, L, per_pair, r, margin=2e-3):
    """The Euclidean test's inputs (normal clouds, unit directions).  In low dimension a normal cloud of 4096 points puts
    some point within 1e-3 of some r theta (in R^1 r theta is one of two numbers); such points are drawn again, from the
    same generator, until none is left, so that the bounds below never sit on a singular point."""
    a, b = clouds(gen, B, n, D)
    th = directions(shw, B, L, D, per_pair)
    for _ in range(200):
        keys = smallest_key(a, b, th, r)                         # (2B, L, n)
        bad = (keys < margin).any(1).view(2, B, n)
        if not bad.any():
            break
        for x, m, scale, shift in ((a, bad[0], 1.0, 0.0), (b, bad[1], 0.7, 0.2)):
            x[m] = torch.randn(int(m.sum()), D, generator=gen) * scale + shift
    return a, b, th


# ------------------------------------------------------------------------------------------- rows primitive
@pytest.mark.parametrize("n", [1, 63, 64, 65, 1200, 4096])
@pytest.mark.parametrize("p", [1, 2, 3])
@pytest.mark.parametrize("rows", [1, 5, 37])
def test_sorted_row_sums_and_gradients_against_float64(shw, n, p, rows):
    """Row sums 2e-5 relative plus 1e-6 of the largest; both gradients, under a random upstream weight per row, within
    5e-4 of the largest entry (grad_close).  1, 5 and 37 rows are no multiple of a workgroup's 4, 2 or 1 waves."""
    g = torch.Generator().manual_seed(16000 + 31 * n + 7 * p + rows)
    u, v = torch.randn(rows, n, generator=g), torch.randn(rows, n, generator=g) * 0.7 + 0.2
    w = torch.rand(rows, generator=g) + 0.5
    ug, vg = u.cuda().requires_grad_(True), v.cuda().requires_grad_(True)
    sums = shw.sorted_row_sums(ug, vg, p)
    assert sums.shape == (rows,)
    ud, vd = u.double().requires_grad_(True), v.double().requires_grad_(True)
    ref = R.sorted_row_sums(ud, vd, p)
    sums_close(sums.detach().cpu().numpy(), ref.detach().numpy())
    (sums * w.cuda()).sum().backward()
    (ref * w.double()).sum().backward()
    grad_close(ug.grad.cpu().numpy(), ud.grad.numpy(), strict=CLOUD_STRICT)
    grad_close(vg.grad.cpu().numpy(), vd.grad.numpy(), strict=CLOUD_STRICT)


def test_sorted_row_sums_takes_a_transposed_input_and_returns_its_layout(shw):
    """A network's (n, L') output, transposed: a non-contiguous (L', n) view.  Leading dimensions are kept, and the
    gradient has the input's shape and strides."""
    g = torch.Generator().manual_seed(16500)
    n, Lp = 300, 5
    u = torch.randn(n, Lp, generator=g).cuda().t().requires_grad_(True)            # a non-contiguous leaf
    v = (torch.randn(n, Lp, generator=g) * 0.7).cuda()
    assert not u.is_contiguous()
    sums = shw.sorted_row_sums(u, v.t(), 2)
    assert sums.shape == (Lp,)
    ref = R.sorted_row_sums(u.detach().cpu().double().requires_grad_(True), v.t().cpu().double(), 2)
    sums_close(sums.detach().cpu().numpy(), ref.detach().numpy())
    sums.sum().backward()
    assert u.grad.shape == u.shape and u.grad.stride() == u.stride()
    ud = u.detach().cpu().double().requires_grad_(True)
    R.sorted_row_sums(ud, v.t().cpu().double(), 2).sum().backward()
    grad_close(u.grad.cpu().numpy(), ud.grad.numpy(), strict=CLOUD_STRICT)
    batched = shw.sorted_row_sums(u.detach().reshape(1, Lp, n).expand(2, Lp, n), v.t().reshape(1, Lp, n).expand(2, Lp, n))
    assert batched.shape == (2, Lp) and torch.equal(batched[1], batched[0])
    assert torch.allclose(batched[0], sums.detach(), rtol=1e-6, atol=0)     # the value-only kernel against the training one


# ------------------------------------------------------------------------------------------- circular, fused
@pytest.mark.parametrize("D", [1, 2, 3, 4, 5, 6, 64])
@pytest.mark.parametrize("n", [1, 64, 65, 1200, 4096])
@pytest.mark.parametrize("p", [1, 2, 3])
@pytest.mark.parametrize("r", [1, 0.5])
@pytest.mark.parametrize("B,per_pair", [(1, False), (3, True), (3, False)])
def test_circular_slice_sums_and_gradients_against_float64(shw, D, n, p, r, B, per_pair):
    """Slice sums 2e-5 relative plus 1e-6 of the largest; gradients w.r.t. both clouds within 5e-4 of the largest entry
    (grad_close); gradients w.r.t. the directions 1e-3 of the largest entry (grad_close): the Euclidean kernels' bounds.
    One shape needs another bound for the directions, D = 1 with n = 1: see one_point_on_a_line_dirs_close.  The smallest
    float64 key of the case is asserted to exceed 1e-3, so no bound hides a singular point."""
    g = torch.Generator().manual_seed(17000 + 97 * D + n + 13 * p + B + (1000 if r == 1 else 0))
    L = 8
    torch.manual_seed(17100 + D + n + p)
    a, b, th = clouds_off_the_singular_points(g, shw, B, n, D, L, per_pair, r)
    assert smallest_key(a, b, th, r).min().item() > 1e-3
    xa, xb, tg = a.cuda().requires_grad_(True), b.cuda().requires_grad_(True), th.cuda().requires_grad_(True)
    sums = shw.gsw_circular_slice_sums(xa, xb, tg, r, p)
    assert sums.shape == (B, L)
    ad, bd, td = (t.double().requires_grad_(True) for t in (a, b, th))
    ref = R.circular_slice_sums(ad, bd, td, r, p)
    sums_close(sums.detach().cpu().numpy(), ref.detach().numpy())
    w = torch.rand(B, L, generator=g) + 0.5
    (sums * w.cuda()).sum().backward()
    (ref * w.double()).sum().backward()
    assert xa.grad.shape == (B, n, D) and tg.grad.shape == th.shape
    grad_close(xa.grad.cpu().numpy(), ad.grad.numpy(), strict=CLOUD_STRICT)
    grad_close(xb.grad.cpu().numpy(), bd.grad.numpy(), strict=CLOUD_STRICT)
    got, want = tg.grad.cpu().double().numpy(), td.grad.numpy()
    print("directions", D, n, p, r, B, per_pair, "largest entry", np.abs(want).max(), "error", np.abs(got - want).max())
    if D == 1 and n == 1:
        one_point_on_a_line_dirs_close(got, want)
    else:
        grad_close(got, want, strict=DIRS_STRICT)


ONE_POINT_ON_A_LINE_ABS = 4 * 2.4e-7


def one_point_on_a_line_dirs_close(got, want):
    """D = 1, n = 1: theta is +-1, a slice's gradient is -r w g (s_s - s_t) with s = sign(x - r theta) of the one point of
    each cloud, and where both points lie on the same side of r theta it cancels to nothing: in 9 of the 18 cases of this
    shape every slice does, the float64 gradient is 0 or its own rounding (<= 4.4e-16), and 1e-3 of its largest entry
    bounds nothing.  Set as the issue prescribes for a bound that does not hold: the float32 run of the restatement
    deviates from its float64 run, on the same inputs on the CPU, by at most 2.4e-7 over those cases (the kernel: 9.5e-8),
    and 4 x that, 9.6e-7 absolute, is allowed on every entry -- or 1e-3 of the largest entry where that is more, which
    is the Euclidean bound and holds for the other 9 cases; no near-tie allowance, one point has no ties."""
    err = np.abs(got - want).max()
    assert err < max(DIRS_STRICT * np.abs(want).max(), ONE_POINT_ON_A_LINE_ABS), (err, np.abs(want).max())


@pytest.mark.parametrize("n,D,p,r,per_pair", [(1200, 3, 2, 1, False), (65, 5, 1, 0.5, True), (4096, 64, 3, 1, True),
                                              (700, 2, 2, 0.5, False)])
def test_fused_circular_call_agrees_with_rows_fed_by_torch_keys(shw, n, D, p, r, per_pair):
    """The composed path -- torch forms the (B, L, n) keys, sorted_row_sums sorts them -- within the same bounds."""
    g = torch.Generator().manual_seed(17500 + n + D)
    B, L = 3, 8
    torch.manual_seed(17600 + n)
    a, b, th = clouds_off_the_singular_points(g, shw, B, n, D, L, per_pair, r)
    w = (torch.rand(B, L, generator=g) + 0.5).cuda()
    out = {}
    for tag in ("fused", "composed"):
        xa, xb, tg = a.cuda().requires_grad_(True), b.cuda().requires_grad_(True), th.cuda().requires_grad_(True)
        if tag == "fused":
            sums = shw.gsw_circular_slice_sums(xa, xb, tg, r, p)
        else:
            centre = (tg * r).unsqueeze(-2) if per_pair else (tg * r).unsqueeze(0).unsqueeze(-2)   # (B or 1, L, 1, D)
            keys = [(x.unsqueeze(1) - centre).pow(2).sum(-1).sqrt() for x in (xa, xb)]
            sums = shw.sorted_row_sums(keys[0], keys[1], p)
        (sums * w).sum().backward()
        out[tag] = [t.detach().cpu().numpy() for t in (sums, xa.grad, xb.grad, tg.grad)]
    sums_close(out["fused"][0], out["composed"][0])
    grad_close(out["fused"][1], out["composed"][1], strict=CLOUD_STRICT)
    grad_close(out["fused"][2], out["composed"][2], strict=CLOUD_STRICT)
    grad_close(out["fused"][3], out["composed"][3], strict=DIRS_STRICT)


@pytest.mark.parametrize("p,r", [(2, 1), (1, 0.5), (3, 0.5)])
def test_a_point_exactly_at_r_theta_gives_finite_sums_and_gradients(shw, p, r):
    """key 0: the notebook's sqrt has an infinite slope there and its autograd returns NaN; the kernel's contribution of
    that point on that slice is 0 (the one deliberate deviation), and everything stays finite."""
    g = torch.Generator().manual_seed(17700)
    B, n, D, L = 2, 130, 3, 8
    a, b = clouds(g, B, n, D)
    torch.manual_seed(17701)
    th = directions(shw, B, L, D, True)
    a[0, 5] = th[0, 2] * r
    b[1, 77] = th[1, 0] * r
    xa, xb, tg = a.cuda().requires_grad_(True), b.cuda().requires_grad_(True), th.cuda().requires_grad_(True)
    sums = shw.gsw_circular_slice_sums(xa, xb, tg, r, p)
    sums.sum().backward()
    for t in (sums, xa.grad, xb.grad, tg.grad):
        assert torch.isfinite(t).all()
    ref = R.circular_slice_sums(a.double(), b.double(), th.double(), r, p)
    sums_close(sums.detach().cpu().numpy(), ref.numpy())


def test_limits_raise_errors_that_name_them(shw):
    z = lambda *s: torch.zeros(*s, device="cuda")                                   # noqa: E731
    with pytest.raises(ValueError, match="1 to 64"):
        shw.gsw_circular_slice_sums(z(1, 8, 0), z(1, 8, 0), z(4, 0))
    with pytest.raises(ValueError, match="1 to 64"):
        shw.gsw_circular_slice_sums(z(1, 8, 65), z(1, 8, 65), z(4, 65))
    with pytest.raises(ValueError, match="4096"):
        shw.gsw_circular_slice_sums(z(1, 4097, 6), z(1, 4097, 6), z(4, 6))
    with pytest.raises(ValueError, match="equal size"):
        shw.gsw_circular_slice_sums(z(1, 8, 6), z(1, 9, 6), z(4, 6))
    with pytest.raises(TypeError, match="thetas"):
        shw.gsw_circular_slice_sums(z(1, 8, 6), z(1, 8, 6), z(4, 5))
    with pytest.raises(ValueError, match="4096"):
        shw.sorted_row_sums(z(3, 4097), z(3, 4097))
    with pytest.raises(ValueError, match="equal shape"):
        shw.sorted_row_sums(z(3, 8), z(3, 9))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        shw.sorted_row_sums(torch.zeros(3, 8), torch.zeros(3, 8))
    # degree 10 in R^3 has 66 monomials: over the 64 coordinates of the Euclidean kernels
    with pytest.raises(ValueError, match="at most 64"):
        shw.gsw_polynomial_slice_sums(z(1, 8, 3), z(1, 8, 3), z(66, 4), 10)
    with pytest.raises(ValueError, match="at most 64"):
        shw.GSWD_polynomial(z(8, 3), z(8, 3), degree=10, num_projection=4)


# ------------------------------------------------------------------------------------------- fixture G16
def _bounds(g, name):
    """(value relative, gradient strict fraction, parameter absolute) of a fixture case: 8 x the fixture's float32 gaps
    of the case where it has an ascent loop, never below the single-evaluation bounds."""
    value = max(8 * float(g.get(f"{name}_f32_gap", 0.0)), SUM_RTOL)
    grad = max(8 * float(g.get(f"{name}_grad_f32_gap", 0.0)), CLOUD_STRICT)
    param = 8 * float(g.get(f"{name}_param_f32_gap", 0.0))
    return value, grad, param


def _check_case(g, name, val, grad):
    value_tol, grad_tol, _ = _bounds(g, name)
    print(name, "value rel", rel(val.item(), g[f"{name}_value"]), "bound", value_tol, "grad bound", grad_tol)
    assert rel(val.item(), g[f"{name}_value"]) < value_tol
    grad_close(grad.cpu().numpy(), g[f"{name}_grad_first"], strict=grad_tol, loose=max(2e-2, grad_tol))


def _param_close(g, name, got, want):
    tol = max(_bounds(g, name)[2] * np.abs(want).max(), PARAM_ABS)
    err = np.abs(np.asarray(got, dtype=np.float64) - want).max()
    print(name, "parameter abs err", err, "bound", tol)
    assert err < tol, (name, err, tol)


@pytest.mark.parametrize("name", ["circ_p2", "circ_p1"])
def test_g16_gswd_circular(shw, g16, g10_clouds, name):
    """GSWD_circular on the theta the cell drew from the stored seed: value 2e-5 relative, gradient 5e-4."""
    first, target = dev(g10_clouds[0]).requires_grad_(True), dev(g10_clouds[1])
    torch.manual_seed(int(g16[f"{name}_seed"]))
    val = shw.GSWD_circular(first, target, p=float(g16[f"{name}_p"]), num_projection=int(g16[f"{name}_L"]),
                            r=float(g16[f"{name}_r"]), device="cuda")
    val.backward()
    _check_case(g16, name, val, first.grad)
    torch.manual_seed(int(g16[f"{name}_seed"]))
    assert np.allclose(shw.rand_projections(3, int(g16[f"{name}_L"])).numpy(), g16[f"{name}_theta"], rtol=1e-6, atol=1e-7)


def test_g16_max_gswd_circular(shw, g16, g10_clouds):
    """max_iter = 10: value, gradient and the theta reached, 8 x the fixture's float32 gaps or the single-evaluation
    bounds (theta: 1e-4 absolute), whichever is larger."""
    first, target = dev(g10_clouds[0]).requires_grad_(True), dev(g10_clouds[1])
    seed = int(g16["maxcirc_seed"])
    torch.manual_seed(seed)
    val = shw.max_GSWD_circular(first, target, p=2, r=1, device="cuda", max_iter=int(g16["max_iter"]))
    val.backward()
    _check_case(g16, "maxcirc", val, first.grad)
    torch.manual_seed(seed)
    again, theta = shw.gsw._max_GSWD_circular(first.detach(), target, 2, 1, "cuda", int(g16["max_iter"]))
    assert rel(again.item(), val.item()) < 1e-6          # the value-only kernel against the training one
    _param_close(g16, "maxcirc", theta.cpu().numpy(), g16["maxcirc_theta"])


@pytest.mark.parametrize("name,degree", [("poly3", 3), ("poly5", 5)])
def test_g16_gswd_polynomial(shw, g16, g10_clouds, name, degree):
    first, target = dev(g10_clouds[0]).requires_grad_(True), dev(g10_clouds[1])
    assert shw.poly_degree(degree, 3).shape[0] == int(g16[f"{name}_features"])
    val = shw.GSWD_polynomial(first, target, p=2, num_projection=100, degree=degree, device="cuda",
                              coefficient=dev(g16[f"{name}_coefficient"]))
    val.backward()
    _check_case(g16, name, val, first.grad)


@pytest.mark.parametrize("name,degree", [("maxpoly3", 3), ("maxpoly5", 5)])
def test_g16_max_gswd_polynomial(shw, g16, g10_clouds, name, degree):
    first, target = dev(g10_clouds[0]).requires_grad_(True), dev(g10_clouds[1])
    fn = shw.max_GSWD_polynomial_3 if degree == 3 else shw.max_GSWD_polynomial_5
    c0 = dev(g16[f"{name}_coefficient0"])
    val = fn(first, target, p=2, device="cuda", max_iter=int(g16["max_iter"]), coefficient=c0)
    val.backward()
    _check_case(g16, name, val, first.grad)
    again, coef = shw.gsw._max_GSWD_polynomial(first.detach(), target, 2, degree, "cuda", int(g16["max_iter"]), c0)
    assert rel(again.item(), val.item()) < 1e-6          # the value-only kernel against the training one
    _param_close(g16, name, coef.cpu().numpy(), g16[f"{name}_coefficient"])


def test_g16_dswd(shw, g16, g10_clouds):
    """The notebook's DSWD call (L = 100, max_iter = 10, lam = 10, Adam lr 0.005 betas (0.999, 0.999) on a TransformNet(3)).
    The fixture's own float32 run differs from its float64 run by 2e-2 of the largest gradient entry (near-ties in the
    sort resolve differently after ten steps), hence a gradient bound of 8 x that; value and f's parameters are held to
    the single-evaluation bounds, their gaps being far smaller."""
    first, target = dev(g10_clouds[0]).requires_grad_(True), dev(g10_clouds[1])
    f = R.UnitLinear(3, g16["dswd_weight0"], g16["dswd_bias0"]).cuda()
    f_op = torch.optim.Adam(f.parameters(), lr=0.005, betas=(0.999, 0.999))
    torch.manual_seed(int(g16["dswd_seed"]))
    val = shw.distributional_sliced_wasserstein_distance(first, target, int(g16["dswd_L"]), f, f_op, p=2,
                                                         max_iter=int(g16["max_iter"]), lam=float(g16["dswd_lam"]),
                                                         device="cuda")
    val.backward()
    _check_case(g16, "dswd", val, first.grad)
    _param_close(g16, "dswd", f.net[0].weight.detach().cpu().numpy(), g16["dswd_weight"])
    _param_close(g16, "dswd", f.net[0].bias.detach().cpu().numpy(), g16["dswd_bias"])


def _mlp(g, prefix):
    params = [g[f"{prefix}_{k}"] for k in range(6)]
    return R.SmallMLP(3, 4, 8, 2, params).cuda()


def test_g16_gsw_nn_1(shw, g16, g10_clouds):
    first, target = dev(g10_clouds[0]).requires_grad_(True), dev(g10_clouds[1])
    net = _mlp(g16, "mlp_param0")
    val = shw.gsw_nn_1(first, target, net, None, max_iter=10, p=2)
    val.backward()
    _check_case(g16, "nn1", val, first.grad)
    assert shw.gsw_nn_3 is shw.gsw_nn_1 and shw.max_gsw_nn_3 is shw.max_gsw_nn_1


def test_g16_max_gsw_nn_1(shw, g16, g10_clouds):
    """Ten Adam steps (lr 0.005) on the MLP.  Adam moves a weight whose gradient is rounding noise by lr per step in a
    direction the noise picks, so the fixture's own float32 and float64 runs end 4.9e-2 (of the largest weight) apart
    in some weight: the parameter bound is 8 x that, the gradient bound 8 x 2.5e-3."""
    first, target = dev(g10_clouds[0]).requires_grad_(True), dev(g10_clouds[1])
    net = _mlp(g16, "mlp_param0")
    net_op = torch.optim.Adam(net.parameters(), lr=0.005)
    val = shw.max_gsw_nn_1(first, target, net, net_op, max_iter=int(g16["max_iter"]), p=2)
    val.backward()
    _check_case(g16, "maxnn1", val, first.grad)
    scale = max(np.abs(g16[f"maxnn1_param_{k}"]).max() for k in range(6))
    tol = max(_bounds(g16, "maxnn1")[2] * scale, PARAM_ABS)
    for k, q in enumerate(net.parameters()):
        assert np.abs(q.detach().cpu().numpy() - g16[f"maxnn1_param_{k}"]).max() < tol, k


# ------------------------------------------------------------------------------------------- generator streams
def test_gswd_circular_draws_l_times_d_normals_from_the_cpu_generator(shw, g10_clouds):
    first, target = dev(g10_clouds[0]), dev(g10_clouds[1])
    torch.manual_seed(18001)
    shw.GSWD_circular(first, target, p=2, num_projection=37, r=1, device="cuda")
    after = torch.randn(5)
    torch.manual_seed(18001)
    torch.randn((37, 3))
    assert torch.equal(after, torch.randn(5))
    torch.manual_seed(18001)
    shw.max_GSWD_circular(first, target, max_iter=2, device="cuda")
    after = torch.randn(5)
    torch.manual_seed(18001)
    torch.randn((1, 3))
    assert torch.equal(after, torch.randn(5))


def test_dswd_draws_max_iter_plus_two_direction_sets(shw, g16, g10_clouds):
    first, target = dev(g10_clouds[0]), dev(g10_clouds[1])
    f = R.UnitLinear(3, g16["dswd_weight0"], g16["dswd_bias0"]).cuda()
    f_op = torch.optim.Adam(f.parameters(), lr=0.005, betas=(0.999, 0.999))
    max_iter, L = 3, 20
    torch.manual_seed(18002)
    shw.distributional_sliced_wasserstein_distance(first, target, L, f, f_op, max_iter=max_iter, lam=10, device="cuda")
    after = torch.randn(5)
    torch.manual_seed(18002)
    for _ in range(max_iter + 2):
        torch.randn((L, 3))
    assert torch.equal(after, torch.randn(5))


@pytest.mark.parametrize("degree", [3, 5])
def test_gswd_polynomial_draws_its_coefficient_on_the_device(shw, g10_clouds, degree):
    first, target = dev(g10_clouds[0]), dev(g10_clouds[1])
    count = shw.poly_degree(degree, 3).shape[0]
    torch.manual_seed(18003)
    val = shw.GSWD_polynomial(first, target, p=2, num_projection=8, degree=degree, device="cuda")
    torch.manual_seed(18003)
    c = torch.randn((count, 8), device="cuda")
    c = c / torch.sqrt(torch.sum(c ** 2, dim=0))
    sums = shw.gsw_polynomial_slice_sums(first.unsqueeze(0), target.unsqueeze(0), c, degree, 2)
    assert sums.shape == (1, 8)
    assert val.item() == torch.pow(sums.mean(), 0.5).item()
    ref = R.gswd_polynomial(first.cpu().double(), target.cpu().double(), c.cpu().double(), degree, 2)
    assert rel(val.item(), ref.item()) < SUM_RTOL


# ------------------------------------------------------------------------------------------- determinism
def test_gradients_are_bit_identical_from_run_to_run(shw):
    g = torch.Generator().manual_seed(19000)
    B, n, D, L = 3, 1200, 3, 8
    a, b = clouds(g, B, n, D)
    torch.manual_seed(19100)
    th = directions(shw, B, L, D, True)
    w = (torch.rand(B, L, generator=g) + 0.5).cuda()
    u, v = torch.randn(B * L, n, generator=g), torch.randn(B * L, n, generator=g)
    runs = []
    for _ in range(2):
        xa, xb, tg = a.cuda().requires_grad_(True), b.cuda().requires_grad_(True), th.cuda().requires_grad_(True)
        sums = shw.gsw_circular_slice_sums(xa, xb, tg, 1.0, 2)
        (sums * w).sum().backward()
        ug, vg = u.cuda().requires_grad_(True), v.cuda().requires_grad_(True)
        rows = shw.sorted_row_sums(ug, vg, 2)
        (rows * w.reshape(-1)).sum().backward()
        runs.append([t.detach().cpu() for t in (sums, xa.grad, xb.grad, tg.grad, rows, ug.grad, vg.grad)])
    for first, second in zip(*runs):
        assert torch.equal(first, second)
