"""GPU tests of the D-generic spherical sliced-W path (`-m gpu`): clouds (B, n, d) on S^(d-1) and frames (..., d, 2),
2 <= d <= 64, float32 -- the coordinates kernel, the circle-level solvers on its rows, the D-generic point-gradient and
frames kernels of csrc/shw_ssw_dim.hip, through the package's mirror of the reference signatures, against
  (a) fixture G15, the real reference at d != 3 in float32 and float64 (tools/make_golden_sphere_dim.py),
  (b) the CPU oracle in float64 (oracle/ref_mirror.py: dimension-blind, differentiated by autograd) on seeded inputs.

Tolerances are those of tests/test_ssw_gpu.py's header: values 1e-5 relative; per-slice costs 2e-5 relative -- or four
times the gap between the reference's own float32 and float64 per-slice arrays stored in the fixture where that is
larger (d = 64: a 64-term projection); gradients by grad_close() (every entry within 2e-2 of the largest, all but 0.15 %
or 8 entries within 2e-4), on the fixture with the count outside 2e-4 pinned at one swapped pair of points = 2 d entries,
which the reference's own float32 run meets against its float64 run (asserted when the fixture was made, `swap_*`).
Coordinates: circular distance to the float64 oracle <= 1e-6 + 4 x the float32 oracle's own worst distance on the same
inputs.  Frames: 4 x the largest difference between torch.linalg.qr in float32 and in float64 on the same Z (CPU).
"""
import functools

import numpy as np
import pytest
import torch

from helpers.compare import grad_close

pytestmark = pytest.mark.gpu

PAIR_CASES = (("d2_n64_m64_L8u", (1, 2)), ("d8_n256_m256_L16u", (1, 2, 3)), ("d6_n200_m256_L8u", (1, 2)),
              ("d16_n128_m128_L8w", (2,)), ("d64_n100_m100_L8u", (2,)))


@pytest.fixture(scope="module")
def shw():
    import shw_amd
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    shw_amd._lib.load()
    return shw_amd


@pytest.fixture(scope="module")
def g15(golden):
    return golden("g15_sphere_dim.npz")


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda")


def rel(a, b):
    a = np.asarray(a, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    return float(np.max(np.abs(a - b) / np.maximum(np.abs(b), 1e-30)))


def case_dim(tag):
    return int(tag[1:tag.index("_")])


# ------------------------------------------------------------------------------ G15 against the reference
@pytest.mark.parametrize("tag,p", [(tag, p) for tag, powers in PAIR_CASES for p in powers])
def test_g15_pair_cases_value_slices_gradients(shw, g15, tag, p):
    g, d = g15, case_dim(tag)
    x, y, U = dev(g[f"x_{tag}"]).requires_grad_(True), dev(g[f"y_{tag}"]).requires_grad_(True), dev(g[f"U_{tag}"])
    wu = dev(g[f"wu_{tag}"]) if tag.endswith("w") else None
    wv = dev(g[f"wv_{tag}"]) if tag.endswith("w") else None
    pair, cost, _ = shw.ssw_pair_losses(x.unsqueeze(0), y.unsqueeze(0), U, p=p, return_slices=True, u_weights=wu,
                                        v_weights=wv)
    loss = shw.sliced_cost(x, y, U, p=p, u_weights=wu, v_weights=wv)
    assert loss.dim() == 0 and loss.dtype == torch.float32
    loss.backward()
    s32, s64 = g[f"slices_{tag}_p{p}"].astype(np.float64), g[f"slices64_{tag}_p{p}"]
    slice_tol = max(2e-5, 4 * float(np.max(np.abs(s32 - s64) / np.abs(s64))))
    got = cost[0].cpu().numpy().astype(np.float64)
    print(f"{tag} p={p}: loss rel {rel(loss.item(), g[f'val64_{tag}_p{p}']):.2e}, slices rel {rel(got, s64):.2e} "
          f"(tolerance {slice_tol:.2e})")
    assert rel(loss.item(), g[f"val_{tag}_p{p}"]) < 1e-5
    assert rel(loss.item(), g[f"val64_{tag}_p{p}"]) < 1e-5
    assert rel(pair[0].item(), g[f"val64_{tag}_p{p}"]) < 1e-5
    assert np.all(np.abs(got - s64) <= slice_tol * np.abs(s64) + 1e-10)
    grad_close(x.grad.cpu().numpy(), g[f"gx64_{tag}_p{p}"], max_outside=2 * d)
    grad_close(y.grad.cpu().numpy(), g[f"gy64_{tag}_p{p}"], max_outside=2 * d)


def test_g15_batched_total_and_first_pair(shw, g15):
    g = g15
    x, y, U = dev(g["batched_x"]), dev(g["batched_y"]), dev(g["batched_U"])
    total = shw.sliced_cost(x, y, U, p=2)
    assert tuple(total.shape) == (1,)
    assert rel(total.item(), g["batched_total"][0]) < 1e-5 and rel(total.item(), g["batched_total64"][0]) < 1e-5
    first = shw.ssw_pair_losses(x, y, U, p=2, return_first=True)
    assert first.dim() == 0
    assert rel(first.item(), g["batched_first"]) < 1e-5 and rel(first.item(), g["batched_first64"]) < 1e-5


@pytest.mark.parametrize("d", [2, 5, 64])
def test_g15_frames_kernel_against_lapack(shw, g15, d):
    Z, U_ref = g15[f"frames_Z_d{d}"], g15[f"frames_U_d{d}"]
    Zt = torch.from_numpy(Z)
    q32, q64 = torch.linalg.qr(Zt)[0], torch.linalg.qr(Zt.double())[0]
    bound = 4 * float((q32.double() - q64).abs().max())
    U = shw.stiefel_frames(dev(Z))
    assert U.dtype == torch.float32 and tuple(U.shape) == Z.shape
    U = U.cpu().numpy().astype(np.float64)
    gram = np.einsum("ldj,ldk->ljk", U, U) - np.eye(2)
    print(f"d={d}: frames vs LAPACK {np.abs(U - U_ref).max():.2e}, orthonormal to {np.abs(gram).max():.2e} (bound {bound:.2e})")
    assert np.abs(U - U_ref).max() <= bound
    assert np.abs(gram).max() <= bound


def test_g15_rng_case_and_generator_consumption(shw, g15):
    g = g15
    x, y = dev(g["rng_x"]), dev(g["rng_y"])
    U = shw.stiefel_frames(dev(g["rng_Z"]))                   # the Z the reference drew, through the frames kernel
    assert rel(shw.sliced_cost(x, y, U, p=2).item(), g["rng_val"]) < 1e-5
    # the public entries draw (L, d, 2) resp. (B, L, d, 2) from the global generator and then are sliced_cost
    torch.manual_seed(7)
    v1 = shw.sliced_wasserstein_sphere(x, y, 16, "cuda")
    torch.manual_seed(7)
    Ud = shw.draw_directions(16, "cuda", d=8)
    assert tuple(Ud.shape) == (16, 8, 2) and v1.dim() == 0
    assert v1.item() == shw.sliced_cost(x, y, Ud, p=2).item()
    xb, yb = torch.stack([x, y]), torch.stack([y, x])
    torch.manual_seed(7)
    v2 = shw.sliced_wasserstein_sphere_fast(xb, yb, 16, "cuda")
    torch.manual_seed(7)
    Ub = shw.draw_directions(16, "cuda", batch=2, d=8)
    assert tuple(v2.shape) == (1,) and v2.item() == shw.sliced_cost(xb, yb, Ub, p=2).item()


# ------------------------------------------------------------------------------ coordinates kernel at its edges
def circular(a, b):
    dd = np.abs(np.asarray(a, dtype=np.float64) - np.asarray(b, dtype=np.float64))
    return np.minimum(dd, 1.0 - dd)


def coords_inputs(d, n, L, shared):
    """B = 2 clouds of unit rows; from n = 63 on point 5 of pair 0 is all zero, and for d >= 3 point 7 of pair 0 is the
    last axis while slice 0 of pair 0 (or of the shared frames) has an exactly zero last row: that point is orthogonal
    to both columns and projects to exactly (0, 0).  (At d = 2 only the zero vector is orthogonal to a frame.)"""
    gen = torch.Generator().manual_seed(1000 * d + 10 * n + L + (5 if shared else 0))
    x = torch.nn.functional.normalize(torch.randn(2, n, d, generator=gen), dim=-1)
    Z = torch.randn(*((L,) if shared else (2, L)), d, 2, generator=gen)
    if d >= 3:
        Z.view(-1, d, 2)[0, d - 1, :] = 0.0
    U = torch.linalg.qr(Z)[0]
    if n >= 63:
        x[0, 5] = 0.0
        if d >= 3:
            assert float(U.view(-1, d, 2)[0, d - 1].abs().max()) == 0.0
            x[0, 7] = 0.0
            x[0, 7, d - 1] = 1.0
    return x, U


@pytest.mark.parametrize("shared", [True, False])
@pytest.mark.parametrize("L", [1, 3])
@pytest.mark.parametrize("n", [1, 63, 65, 257])
@pytest.mark.parametrize("d", [2, 3, 5, 17, 64])
def test_circle_coordinates_against_the_float64_oracle(shw, d, n, L, shared):
    from oracle import ref_mirror
    x, U = coords_inputs(d, n, L, shared)
    ref64 = ref_mirror.circle_coords(x.double(), U.double() if not shared else U.double().unsqueeze(0)).numpy()
    ref32 = ref_mirror.circle_coords(x, U if not shared else U.unsqueeze(0)).numpy()
    bound = 1e-6 + 4 * float(circular(ref32, ref64).max())
    got = shw.circle_coordinates(x.cuda(), U.cuda())
    assert tuple(got.shape) == (2, L, n) and got.dtype == torch.float32
    got = got.cpu().numpy()
    assert np.all((got >= 0.0) & (got <= 1.0))
    assert circular(got, ref64).max() <= bound, (circular(got, ref64).max(), bound)
    if n >= 63:
        assert got[0, :, 5].max() == 0.0                      # an all-zero point lands on coordinate 0
        if d >= 3:
            assert got[0, 0, 7] == 0.0                        # and so does an exactly orthogonal one


def test_circle_coordinates_at_d3_feed_the_circle_level_like_the_sliced_kernels(shw):
    gen = torch.Generator().manual_seed(33)
    x = torch.nn.functional.normalize(torch.randn(2, 300, 3, generator=gen), dim=-1).cuda()
    y = torch.nn.functional.normalize(torch.randn(2, 300, 3, generator=gen), dim=-1).cuda()
    U = torch.linalg.qr(torch.randn(2, 6, 3, 2, generator=gen))[0].cuda()
    _, cost, _ = shw.ssw_pair_losses(x, y, U, p=2, return_slices=True)
    cx, cy = shw.circle_coordinates(x, U), shw.circle_coordinates(y, U)
    rows = shw.binary_search_circle(cx.reshape(12, 300), cy.reshape(12, 300), p=2)
    assert rel(rows.cpu().numpy(), cost.reshape(12).cpu().numpy()) < 2e-5
    single = shw.circle_coordinates(x[0], U[0])               # one cloud, its frames: (L, n)
    assert torch.equal(single, cx[0])


def test_circle_coordinates_rows_past_2_to_the_31_elements(shw):
    """Row offsets are 64-bit: L n > 2^31 output elements (8.6 GB) with frames that repeat with period 64, so every row
    past the 2^31-st element must equal one of the first 64 rows bit for bit (compared on the device)."""
    n, L, period = 8192, 262400, 64
    assert (L - period) * n > 2 ** 31
    gen = torch.Generator().manual_seed(5)
    x = torch.nn.functional.normalize(torch.randn(1, n, 2, generator=gen), dim=-1).cuda()
    U = torch.linalg.qr(torch.randn(period, 2, 2, generator=gen))[0].cuda().repeat(L // period, 1, 1)
    out = shw.circle_coordinates(x, U)[0]
    first = out[:period]
    ref = shw.circle_coordinates(x, U[:period])[0]            # a launch whose offsets fit 32 bits
    assert torch.equal(first, ref)
    for row in (2 ** 31 // n - period, 2 ** 31 // n, L - period):        # up to, across and past 2^31; the last rows
        assert torch.equal(out[row:row + period], first), row
    del out
    torch.cuda.empty_cache()


# ------------------------------------------------------------------------------ whole path against the float64 oracle
SHAPES = {                      # n, m, weights
    "64x64": (64, 64, None),
    "1200x1200": (1200, 1200, None),
    "3000x3000": (3000, 3000, None),
    "256x200": (256, 200, None),
    "128x128_shared_w": (128, 128, "shared"),
    "128x128_pair_w": (128, 128, "pair"),
}
WHOLE = [(s, d, p) for s in SHAPES if s != "3000x3000" for d in (4, 33) for p in (1, 2, 3)] + [("3000x3000", 4, 2)]
B, L = 2, 7
PAIR_W = (0.75, -1.25)          # upstream gradient of the per-pair losses
TOTAL_W = 0.5                   # and of the total


def draw_whole_inputs(shape, d, seed):
    n, m, weights = SHAPES[shape]
    gen = torch.Generator().manual_seed(seed)
    x = torch.nn.functional.normalize(torch.randn(B, n, d, generator=gen), dim=-1)
    y = torch.nn.functional.normalize(torch.randn(B, m, d, generator=gen), dim=-1)
    U = torch.linalg.qr(torch.randn(B, L, d, 2, generator=gen))[0]
    wu = wv = None
    if weights is not None:
        rows = (B,) if weights == "pair" else ()
        wu = torch.rand(*rows, n, generator=gen) + 0.25
        wv = torch.rand(*rows, m, generator=gen) + 0.25
        wu, wv = wu / wu.sum(-1, keepdim=True), wv / wv.sum(-1, keepdim=True)
    return x, y, U, wu, wv


def oracle_pair_values(inputs, p, dtype):
    from oracle import ref_mirror
    x, y, U, wu, wv = inputs
    vals = []
    for b in range(B):
        a = None if wu is None else (wu[b] if wu.dim() == 2 else wu).to(dtype)
        c = None if wv is None else (wv[b] if wv.dim() == 2 else wv).to(dtype)
        vals.append(ref_mirror.sliced_cost(x[b].to(dtype), y[b].to(dtype), U[b].to(dtype), p, a, c))
    return torch.stack(vals)


# Seeds of the whole-path inputs, fixed: 7000 + 13 d + n + 3 m, except where noted.
WHOLE_SEEDS = {(shape, d): 7000 + 13 * d + SHAPES[shape][0] + 3 * SHAPES[shape][1]
               for shape in SHAPES for d in (4, 33) if (shape, d) != ("3000x3000", 33)}
# 256x200 at d = 33: at seed 8285 the CPU ORACLE run in float32 is 1.3e-5 (p = 3) and 5.1e-6 (p = 2) from its own float64
# run, and so is a float64 solve on float32 coordinates: with 14 slices a pair's loss is small where both clouds project
# nearly uniformly, and one ill-conditioned slice moves it.  That draw cannot hold a float32 kernel to 1e-5, so the next
# seed of the sequence (+ 100000) is used.  Chosen from CPU oracle results alone, as the seeds of fixture G15.
WHOLE_SEEDS[("256x200", 33)] += 100000
ORACLE_GAP = 2.5e-6             # float32 oracle against float64 oracle on the inputs above: a quarter of the tolerance
                                # (measured: at most 5.0e-7 over all cases)


@functools.lru_cache(maxsize=None)
def whole_inputs(shape, d):
    """Seeded inputs of one (shape, d), the same for every p."""
    return draw_whole_inputs(shape, d, WHOLE_SEEDS[(shape, d)])


@functools.lru_cache(maxsize=None)
def whole_oracle(shape, d, p):
    """Per-pair values and the gradients of sum_b PAIR_W[b] v_b + TOTAL_W sum_b v_b, float64, computed once per case."""
    x, y, U, wu, wv = whole_inputs(shape, d)
    xs, ys = x.double().requires_grad_(True), y.double().requires_grad_(True)
    vals = oracle_pair_values((xs, ys, U, wu, wv), p, torch.float64)
    ((vals * torch.tensor(PAIR_W, dtype=torch.float64)).sum() + TOTAL_W * vals.sum()).backward()
    return vals.detach().numpy(), xs.grad.numpy(), ys.grad.numpy()


@pytest.mark.parametrize("shape,d,p", WHOLE)
def test_whole_path_values_gradients_determinism(shw, shape, d, p):
    x, y, U, wu, wv = whole_inputs(shape, d)
    ref_vals, ref_gx, ref_gy = whole_oracle(shape, d, p)
    # the inputs are well conditioned for float32: the oracle's own float32 run stays within ORACLE_GAP
    assert rel(oracle_pair_values((x, y, U, wu, wv), p, torch.float32).numpy(), ref_vals) <= ORACLE_GAP
    Ud = U.cuda()
    wud, wvd = (None if wu is None else wu.cuda()), (None if wv is None else wv.cuda())
    grads = []
    for _run in range(2):
        xs, ys = x.cuda().requires_grad_(True), y.cuda().requires_grad_(True)
        pair, total = shw.ssw_pair_losses(xs, ys, Ud, p=p, u_weights=wud, v_weights=wvd, return_total=True)
        assert tuple(pair.shape) == (B,) and tuple(total.shape) == (1,)
        ((pair * torch.tensor(PAIR_W, device="cuda")).sum() + TOTAL_W * total.sum()).backward()
        grads.append((xs.grad.clone(), ys.grad.clone()))
    print(f"{shape} d={d} p={p}: pair rel {rel(pair.detach().cpu().numpy(), ref_vals):.2e}")
    assert rel(pair.detach().cpu().numpy(), ref_vals) < 1e-5
    assert rel(total.item(), ref_vals.sum()) < 1e-5
    assert tuple(grads[0][0].shape) == (B, x.shape[1], d) and tuple(grads[0][1].shape) == (B, y.shape[1], d)
    grad_close(grads[0][0].cpu().numpy(), ref_gx)
    grad_close(grads[0][1].cpu().numpy(), ref_gy)
    assert torch.equal(grads[0][0], grads[1][0]) and torch.equal(grads[0][1], grads[1][1])   # bit-identical runs


def test_no_grad_allocates_no_coefficient_scratch(shw, monkeypatch):
    x, y, U, _, _ = whole_inputs("64x64", 4)
    xs, ys, Ud = x.cuda().requires_grad_(True), y.cuda().requires_grad_(True), U.cuda()
    leases = []
    lease = shw.ssw.SSWWorkspace.lease

    def spy(*args, **kwargs):
        ws = lease(*args, **kwargs)
        leases.append(ws)
        return ws
    monkeypatch.setattr(shw.ssw.SSWWorkspace, "lease", staticmethod(spy))
    with torch.no_grad():
        quiet = shw.ssw_pair_losses(xs, ys, Ud, p=2)
    assert len(leases) == 1 and leases[0].coef_s is None and leases[0].coef_t is None
    assert not quiet.requires_grad
    loud = shw.ssw_pair_losses(xs, ys, Ud, p=2)
    assert len(leases) == 2 and leases[1].coef_s is not None and loud.requires_grad
    assert rel(quiet.cpu().numpy(), loud.detach().cpu().numpy()) < 1e-6


# ------------------------------------------------------------------------------ limits
@pytest.mark.parametrize("d", [1, 65])
def test_point_dimension_outside_2_to_64_is_a_value_error(shw, d):
    x = torch.zeros(1, 8, d, device="cuda")
    U = torch.zeros(2, d, 2, device="cuda")
    with pytest.raises(ValueError, match=r"2\.\.64"):
        shw.ssw_pair_losses(x, x, U)
    with pytest.raises(ValueError, match=r"2\.\.64"):
        shw.sliced_cost(x[0], x[0], U)


def test_float64_at_d5_says_the_generic_path_is_float32(shw):
    x = torch.zeros(1, 8, 5, device="cuda", dtype=torch.float64)
    U = torch.zeros(2, 5, 2, device="cuda", dtype=torch.float64)
    with pytest.raises(ValueError, match="D-generic path.*float32"):
        shw.ssw_pair_losses(x, x, U)


def test_dimension_mismatch_between_clouds_and_frames_is_named(shw):
    x = torch.zeros(1, 8, 5, device="cuda")
    with pytest.raises(ValueError, match="point dimension mismatch"):
        shw.ssw_pair_losses(x, x, torch.zeros(2, 6, 2, device="cuda"))
    with pytest.raises(ValueError, match="point dimension mismatch"):
        shw.ssw_pair_losses(x, torch.zeros(1, 8, 3, device="cuda"), torch.zeros(2, 5, 2, device="cuda"))


@pytest.mark.parametrize("d", [2, 5])
def test_chamfer_and_sinkhorn_still_refuse_clouds_that_are_not_r3(shw, d):
    """Their kernels know 3 coordinates per point only: only the spherical sliced-W functions gained the D-generic check."""
    x = torch.zeros(1, 8, d, device="cuda")
    ok = torch.zeros(1, 8, 3, device="cuda")
    for a, b in ((x, x), (ok, x), (x, ok)):
        with pytest.raises(ValueError, match="3 coordinates per point"):
            shw.chamfer_pair_losses(a, b)
        with pytest.raises(ValueError, match="3 coordinates per point"):
            shw.chamfer_distance(a, b)
        with pytest.raises(ValueError, match="3 coordinates per point"):
            shw.sinkhorn_pair_costs(a, b, 0.01, 5)
        with pytest.raises(ValueError, match="3 coordinates per point"):
            shw.log_Sinkhorn_Distance_Loss(eps=0.01, max_iter=5)(a, b, "cuda")
