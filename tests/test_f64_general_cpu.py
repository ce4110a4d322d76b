"""CPU checks of the general float64 path's boundary, of the definition it is tested against and of fixture G14 (no GPU
needed).

The header declares the four general float64 entries and the library exports them; each refuses bad arguments before any
HIP call; the switch is off by default.  The two minimisers of tests/helpers/circle_general_exact.py agree.  Fixture G14
(the REAL reference in double on unequal-size and weighted clouds, tools/make_golden_f64_general.py) is reproduced by
`oracle/ref_mirror` in double, and the gaps between the reference and the definition that the fixture stores -- from
which the GPU test takes its gradient bound -- are recomputed here.  What the GPU file relies on for its own inputs is
asserted here too: every slice of its gradient cases has an isolated minimiser, its gradcheck inputs keep their margins,
and the rounding spread S it adds to its cost bound is measured."""
import os
import re

import numpy as np
import pytest
import torch

from helpers import circle_general_exact as exact
from helpers import f64_general_cases as cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("shw_max_points_f64_general", "shw_ssw_forward_general_f64", "shw_ssw_backward_points_general_f64",
           "shw_circle_ot_general_f64")
G14_SLICED = (("n256_m200_L16w", True, (1, 2, 3), True), ("n256_m200_L8u", False, (1, 2), False),
              ("n1200_m1000_L4w", True, (2,), False))
G14_GRAD_BOUND = 1.396e-05          # ten times the worst gap measured when the fixture was made (its generator's docstring)
F64 = torch.float64


@pytest.fixture(scope="module")
def shw():
    import shw_amd
    if not os.path.exists(shw_amd._lib.LIB_PATH):
        shw_amd._lib.build()
    return shw_amd


# ------------------------------------------------------------------------------------------------ the boundary
def test_header_declares_and_library_exports_the_entries(shw):
    text = open(os.path.join(ROOT, "include", "shw.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(shw_[a-z0-9_]+)\s*\(", text))
    assert set(ENTRIES) <= declared
    assert re.search(r"#define\s+SHW_ABI_VERSION\s+3\b", text)          # additive: the ABI number stays
    lib = shw._lib.load()
    for name in ENTRIES:
        assert name in shw._lib.EXPORTED_SYMBOLS and hasattr(lib, name), name
    assert lib.shw_max_points_f64_general() >= 2048
    assert shw.max_points_f64_general() == lib.shw_max_points_f64_general()


def test_entries_refuse_bad_arguments_without_a_gpu(shw):
    lib = shw._lib.load()
    fake, limit = 4096, lib.shw_max_points_f64_general()
    fwd, bwd, circ = lib.shw_ssw_forward_general_f64, lib.shw_ssw_backward_points_general_f64, lib.shw_circle_ot_general_f64
    # NULL pointers
    assert fwd(None, None, None, None, None, 0, 0, 1, 8, 9, 1, 0, 2.0, None, None, None, None, None) == 1
    assert fwd(fake, fake, fake, None, None, 0, 0, 1, 8, 9, 1, 0, 2.0, None, None, None, None, None) == 1
    assert bwd(None, None, None, None, None, 1, 8, 9, 1, 0, 1.0, None, None, None, None, None) == 1
    assert bwd(fake, fake, fake, fake, fake, 1, 8, 9, 1, 0, 1.0, None, None, fake, None, None) == 1
    assert circ(None, None, None, None, 0, 0, 1, 8, 9, 2.0, 1, None, None, None, None, None) == 1
    # sizes above the limit (either cloud), no points, p < 1, exactly one coefficient row: the pointers are never read
    assert fwd(fake, fake, fake, None, None, 0, 0, 1, limit + 1, 8, 1, 0, 2.0, fake, None, None, None, None) == 1
    assert fwd(fake, fake, fake, None, None, 0, 0, 1, 8, limit + 1, 1, 0, 2.0, fake, None, None, None, None) == 1
    assert fwd(fake, fake, fake, None, None, 0, 0, 1, 0, 8, 1, 0, 2.0, fake, None, None, None, None) == 1
    assert fwd(fake, fake, fake, None, None, 0, 0, 1, 8, 9, 1, 0, 0.5, fake, None, None, None, None) == 1
    assert fwd(fake, fake, fake, None, None, 0, 0, 1, 8, 9, 1, 0, float("nan"), fake, None, None, None, None) == 1
    assert fwd(fake, fake, fake, None, None, 0, 0, 1, 8, 9, 1, 0, 2.0, fake, None, fake, None, None) == 1
    assert fwd(fake, fake, fake, None, None, 0, 0, 1, 8, 9, 1, 0, 2.0, fake, None, None, fake, None) == 1
    assert fwd(fake, fake, fake, None, None, 0, 0, 1, 8, 9, 4, 6, 2.0, fake, None, None, None, None) == 1      # short direction stride
    assert bwd(fake, fake, fake, fake, fake, 1, limit + 1, 9, 1, 0, 1.0, None, None, fake, fake, None) == 1
    assert bwd(fake, fake, fake, fake, fake, 1, 8, limit + 1, 1, 0, 1.0, None, None, fake, fake, None) == 1
    assert circ(fake, fake, None, None, 0, 0, 1, limit + 1, 9, 2.0, 1, fake, None, None, None, None) == 1
    assert circ(fake, fake, None, None, 0, 0, 1, 8, limit + 1, 2.0, 1, fake, None, None, None, None) == 1
    assert circ(fake, fake, None, None, 0, 0, 1, 8, 9, 0.5, 1, fake, None, None, None, None) == 1
    assert circ(fake, fake, None, None, 0, 0, 1, 8, 9, 2.0, 2, fake, None, None, None, None) == 1             # level median needs p = 1
    assert circ(fake, fake, None, None, 0, 0, 1, 8, 9, 2.0, 7, fake, None, None, None, None) == 1             # no such method
    assert circ(fake, fake, None, None, 0, 0, 1, 8, 9, 2.0, 1, fake, None, fake, None, None) == 1
    # nothing to do: success without a launch
    assert fwd(fake, fake, fake, None, None, 0, 0, 0, 8, 9, 1, 0, 2.0, fake, None, None, None, None) == 0
    assert circ(fake, fake, None, None, 0, 0, 0, 8, 9, 2.0, 1, fake, None, None, None, None) == 0


def test_switch_is_off_by_default_and_returns_the_previous_setting(shw):
    start = os.environ.get("SHW_FLOAT64_GENERAL", "0") == "1"        # the one way to start a process with it on
    assert shw.float64_general_enabled() is start
    assert shw.enable_float64_general() is start and shw.float64_general_enabled() is True
    assert shw.enable_float64_general(False) is True and shw.float64_general_enabled() is False
    assert shw.enable_float64_general(start) is False


def test_cpu_double_tensors_are_refused_not_silently_computed(shw):
    x, y = torch.zeros(8, 3, dtype=F64), torch.zeros(6, 3, dtype=F64)
    U = torch.zeros(2, 3, 2, dtype=F64)
    before = shw.enable_float64(True), shw.enable_float64_general(True)
    try:
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            shw.sliced_cost(x, y, U)
        with pytest.raises(TypeError, match="no CPU fallback"):
            shw.binary_search_circle(torch.zeros(2, 8, dtype=F64), torch.zeros(2, 6, dtype=F64), p=2)
    finally:
        shw.enable_float64(before[0])
        shw.enable_float64_general(before[1])


# ------------------------------------------------------------------------------------------------ the definition
@pytest.mark.parametrize("n,m,weighted,p", [(7, 5, False, 2), (33, 20, True, 2), (64, 48, True, 3), (40, 40, True, 1)])
def test_the_two_minimisers_agree(n, m, weighted, p):
    g = torch.Generator().manual_seed(14050 + n)
    u, v = torch.rand(6, n, generator=g, dtype=F64), torch.rand(6, m, generator=g, dtype=F64)
    wu = cases.weights(g, n) if weighted else None
    wv = cases.weights(g, m) if weighted else None
    args = exact.sorted_cdfs(u, v, wu, wv)
    rounds = []
    a, _ = exact.min_exhaustive(*args, p)
    b, _ = exact.min_certificate(*args, p, rounds_out=rounds)
    print(f"{n} x {m} p={p}: |exhaustive - certificate| max {(a - b).abs().max().item():.2e}, {rounds[0]} rounds")
    assert bool(((a - b).abs() <= 1e-15 * a + 1e-17).all())


# ------------------------------------------------------------------------------------------------ fixture G14
def test_g14_is_double_and_not_float32_representable(golden):
    g = golden("g14_f64_general.npz")
    for key in g.files:
        assert g[key].dtype == np.float64, key
    inputs = [k for k in g.files if k.split("_")[0] in ("x", "y", "U", "u", "v", "wu", "wv")]
    assert len(inputs) == 17
    for key in inputs:
        assert not np.array_equal(g[key], g[key].astype(np.float32).astype(np.float64)), key
    for tag, _, _, _ in G14_SLICED:
        assert np.abs(np.linalg.norm(g[f"x_{tag}"], axis=-1) - 1).max() < 1e-15
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "g14_f64_general.npz")) < 200 * 1000


def g14_case(g, tag, weighted):
    x, y, U = (torch.from_numpy(g[f"{k}_{tag}"]) for k in ("x", "y", "U"))
    wu = torch.from_numpy(g[f"wu_{tag}"]) if weighted else None
    wv = torch.from_numpy(g[f"wv_{tag}"]) if weighted else None
    return x, y, U, wu, wv


def rel(got, want):
    return np.abs(np.asarray(got) - want).max() / np.abs(want).max()


def reference_projection(X, U):
    """Circle coordinates in the arithmetic the reference uses: a matrix product per slice, then normalize and atan2
    (:270-279).  `ref_mirror.circle_coords` states the same projection as an einsum, whose sums round in another order:
    its coordinates differ from these by an ulp on some atoms."""
    planar = torch.matmul(torch.transpose(U, 1, 2)[:, None], X[:, :, None]).reshape(U.shape[0], X.shape[0], 2)
    planar = torch.nn.functional.normalize(planar, p=2, dim=-1)
    return (torch.atan2(-planar[:, :, 1], -planar[:, :, 0]) + np.pi) / (2 * np.pi)


def mirror_on_g14(g, tag, weighted, p, projection):
    """-> the mirror's per-slice costs, value and gradients on a G14 case, the coordinates from `projection`."""
    from oracle import ref_mirror
    x, y, U, wu, wv = g14_case(g, tag, weighted)
    xs, ys = x.clone().requires_grad_(True), y.clone().requires_grad_(True)
    cu, cv = projection(xs, U), projection(ys, U)
    if p == 1:
        slices = ref_mirror.circular_w1_level_median(cu, cv, wu, wv)
    else:
        slices = ref_mirror.circular_ot_bisect(cu, cv, p=p, u_weights=wu, v_weights=wv)
    val = slices.mean()
    val.backward()
    assert val.dtype == F64
    return slices.detach().numpy(), val.item(), xs.grad.numpy(), ys.grad.numpy()


@pytest.mark.parametrize("tag,weighted,powers,with_gy", G14_SLICED)
def test_ref_mirror_in_double_reproduces_g14(golden, tag, weighted, powers, with_gy):
    """Every G14 value, per-slice cost and gradient within 1e-15 relative (largest difference over largest entry) of the
    mirror's circle routines (`circular_ot_bisect` with `cut_cost` / `cut_slopes`, `circular_w1_level_median`: what the
    definition in helpers/circle_general_exact.py is built from) and their autograd, on coordinates projected in the
    reference's arithmetic.  Measured: 0.0 on every quantity -- the mirror follows the reference bit for bit."""
    g = golden("g14_f64_general.npz")
    for p in powers:
        slices, val, gx, gy = mirror_on_g14(g, tag, weighted, p, reference_projection)
        assert rel(slices, g[f"slices_{tag}_p{p}"]) <= 1e-15, (tag, p)
        assert abs(val - float(g[f"val_{tag}_p{p}"])) <= 1e-15 * abs(val)
        assert rel(gx, g[f"gx_{tag}_p{p}"]) <= 1e-15, (tag, p)
        if with_gy:
            assert rel(gy, g[f"gy_{tag}_p{p}"]) <= 1e-15, (tag, p)


@pytest.mark.parametrize("tag,weighted,powers,with_gy", G14_SLICED)
def test_ref_mirror_with_its_own_projection_stays_at_rounding_level_of_g14(golden, tag, weighted, powers, with_gy):
    """The same through `ref_mirror.circle_coords`, the projection the definition uses at the sliced level.  Its
    coordinates differ from the reference's by an ulp (1.1e-16), which no comparison of gradients survives at 1e-15: a
    coefficient p |D|^(p-1) sgn D moves by (p - 1) ulp / |D| relative, and differences D between matched atoms go down to
    1e-5 at these sizes.  Bounds: 1e-13 on values and per-slice costs (an ulp of a coordinate against costs of 1e-3), 1e-11
    on gradients (an ulp against |D| = 1e-5) -- the bounds test_f64_cpu.py holds the mirror to on G12 for the same reason.
    Measured: values <= 2.1e-16, per-slice costs <= 5.4e-16, gradients 4.7e-16 ... 1.4e-14 (n1200_m1000_L4w, p = 2)."""
    from oracle import ref_mirror
    g = golden("g14_f64_general.npz")
    for p in powers:
        slices, val, gx, gy = mirror_on_g14(g, tag, weighted, p, ref_mirror.circle_coords)
        print(f"G14 {tag} p={p}: own projection, slices {rel(slices, g[f'slices_{tag}_p{p}']):.1e} "
              f"gx {rel(gx, g[f'gx_{tag}_p{p}']):.1e}" + (f" gy {rel(gy, g[f'gy_{tag}_p{p}']):.1e}" if with_gy else ""))
        assert rel(slices, g[f"slices_{tag}_p{p}"]) <= 1e-13, (tag, p)
        assert abs(val - float(g[f"val_{tag}_p{p}"])) <= 1e-13 * abs(val)
        assert rel(gx, g[f"gx_{tag}_p{p}"]) <= 1e-11, (tag, p)
        if with_gy:
            assert rel(gy, g[f"gy_{tag}_p{p}"]) <= 1e-11, (tag, p)


def test_ref_mirror_in_double_reproduces_the_g14_circle_rows(golden):
    from oracle import ref_mirror
    g = golden("g14_f64_general.npz")
    u, v = torch.from_numpy(g["u_rows"]), torch.from_numpy(g["v_rows"])
    for tag, wu, wv in (("rows_w", torch.from_numpy(g["wu_rows"]), torch.from_numpy(g["wv_rows"])), ("rows_u", None, None)):
        for p in (1, 2, 3):
            got = ref_mirror.circular_ot_bisect(u, v, p=p, u_weights=wu, v_weights=wv)
            assert rel(got.numpy(), g[f"bsc_p{p}_{tag}"]) <= 1e-15, (tag, p)
        assert rel(ref_mirror.circular_w1_level_median(u, v, wu, wv).numpy(), g[f"emd1_{tag}"]) <= 1e-15, tag


@pytest.mark.parametrize("tag,weighted,powers,with_gy", G14_SLICED)
def test_g14_gaps_to_the_definition_are_what_the_generator_recorded(golden, tag, weighted, powers, with_gy):
    """The kernels implement the minimum over the cut; the reference bisects and stops off the kink.  The GPU test bounds
    the G14 gradients by ten times the worst gap between the definition's gradient and the fixture's: recompute it."""
    g = golden("g14_f64_general.npz")
    assert 10 * float(g["grad_gap_worst"]) <= G14_GRAD_BOUND
    x, y, U, wu, wv = g14_case(g, tag, weighted)
    for p in powers:
        if p == 1:
            continue
        xe, ye = x.clone().requires_grad_(True), y.clone().requires_grad_(True)
        cost, iso = exact.slice_costs(xe, ye, U, p, wu, wv)
        assert bool(iso.all())
        cost.mean().backward()
        gaps = [rel(xe.grad.numpy(), g[f"gx_{tag}_p{p}"])]
        if with_gy:
            gaps.append(rel(ye.grad.numpy(), g[f"gy_{tag}_p{p}"]))
        print(f"G14 {tag} p={p}: gradient gaps {gaps}, stored {g[f'grad_gap_{tag}_p{p}']}")
        assert np.allclose(gaps, g[f"grad_gap_{tag}_p{p}"], rtol=1e-6, atol=1e-15)
        assert max(gaps) <= float(g["grad_gap_worst"])
        d = g[f"slices_{tag}_p{p}"] - cost.detach().numpy()
        assert np.allclose([d.min(), d.max()], g[f"slice_gap_{tag}_p{p}"], rtol=0, atol=1e-18)
        assert np.abs(d).max() <= 1e-9                                           # the issue's bound on G14 slice costs
        assert (-d <= 1e-12 * cost.detach().numpy() + 1e-14).all()               # a minimum cannot exceed a bisection's result


def test_g14_circle_row_gaps_are_what_the_generator_recorded(golden):
    g = golden("g14_f64_general.npz")
    u, v = torch.from_numpy(g["u_rows"]), torch.from_numpy(g["v_rows"])
    for tag, wu, wv in (("rows_w", torch.from_numpy(g["wu_rows"]), torch.from_numpy(g["wv_rows"])), ("rows_u", None, None)):
        for p in (1, 2, 3):
            cost, _, _ = exact.circle_min(u, v, p, wu, wv)
            d = g[f"bsc_p{p}_{tag}"] - cost.numpy()
            assert np.allclose([d.min(), d.max()], g[f"slice_gap_{tag}_p{p}"], rtol=0, atol=1e-18), (tag, p)
            assert np.abs(d).max() <= 1e-9


# ------------------------------------------------------------------------------------------------ the GPU file's inputs
def coordinates(x, y, U, wu, wv):
    from oracle import ref_mirror
    for b in range(x.shape[0]):
        Ub = U if U.dim() == 3 else U[b]
        a = None if wu is None else (wu if wu.dim() == 1 else wu[b])
        c = None if wv is None else (wv if wv.dim() == 1 else wv[b])
        yield ref_mirror.circle_coords(x[b], Ub), ref_mirror.circle_coords(y[b], Ub), a, c


def test_gradient_cases_of_the_gpu_file_leave_out_no_slice():
    for n, m in cases.GRAD_SHAPES:
        for p in cases.POWERS[1:]:
            for mode in cases.modes_for(n, m):
                for cu, cv, wu, wv in coordinates(*cases.case(n, m, p, mode)):
                    assert bool(exact.circle_min(cu, cv, p, wu, wv)[2].all()), (n, m, p, mode)


def test_rounding_spread_of_the_gpu_file_cases():
    spread = 0.0
    todo = [(n, m, False) for n, m in cases.SHAPES] + [(n, m, True) for n, m in cases.MANY]
    for n, m, many in todo:
        for p in cases.POWERS:
            for mode in cases.modes_for(n, m):
                for cu, cv, wu, wv in coordinates(*cases.case(n, m, p, mode, many)):
                    spread = max(spread, exact.rounding_spread(cu, cv, p, wu, wv))
    g = torch.Generator().manual_seed(14200 + 20)                                # the limit case at p = 2
    x, y, U = cases.unit_cloud(g, 1, 2048), cases.unit_cloud(g, 1, 2047), cases.frames(g, 2)
    for cu, cv, wu, wv in coordinates(x, y, U, cases.weights(g, 2048), None):
        spread = max(spread, exact.rounding_spread(cu, cv, 2, wu, wv))
    print(f"rounding spread S = {spread:.3e} (stated {cases.ROUNDING_SPREAD:.1e})")
    assert spread <= cases.ROUNDING_SPREAD


def test_gradcheck_inputs_of_the_gpu_file_keep_their_margins():
    clouds = cases.gradcheck_clouds(cases.GRADCHECK_SEED)
    for p in (1, 2, 3):
        assert cases.gradcheck_margins_ok(*clouds, p)
    rows = cases.gradcheck_rows(cases.GRADCHECK_ROWS_SEED)
    assert cases.gradcheck_rows_margins_ok(*rows, 2) and cases.gradcheck_rows_margins_ok(*rows, 1)
