"""CPU checks of the float64 path's boundary and of fixture G12 (no GPU needed).

The header declares the six float64 entries and the library exports them; each refuses null pointers and unsupported
sizes before any HIP call; the float64 point limit is at least 4096.  Fixture G12 (the REAL reference in double,
tools/make_golden_f64.py) is reproduced by `oracle/ref_mirror` in double -- this pins the fixture to the oracle the way
test_oracle_golden.py does for the others -- and the gradient gap between `oracle/exact_shift` and the fixture, from
which the GPU test takes its bound, is recomputed here."""
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F64_ENTRIES = ("shw_max_points_f64", "shw_stiefel_frames_f64", "shw_ssw_forward_f64", "shw_ssw_backward_points_f64",
               "shw_ssw_reduce_f64", "shw_circle_ot_f64")
G12_CASES = (("n256_L32", (1, 2, 3), True), ("n1200_L8", (1, 2), False))
G12_GRAD_BOUND = 2.54e-13          # ten times the worst gap measured when the fixture was made (its generator's docstring)


@pytest.fixture(scope="module")
def shw():
    import shw_amd
    if not os.path.exists(shw_amd._lib.LIB_PATH):
        shw_amd._lib.build()
    return shw_amd


def test_header_declares_the_float64_entries():
    text = open(os.path.join(ROOT, "include", "shw.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(shw_[a-z0-9_]+)\s*\(", text))
    assert set(F64_ENTRIES) <= declared
    assert re.search(r"#define\s+SHW_ABI_VERSION\s+3\b", text)          # additive: the ABI number stays


def test_library_exports_the_float64_entries(shw):
    lib = shw._lib.load()
    for name in F64_ENTRIES:
        assert name in shw._lib.EXPORTED_SYMBOLS and hasattr(lib, name), name
    assert lib.shw_max_points_f64() >= 4096
    assert shw.ssw.max_points_f64() == lib.shw_max_points_f64()


def test_float64_entries_refuse_bad_arguments_without_a_gpu(shw):
    lib = shw._lib.load()
    assert lib.shw_stiefel_frames_f64(None, 4, None, None) == 1
    assert lib.shw_ssw_forward_f64(None, None, None, 1, 8, 8, 1, 0, 2.0, None, None, None, None, None) == 1
    assert lib.shw_ssw_backward_points_f64(None, None, None, None, None, 1, 8, 8, 1, 0, 1.0, None, None, None, None, None) == 1
    assert lib.shw_ssw_reduce_f64(None, 1, 1, 1.0, None, None, None) == 1
    assert lib.shw_circle_ot_f64(None, None, 1, 8, 8, 2.0, 1, None, None, None, None, None) == 1
    # sizes are checked before any HIP call too: n != m, n above the limit, p < 1 (the pointers are never dereferenced)
    fake = 4096
    limit = lib.shw_max_points_f64()
    assert lib.shw_ssw_forward_f64(fake, fake, fake, 1, 8, 9, 1, 0, 2.0, fake, None, None, None, None) == 1
    assert lib.shw_ssw_forward_f64(fake, fake, fake, 1, limit + 1, limit + 1, 1, 0, 2.0, fake, None, None, None, None) == 1
    assert lib.shw_ssw_forward_f64(fake, fake, fake, 1, 8, 8, 1, 0, 0.5, fake, None, None, None, None) == 1
    assert lib.shw_ssw_forward_f64(fake, fake, fake, 1, 8, 8, 1, 0, 2.0, fake, None, fake, None, None) == 1   # one coefficient row
    assert lib.shw_circle_ot_f64(fake, fake, 1, 8, 9, 2.0, 1, fake, None, None, None, None) == 1
    assert lib.shw_circle_ot_f64(fake, fake, 1, limit + 1, limit + 1, 2.0, 1, fake, None, None, None, None) == 1
    assert lib.shw_circle_ot_f64(fake, fake, 1, 8, 8, 2.0, 2, fake, None, None, None, None) == 1             # level median needs p = 1
    assert lib.shw_ssw_backward_points_f64(fake, fake, fake, fake, fake, 1, 8, 9, 1, 0, 1.0, None, None, fake, fake, None) == 1


def test_cpu_double_tensors_are_refused_not_silently_computed(shw):
    x = torch.zeros(8, 3, dtype=torch.float64)
    U = torch.zeros(2, 3, 2, dtype=torch.float64)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        shw.sliced_cost(x, x, U)


def test_float64_switch_is_off_by_default_and_returns_the_previous_setting(shw):
    start = os.environ.get("SHW_FLOAT64", "0") == "1"        # the one way to start a process with it on
    assert shw.float64_enabled() is start
    assert shw.enable_float64() is start and shw.float64_enabled() is True
    assert shw.enable_float64(False) is True and shw.float64_enabled() is False
    assert shw.enable_float64(start) is False


def test_draw_directions_dtype_on_cpu(shw):
    torch.manual_seed(5)
    U = shw.draw_directions(6, "cpu", dtype=torch.float64)
    torch.manual_seed(5)
    ref = torch.linalg.qr(torch.randn(6, 3, 2, dtype=torch.float64))[0]
    assert U.dtype == torch.float64 and torch.equal(U, ref)
    torch.manual_seed(5)
    assert shw.draw_directions(6, "cpu").dtype == torch.get_default_dtype()


def test_g12_is_double_and_not_float32_representable(golden):
    g = golden("g12_f64.npz")
    for key in g.files:
        assert g[key].dtype == np.float64, key
    for tag, _, _ in G12_CASES:
        x = g[f"x_{tag}"]
        assert not np.array_equal(x, x.astype(np.float32).astype(np.float64))
        assert np.abs(np.linalg.norm(x, axis=-1) - 1).max() < 1e-15
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "g12_f64.npz")) <= 194208


@pytest.mark.parametrize("tag,powers,with_gy", G12_CASES)
def test_ref_mirror_in_double_reproduces_g12(golden, tag, powers, with_gy):
    from oracle import ref_mirror
    g = golden("g12_f64.npz")
    x, y, U = (torch.from_numpy(g[f"{k}_{tag}"]) for k in ("x", "y", "U"))
    for p in powers:
        xs, ys = x.clone().requires_grad_(True), y.clone().requires_grad_(True)
        slices = ref_mirror.per_slice_costs(xs, ys, U, p)
        val = slices.mean()
        val.backward()
        assert val.dtype == torch.float64
        want = g[f"slices_{tag}_p{p}"]
        assert np.abs(slices.detach().numpy() - want).max() <= 1e-13 * np.abs(want).max(), (tag, p)
        assert abs(val.item() - float(g[f"val_{tag}_p{p}"])) <= 1e-13 * abs(val.item())
        gx = g[f"gx_{tag}_p{p}"]
        assert np.abs(xs.grad.numpy() - gx).max() <= 1e-11 * np.abs(gx).max(), (tag, p)
        if with_gy:
            gy = g[f"gy_{tag}_p{p}"]
            assert np.abs(ys.grad.numpy() - gy).max() <= 1e-11 * np.abs(gy).max(), (tag, p)


@pytest.mark.parametrize("tag,powers,with_gy", G12_CASES)
def test_g12_gap_to_the_definition_is_what_the_generator_recorded(golden, tag, powers, with_gy):
    """The kernels implement min_k c(k); the reference bisects.  The GPU test bounds the G12 gradients by ten times the
    worst gap between the exact-shift gradient and the fixture, measured on the CPU: recompute it."""
    from oracle import exact_shift
    g = golden("g12_f64.npz")
    x, y, U = (g[f"{k}_{tag}"] for k in ("x", "y", "U"))
    assert 10 * float(g["grad_gap_worst"]) <= G12_GRAD_BOUND
    for p in powers:
        if p == 1:
            w = [exact_shift.w1_level_median(cu, cv) for cu, cv in zip(exact_shift.circle_coords(x, U),
                                                                       exact_shift.circle_coords(y, U))]
            want = g[f"slices_{tag}_p1"]
            assert np.abs(np.asarray(w) - want).max() <= 1e-12 * np.abs(want).max()
            continue
        ex, ey = exact_shift.ssw_pair_grad(x, y, U, p)
        gaps = [np.abs(ex - g[f"gx_{tag}_p{p}"]).max() / np.abs(g[f"gx_{tag}_p{p}"]).max()]
        if with_gy:
            gaps.append(np.abs(ey - g[f"gy_{tag}_p{p}"]).max() / np.abs(g[f"gy_{tag}_p{p}"]).max())
        assert max(gaps) <= float(g["grad_gap_worst"]) * 1.5 + 1e-15, (tag, p, gaps)
        cost, _ = exact_shift.circular_ot_equal(exact_shift.circle_coords(x, U), exact_shift.circle_coords(y, U), p)
        want = g[f"slices_{tag}_p{p}"]
        assert np.abs(cost - want).max() <= 1e-9                     # the issue's bound on G12 slice costs
        assert (cost - want <= 1e-12 * want + 1e-14).all()           # a minimum cannot exceed what a bisection returns
