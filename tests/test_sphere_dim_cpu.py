"""CPU checks of the D-generic spherical sliced-W path (points on S^(d-1), 2 <= d <= 64; csrc/shw_ssw_dim.hip).

* Fixture G15 (tools/make_golden_sphere_dim.py: the real reference at d != 3) is pinned to the oracle:
  `oracle.ref_mirror` in float64 reproduces every float64 value and per-slice array to 1e-12 relative and every
  float64 gradient to 1e-10 of its largest entry.  The oracle is dimension-blind (`circle_coords` is an einsum).
* The new C entries are declared, bound and exported, and refuse a point dimension outside 2..64 and clouds beyond the
  circle level's limits (8192 points; 4096 with weights or n != m at p != 1) before any HIP call (no GPU needed).
"""
import ctypes
import os

import numpy as np
import pytest
import torch

NEW = ("shw_max_point_dim", "shw_stiefel_frames_dim", "shw_ssw_coords_dim", "shw_ssw_dim_workspace_bytes",
       "shw_ssw_forward_dim", "shw_ssw_backward_points_dim")
PAIR_CASES = (("d2_n64_m64_L8u", (1, 2)), ("d8_n256_m256_L16u", (1, 2, 3)), ("d6_n200_m256_L8u", (1, 2)),
              ("d16_n128_m128_L8w", (2,)), ("d64_n100_m100_L8u", (2,)))


@pytest.fixture(scope="module")
def shw():
    import shw_amd
    if not os.path.exists(shw_amd._lib.LIB_PATH):
        shw_amd._lib.build()
    return shw_amd


@pytest.fixture(scope="module")
def g15(golden):
    return golden("g15_sphere_dim.npz")


def t64(a):
    return torch.from_numpy(np.asarray(a, dtype=np.float64))


# ------------------------------------------------------------------------------------------ G15 pinned to the oracle
@pytest.mark.parametrize("tag,p", [(tag, p) for tag, powers in PAIR_CASES for p in powers])
def test_oracle_reproduces_g15_pair_cases_in_float64(g15, tag, p):
    from oracle import ref_mirror
    g = g15
    assert g[f"x_{tag}"].dtype == g[f"U_{tag}"].dtype == np.float32
    x, y = t64(g[f"x_{tag}"]).requires_grad_(True), t64(g[f"y_{tag}"]).requires_grad_(True)
    U = t64(g[f"U_{tag}"])
    wu = t64(g[f"wu_{tag}"]) if tag.endswith("w") else None
    wv = t64(g[f"wv_{tag}"]) if tag.endswith("w") else None
    slices = ref_mirror.per_slice_costs(x, y, U, p, wu, wv)
    val = slices.mean()
    val.backward()
    ref_val, ref_slices = g[f"val64_{tag}_p{p}"], g[f"slices64_{tag}_p{p}"]
    assert abs(val.item() - ref_val) <= 1e-12 * abs(ref_val)
    assert np.abs(slices.detach().numpy() - ref_slices).max() <= 1e-12 * np.abs(ref_slices).max()
    for got, name in ((x.grad, "gx64"), (y.grad, "gy64")):
        ref = g[f"{name}_{tag}_p{p}"]
        assert np.abs(got.numpy() - ref).max() <= 1e-10 * np.abs(ref).max(), name


def test_oracle_reproduces_g15_batched_and_rng_values(g15, shw):
    from oracle import ref_mirror
    g = g15
    x, y, U = t64(g["batched_x"]), t64(g["batched_y"]), t64(g["batched_U"])
    total = ref_mirror.sliced_cost_batched(x, y, U, p=2)
    assert abs(total.item() - g["batched_total64"][0]) <= 1e-12 * g["batched_total64"][0]
    first = ref_mirror.sliced_cost(x[0], y[0], U[0], p=2)
    assert abs(first.item() - g["batched_first64"]) <= 1e-12 * g["batched_first64"]
    val = ref_mirror.sliced_cost(t64(g["rng_x"]), t64(g["rng_y"]), t64(g["rng_U"]), p=2)
    assert abs(val.item() - g["rng_val64"]) <= 1e-12 * g["rng_val64"]
    # the generator is consumed as the reference consumes it at d = 8: one randn of (L, d, 2), then the reduced QR (CPU
    # tensors go through torch.linalg.qr).  Compared with the same calls made here, not bit for bit with the stored U:
    # LAPACK's float32 result differs in the last bits between CPUs.
    torch.manual_seed(int(g["rng_seed"]))
    Z = torch.randn((16, 8, 2))
    state = torch.get_rng_state()
    torch.manual_seed(int(g["rng_seed"]))
    U = shw.draw_directions(16, "cpu", d=8)
    assert torch.equal(torch.get_rng_state(), state) and torch.equal(U, torch.linalg.qr(Z)[0])
    assert np.abs(torch.linalg.qr(torch.from_numpy(g["rng_Z"]))[0].numpy() - g["rng_U"]).max() < 1e-6


def test_g15_holds_arrays_only_and_stays_at_its_size(g15):
    """563 KB: 140 KB of float32 inputs and 422 KB of gradients in two precisions that do not compress
    (tools/make_golden_sphere_dim.py); pinned so that it does not grow."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    assert os.path.getsize(os.path.join(root, "tests", "golden", "g15_sphere_dim.npz")) <= 570 * 1000
    for key in g15.files:
        assert g15[key].dtype in (np.float32, np.float64, np.int64), key
        if key.startswith(("x_", "y_", "U_", "wu_", "wv_", "batched_x", "batched_y", "batched_U", "rng_x", "rng_y",
                           "rng_Z", "frames_Z")):
            assert g15[key].dtype == np.float32, key


def test_g15_records_the_reference_s_own_swap_counts(g15):
    """The allowance of the GPU test (one swapped pair, 2 d entries, per gradient) is met by the reference's own float32
    run against its float64 run: recomputed here from the stored gradients."""
    for tag, powers in PAIR_CASES:
        d = int(tag[1:tag.index("_")])
        for p in powers:
            counts = []
            for name in ("gx", "gy"):
                g32, g64 = g15[f"{name}_{tag}_p{p}"].astype(np.float64), g15[f"{name}64_{tag}_p{p}"]
                counts.append(int((np.abs(g32 - g64) > 2e-4 * np.abs(g64).max()).sum()))
            assert counts == list(g15[f"swap_{tag}_p{p}"]) and max(counts) <= 2 * d, (tag, p, counts)


# ------------------------------------------------------------------------------------------ the C entries, no GPU
def test_new_entries_are_declared_bound_and_exported(shw):
    from test_capi_cpu import declared_symbols
    lib = shw._lib.load()
    for name in NEW:
        assert name in declared_symbols(), name
        assert name in shw._lib.EXPORTED_SYMBOLS, name
        assert hasattr(lib, name), name
    assert lib.shw_abi_version() == shw._lib.ABI_VERSION == 3
    assert lib.shw_max_point_dim() == 64
    assert lib.shw_ssw_dim_workspace_bytes(2, 10, 20, 3) == 4 * 2 * 3 * 30


def _bufs(k):
    # distinct non-null host addresses: the entries must refuse before they dereference or launch anything
    keep = [ctypes.create_string_buffer(16) for _ in range(k)]
    return keep, [ctypes.addressof(b) for b in keep]


def _calls(lib, ptrs, dim, n, weighted):
    """Every new entry that takes sizes, with `ptrs` = 10 pointers (all None: the issue's form)."""
    xs, xt, U, ws, cost, cs, ct, gx, gy, w = ptrs
    wu = w if weighted else None
    return (
        lib.shw_stiefel_frames_dim(xs, 4, dim, gx, None) if n == 8 else 1,
        lib.shw_ssw_coords_dim(xs, U, 1, n, dim, 4, 0, ws, None) if not weighted else 1,
        lib.shw_ssw_forward_dim(xs, xt, U, wu, None, 0, 0, 1, n, n, dim, 4, 0, 2.0, ws, cost, None, cs, ct, None),
        lib.shw_ssw_forward_dim(xs, xt, U, wu, None, 0, 0, 1, 8, n, dim, 4, 0, 2.0, ws, cost, None, None, None, None),
        lib.shw_ssw_backward_points_dim(xs, xt, U, cs, ct, 1, n, n, dim, 4, 0, 0.25, None, None, gx, gy, None)
        if not weighted else 1,
    )


@pytest.mark.parametrize("dim,n,weighted", [(1, 8, False), (65, 8, False), (5, 8193, False), (5, 4097, True)])
@pytest.mark.parametrize("null", [True, False])
def test_dimension_and_size_limits_return_1_without_a_gpu(shw, dim, n, weighted, null):
    lib = shw._lib.load()
    keep, ptrs = _bufs(10)
    assert _calls(lib, [None] * 10 if null else ptrs, dim, n, weighted) == (1, 1, 1, 1, 1)


def test_unequal_sizes_at_p_not_1_take_the_4096_limit(shw):
    lib = shw._lib.load()
    _keep, (xs, xt, U, ws, cost) = _bufs(5)
    assert lib.shw_ssw_forward_dim(xs, xt, U, None, None, 0, 0, 1, 4097, 4000, 5, 4, 0, 2.0, ws, cost, None, None, None,
                                   None) == 1
    # null pointers, short frame strides and p < 1 are refused as well
    assert lib.shw_ssw_forward_dim(xs, xt, None, None, None, 0, 0, 1, 8, 8, 5, 4, 0, 2.0, ws, cost, None, None, None, None) == 1
    assert lib.shw_ssw_forward_dim(xs, xt, U, None, None, 0, 0, 1, 8, 8, 5, 4, 0, 2.0, None, cost, None, None, None, None) == 1
    assert lib.shw_ssw_forward_dim(xs, xt, U, None, None, 0, 0, 2, 8, 8, 5, 4, 4 * 5 * 2 - 1, 2.0, ws, cost, None, None, None,
                                   None) == 1
    assert lib.shw_ssw_forward_dim(xs, xt, U, None, None, 0, 0, 1, 8, 8, 5, 4, 0, 0.5, ws, cost, None, None, None, None) == 1
    assert lib.shw_ssw_coords_dim(xs, U, 2, 8, 5, 4, 4 * 5 * 2 - 1, ws, None) == 1


def test_cpu_clouds_of_any_dimension_are_refused_not_silently_computed(shw):
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        shw.sliced_cost(torch.zeros(8, 5), torch.zeros(8, 5), torch.zeros(2, 5, 2))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        shw.circle_coordinates(torch.zeros(1, 8, 5), torch.zeros(2, 5, 2))
