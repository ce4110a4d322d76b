"""CPU checks of the D-generic Euclidean sliced-W entries (include/shw.h shw_esw_*_dim): declared, bound, and
rejecting bad sizes and null pointers before any HIP call (no GPU needed)."""
import ctypes
import os

import pytest

NEW = ("shw_esw_forward_dim", "shw_esw_backward_points_dim", "shw_esw_backward_dirs_dim")


@pytest.fixture(scope="module")
def shw():
    import shw_amd
    if not os.path.exists(shw_amd._lib.LIB_PATH):
        shw_amd._lib.build()
    return shw_amd


def test_new_entries_are_declared_bound_and_exported(shw):
    from test_capi_cpu import declared_symbols
    lib = shw._lib.load()
    for name in NEW:
        assert name in declared_symbols(), name
        assert name in shw._lib.EXPORTED_SYMBOLS, name
        assert hasattr(lib, name), name
    assert lib.shw_abi_version() == shw._lib.ABI_VERSION == 3


def _bufs(k):
    # distinct non-null host addresses: the entries must refuse before they dereference or launch anything
    keep = [ctypes.create_string_buffer(16) for _ in range(k)]
    return keep, [ctypes.addressof(b) for b in keep]


@pytest.mark.parametrize("dim,n", [(0, 8), (65, 8), (-1, 8), (6, 4097), (6, 0)])
def test_bad_sizes_are_rejected_without_a_gpu(shw, dim, n):
    lib = shw._lib.load()
    _keep, (xs, xt, th, out, cs, ct, w) = _bufs(7)
    assert lib.shw_esw_forward_dim(xs, xt, th, 1, n, dim, 4, 0, 2.0, out, cs, ct, None) == 1
    assert lib.shw_esw_backward_points_dim(th, cs, ct, w, 1, n, dim, 4, 0, xs, xt, None) == 1
    assert lib.shw_esw_backward_dirs_dim(xs, xt, cs, ct, w, 1, n, dim, 4, out, None) == 1


def test_null_pointers_and_short_direction_strides_are_rejected(shw):
    lib = shw._lib.load()
    _keep, (xs, xt, th, out, cs, ct, w) = _bufs(7)
    assert lib.shw_esw_forward_dim(None, xt, th, 1, 8, 6, 4, 0, 2.0, out, None, None, None) == 1
    assert lib.shw_esw_forward_dim(xs, xt, None, 1, 8, 6, 4, 0, 2.0, out, None, None, None) == 1
    assert lib.shw_esw_forward_dim(xs, xt, th, 1, 8, 6, 4, 0, 2.0, None, None, None, None) == 1
    assert lib.shw_esw_forward_dim(xs, xt, th, 1, 8, 6, 4, 0, 2.0, out, cs, None, None) == 1    # one coef row only
    assert lib.shw_esw_forward_dim(xs, xt, th, 1, 8, 6, 4, 0, 0.5, out, None, None, None) == 1  # p < 1
    assert lib.shw_esw_forward_dim(xs, xt, th, 2, 8, 6, 4, 4 * 6 - 1, 2.0, out, None, None, None) == 1
    assert lib.shw_esw_backward_points_dim(None, cs, ct, w, 1, 8, 6, 4, 0, xs, xt, None) == 1
    assert lib.shw_esw_backward_points_dim(th, cs, ct, None, 1, 8, 6, 4, 0, xs, xt, None) == 1
    assert lib.shw_esw_backward_points_dim(th, cs, ct, w, 1, 8, 6, 4, 0, xs, None, None) == 1
    assert lib.shw_esw_backward_points_dim(th, cs, ct, w, 65536, 8, 6, 4, 0, xs, xt, None) == 1
    assert lib.shw_esw_backward_dirs_dim(xs, None, cs, ct, w, 1, 8, 6, 4, out, None) == 1
    assert lib.shw_esw_backward_dirs_dim(xs, xt, cs, ct, w, 1, 8, 6, 4, None, None) == 1


def test_cpu_clouds_of_any_dimension_are_refused_not_silently_computed(shw):
    import torch
    from shw_amd import esw
    assert esw.MAX_DIM == 64 and esw.MAX_POINTS == 4096
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        shw.esw_slice_sums(torch.zeros(1, 8, 6), torch.zeros(1, 8, 6), torch.zeros(4, 6))
