"""CPU checks of the line transport (csrc/shw_line_ot.hip, line_ot.py): the two references of
tests/helpers/line_ot_cases.py agree with each other, the boundary carries the new names, and bad arguments are refused
without a GPU."""
import os
import re

import pytest
import torch

from helpers.line_ot_cases import POWERS, SIZES, integer_weights, quantile_merge, replication, rows

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ["shw_line_rows_forward", "shw_line_esw_forward", "shw_line_esw_backward_points", "shw_line_esw_backward_dirs"]
NAMES = ["line_ot_rows", "esw_slice_costs", "weighted_sliced_wasserstein_distance"]


@pytest.fixture(scope="module")
def shw():
    import shw_amd
    if not os.path.exists(shw_amd._lib.LIB_PATH):
        shw_amd._lib.build()
    return shw_amd


@pytest.mark.parametrize("n,m", [s for s in SIZES if s[0] * s[1] <= 2048 * 1536])
def test_restatement_agrees_with_atom_replication(n, m):
    """float64 quantile merge against replicated atoms, <= 1e-12 relative: uniform n != m (k = lcm/n, lcm/m), integer
    weights, and one atom holding 90 % of the mass"""
    u, v = rows(n, m, seed=n * 7 + m, count=1)
    worst = 0.0
    for p in POWERS:
        ref = replication(u[0].numpy(), v[0].numpy(), p)
        worst = max(worst, abs(quantile_merge(u[0], v[0], p).item() - ref) / ref)
        for heavy in (False, True):
            ku, kv = integer_weights(n, m, seed=11, heavy=heavy)
            ref = replication(u[0].numpy(), v[0].numpy(), p, ku, kv)
            got = quantile_merge(u[0], v[0], p, torch.from_numpy(ku), torch.from_numpy(kv)).item()
            worst = max(worst, abs(got - ref) / ref)
    assert worst <= 1e-12, worst


def test_restatement_equal_sizes_is_the_mean_sorted_difference():
    u, v = rows(300, 300, seed=5)
    for p in POWERS:
        want = (torch.sort(u.double(), -1).values - torch.sort(v.double(), -1).values).abs().pow(p).mean(-1)
        assert torch.allclose(quantile_merge(u, v, p), want, rtol=1e-13, atol=0)


def test_restatement_ignores_zero_weight_atoms():
    u, v = rows(48, 36, seed=9)
    pad = torch.full((u.shape[0], 5), 77.0)
    a = torch.cat([torch.ones(48), torch.zeros(5)])
    got = quantile_merge(torch.cat([u, pad], -1), v, 2, a, None)
    assert torch.allclose(got, quantile_merge(u, v, 2), rtol=1e-13, atol=0)


def test_header_loader_and_package_carry_the_new_names(shw):
    text = open(os.path.join(ROOT, "include", "shw.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(shw_[a-z0-9_]+)\s*\(", text))
    lib = shw._lib.load()
    for name in ENTRIES:
        assert name in declared, name
        assert name in shw._lib.EXPORTED_SYMBOLS, name
        assert hasattr(lib, name), name
    assert re.search(r"#define\s+SHW_ABI_VERSION\s+3\b", text)
    assert lib.shw_abi_version() == shw._lib.ABI_VERSION == 3
    for name in NAMES:
        assert name in shw.__all__ and callable(getattr(shw, name)), name
    assert shw.line_ot.line_ot_rows is shw.line_ot_rows


def test_argument_validation_needs_no_gpu(shw):
    lib = shw._lib.load()
    P = 4096            # any non-null value: every call below is refused before a pointer is read
    # null pointers
    assert lib.shw_line_rows_forward(None, None, 1, 8, 8, 2.0, None, None, 0, 0, None, None, None, None) == 1
    assert lib.shw_line_esw_forward(None, None, None, 1, 8, 8, 3, 4, 0, 2.0, None, None, 0, 0, None, None, None, None) == 1
    assert lib.shw_line_esw_backward_points(None, None, None, None, 1, 8, 8, 3, 4, 0, None, None, None) == 1
    assert lib.shw_line_esw_backward_dirs(None, None, None, None, None, 1, 8, 8, 3, 4, None, None) == 1
    # sizes out of range: n, m in 1..4096, D in 1..64, p >= 1, B <= 65535, one coefficient row without the other
    for n, m in ((0, 8), (8, 0), (4097, 8), (8, 4097)):
        assert lib.shw_line_rows_forward(P, P, 1, n, m, 2.0, None, None, 0, 0, P, None, None, None) == 1
        assert lib.shw_line_esw_forward(P, P, P, 1, n, m, 3, 4, 0, 2.0, None, None, 0, 0, P, None, None, None) == 1
        assert lib.shw_line_esw_backward_points(P, P, P, P, 1, n, m, 3, 4, 0, P, P, None) == 1
        assert lib.shw_line_esw_backward_dirs(P, P, P, P, P, 1, n, m, 3, 4, P, None) == 1
    assert lib.shw_line_rows_forward(P, P, 1, 8, 8, 0.5, None, None, 0, 0, P, None, None, None) == 1
    assert lib.shw_line_rows_forward(P, P, -1, 8, 8, 2.0, None, None, 0, 0, P, None, None, None) == 1
    assert lib.shw_line_rows_forward(P, P, 1, 8, 8, 2.0, None, None, 0, 0, P, P, None, None) == 1
    for dim in (0, 65):
        assert lib.shw_line_esw_forward(P, P, P, 1, 8, 8, dim, 4, 0, 2.0, None, None, 0, 0, P, None, None, None) == 1
    assert lib.shw_line_esw_forward(P, P, P, 65536, 8, 8, 3, 4, 0, 2.0, None, None, 0, 0, P, None, None, None) == 1
    assert lib.shw_line_esw_forward(P, P, P, 1, 8, 8, 3, 4, 11, 2.0, None, None, 0, 0, P, None, None, None) == 1
    # weights: a stride without a pointer, a stride shorter than the row
    assert lib.shw_line_rows_forward(P, P, 1, 8, 8, 2.0, None, None, 8, 0, P, None, None, None) == 1
    assert lib.shw_line_rows_forward(P, P, 1, 8, 8, 2.0, P, P, 0, 7, P, None, None, None) == 1
    # nothing to do: no launch, success
    assert lib.shw_line_rows_forward(P, P, 0, 8, 8, 2.0, None, None, 0, 0, P, None, None, None) == 0


def test_cpu_tensors_are_refused_not_silently_computed(shw):
    u, v = torch.zeros(2, 8), torch.zeros(2, 6)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        shw.line_ot_rows(u, v)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        shw.esw_slice_costs(torch.zeros(1, 8, 3), torch.zeros(1, 6, 3), torch.zeros(4, 3))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        shw.weighted_sliced_wasserstein_distance(torch.zeros(8, 3), torch.zeros(6, 3), device="cpu")
    assert "mass-normalised" in shw.weighted_sliced_wasserstein_distance.__doc__
    assert "sliced_wasserstein_distance / n^(1/p)" in shw.weighted_sliced_wasserstein_distance.__doc__
