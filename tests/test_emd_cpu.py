"""CPU checks of the exact-W path (csrc/shw_emd.hip, emd.py): the boundary, and -- on the NumPy restatement of the
auction rule in tests/helpers/emd_cases.py -- the claims the kernel is built on and the conditions the GPU tests
(tests/test_emd_gpu.py) rely on.  No GPU.

The restatement is compared with scipy.optimize.linear_sum_assignment (float64), an independent exact solver; POT, which
the reference calls, is not installed, so parity with ot.emd2 itself is unpinned."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from helpers import emd_cases as cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ["shw_max_points_emd", "shw_emd_workspace_bytes", "shw_emd_forward", "shw_emd_backward"]
NAMES = ["emd_pair_costs", "Cos_disimilarity_W", "Geodesic_distance_W", "wasserstein_distance", "wasserstein_distance_geo"]
IDS = [cases.case_id(c) for c in cases.CASES]


@pytest.fixture(scope="module")
def shw():
    import shw_amd
    if not os.path.exists(shw_amd._lib.LIB_PATH):
        shw_amd._lib.build()
    return shw_amd


# ---------------------------------------------------------------------------------------------------------- boundary
def test_entries_are_declared_bound_and_exported(shw):
    header = open(os.path.join(ROOT, "include", "shw.h")).read()
    lib = shw._lib.load()
    for name in ENTRIES:
        assert re.search(r"SHW_API\s+\w+\s+%s\s*\(" % name, header), name
        assert name in shw._lib.EXPORTED_SYMBOLS and hasattr(lib, name), name
    assert shw._lib.ABI_VERSION == lib.shw_abi_version() == 3
    for name in NAMES:
        assert name in shw.__all__ and callable(getattr(shw, name)), name


def test_limit_workspace_and_helper_constants_agree_with_the_library(shw):
    lib = shw._lib.load()
    assert lib.shw_max_points_emd() == cases.LIMIT >= 2048
    assert shw.max_points_emd() == cases.LIMIT
    # the assignment, its inverse (int32 each) and one flag per pair
    assert lib.shw_emd_workspace_bytes(3, 100) == (2 * 3 * 100 + 3) * 4
    src = open(os.path.join(os.path.dirname(shw.__file__), "csrc", "shw_emd.hip")).read()
    m = re.search(r"emd_round_cap\(int n\) \{ return (\d+) \* n \+ (\d+); \}", src)
    assert m and cases.round_cap(7) == int(m.group(1)) * 7 + int(m.group(2))


def test_invalid_arguments_return_1_before_any_hip_call(shw):
    lib = shw._lib.load()
    limit = lib.shw_max_points_emd()
    one = ctypes.c_void_p(16)             # a non-null pointer that is never dereferenced: validation comes first

    def fwd(pairs=1, n=8, m=8, kind=0, p=2.0, ptr=one):
        return lib.shw_emd_forward(ptr, ptr, pairs, n, m, kind, p, ptr, ptr, ptr, ptr, None)

    def bwd(pairs=1, n=8, kind=0, p=2.0, ptr=one):
        return lib.shw_emd_backward(ptr, ptr, ptr, ptr, pairs, n, kind, p, ptr, ptr, None)

    assert fwd(ptr=None) == 1 and bwd(ptr=None) == 1                          # null pointers
    assert fwd(n=8, m=9) == 1                                                 # unequal sizes
    assert fwd(n=0, m=0) == 1 and bwd(n=0) == 1
    assert fwd(n=limit + 1, m=limit + 1) == 1 and bwd(n=limit + 1) == 1
    assert fwd(p=0.5) == 1 and bwd(p=0.5) == 1 and fwd(p=float("nan")) == 1
    assert fwd(kind=2) == 1 and fwd(kind=-1) == 1 and bwd(kind=2) == 1
    assert fwd(pairs=65536) == 1 and bwd(pairs=65536) == 1 and fwd(pairs=-1) == 1
    assert fwd(pairs=0) == 0 and bwd(pairs=0) == 0                            # a no-op, not an error


def test_cpu_tensors_and_other_dtypes_are_refused(shw):
    x = torch.zeros(2, 8, 3)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        shw.emd_pair_costs(x, x)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        shw.Cos_disimilarity_W("cpu", p=2)(x, x)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        shw.wasserstein_distance(x[0], x[0], "cpu")
    with pytest.raises(TypeError):
        shw.emd_pair_costs(x.double(), x.double())
    with pytest.raises(TypeError):
        shw.emd_pair_costs(x.half(), x.half())


def test_wrapper_argument_checks_name_the_rule(shw, monkeypatch):
    """The size checks come after the device check; on a machine without a GPU they are reached by letting the device
    check pass (nothing is launched: every call below raises before the library is entered)."""
    from importlib import import_module
    emd = import_module(shw.__name__ + ".emd")
    monkeypatch.setattr(emd, "_check_cloud", lambda name, t: None)
    x = torch.zeros(2, 8, 3)
    with pytest.raises(ValueError, match="equal sizes"):
        shw.emd_pair_costs(x, torch.zeros(2, 9, 3))
    with pytest.raises(ValueError, match=f"limit.*{cases.LIMIT + 1}|{cases.LIMIT}.*limit"):
        shw.emd_pair_costs(torch.zeros(1, cases.LIMIT + 1, 3), torch.zeros(1, cases.LIMIT + 1, 3))
    with pytest.raises(ValueError, match="'lp' or 'geodesic'"):
        shw.emd_pair_costs(x, x, cost="cosine")
    with pytest.raises(ValueError, match="p must be >= 1"):
        shw.emd_pair_costs(x, x, p=0.5)


# ------------------------------------------------------------------------------------------------------ restatement
def test_case_list_covers_the_sizes_clouds_and_powers():
    sizes = {c[1] for c in cases.CASES}
    assert {1, 2, 63, 64, 65, 257, 1000, 2048, cases.LIMIT} <= sizes
    assert {c[0] for c in cases.CASES} == {"sphere", "registration", "permuted", "lattice", "clusters", "zeros",
                                          "times1000", "times0.001", "plus100", "cube"}
    assert {c[3] for c in cases.CASES if c[2] == "lp"} == {1.0, 2.0, 3.0}
    assert {c[3] for c in cases.CASES if c[2] == "geodesic"} == {1.0, 2.0}
    assert ("clusters", 512, "lp", 2.0) in cases.CASES and ("cube", 1200, "lp", 2.0) in cases.CASES


@pytest.mark.parametrize("case", cases.CASES, ids=IDS)
def test_restatement_returns_a_permutation_within_the_bound_and_under_the_cap(case):
    cloud, n, kind, p = case
    ref, run = cases.reference(case), cases.restated(case)
    assert run["assign"] is not None, "round cap reached"
    assert np.array_equal(np.sort(run["assign"]), np.arange(n))
    got = cases.mean_along(ref["x"], ref["y"], kind, p, run["assign"])
    g = cases.eval_gap(ref["x"], ref["y"], kind, p, run["assign"])
    gap, allowed = got - ref["opt"], cases.value_bound(ref["K"], g)
    print(f"EMD restatement {cases.case_id(case)}: K {ref['K']:g} optimum {ref['opt']:.9e} gap {gap:.3e} allowed "
          f"{allowed:.3e} rounds {run['rounds']} ({run['rounds'] / n:.1f} n) bids {run['bids'] / n:.1f} n")
    assert -allowed <= gap <= allowed
    assert run["rounds"] < cases.round_cap(n) / 8
    # K bounds every cost the kernel can see, and the integer costs stay in range
    assert ref["K"] == run["K"]
    assert cases.cost_matrix(ref["x"], ref["y"], kind, p, np.float32).max() <= ref["K"]
    assert 0 <= run["c"].min() and run["c"].max() <= 2 ** cases.FRAC_BITS


@pytest.mark.parametrize("case", [c for c in cases.CASES if c[0] == "permuted"],
                         ids=[cases.case_id(c) for c in cases.CASES if c[0] == "permuted"])
def test_permuted_cases_have_one_optimum_at_the_solver_resolution(case):
    """What the GPU test's assignment equality rests on.  The inverse permutation has integer cost 0.  Any other
    permutation differs from it on cycles, and eps-complementary slackness at eps = 1 lets the solver return one only
    if a cycle of k couples costs at most k in all: with every integer cost off the matched couples >= 2 that cannot
    happen, so the solver must return exactly the inverse permutation."""
    cloud, n, kind, p = case
    ref, run = cases.reference(case), cases.restated(case)
    inverse = ref["extra"]["inverse"]
    c = run["c"].copy()
    assert np.all(c[np.arange(n), inverse] == 0)
    c[np.arange(n), inverse] = np.iinfo(np.int64).max
    assert c.min() >= 2
    assert ref["opt"] == 0.0
    assert np.array_equal(run["assign"], inverse)


def test_all_zero_clouds_have_bound_zero_only_for_the_lp_cost():
    """K = 0 (identity returned without a round) is the all-costs-zero case; with the angle cost two all-zero clouds cost
    (pi / 2)^p everywhere, the worst case for the round count (every target ties): the cap table's largest ratio."""
    assert cases.restated(("zeros", 64, "lp", 2.0))["K"] == 0 and cases.restated(("zeros", 64, "lp", 2.0))["rounds"] == 0
    run = cases.restated(("zeros", 64, "geodesic", 2.0))
    assert run["K"] == 16 and np.all(run["c"] == run["c"][0, 0])
    assert 8 * run["rounds"] < cases.round_cap(64)


def test_gradient_inputs_are_away_from_the_kinks():
    """The gradient tests differentiate along the kernel's own assignment; what they need from the inputs is that no
    matched couple sits where the cost has no derivative, whatever the assignment: no coordinate difference is 0 (lp,
    p = 1) and no two points are parallel (angle cost)."""
    for n in sorted({c[0] for c in cases.GRAD_CASES}):
        x, y = cases.grad_inputs(n)
        assert x.shape == y.shape == (len(cases.GRAD_W), n, 3) and x.dtype == np.float32
        for b in range(x.shape[0]):
            assert np.abs(x[b][:, None, :] - y[b][None, :, :]).min() > 0
            theta = cases.cost_matrix(x[b], y[b], "geodesic", 1.0)
            assert theta.min() > 1e-4 and theta.max() < np.pi - 1e-4
