"""CPU checks of the exact-W path for clouds of different sizes (csrc/shw_emd_units.hip, emd.transport_pair_costs): the
boundary, the size rule, and -- on the restatement of tests/helpers/emd_units_cases.py, emd_cases.auction run on the
expanded unit x slot costs -- the claims the kernel is built on and the conditions tests/test_emd_units_gpu.py relies on.
No GPU.

The independent solver is scipy.optimize.linear_sum_assignment on the expanded float64 matrix; POT is not installed, so
parity with ot.emd2 itself is unpinned, as in tests/test_emd_cpu.py."""
import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch

from helpers import emd_cases
from helpers import emd_units_cases as cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ["shw_emd_units_supported", "shw_emd_units_workspace_bytes", "shw_emd_units_forward", "shw_emd_units_backward"]
NAMES = ["transport_pair_costs", "transport_units"]
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
    assert shw._lib.ABI_VERSION == lib.shw_abi_version() == 3          # symbols were added, nothing changed
    for name in NAMES:
        assert name in shw.__all__ and callable(getattr(shw, name)), name


def test_invalid_arguments_return_1_before_any_hip_call(shw):
    lib = shw._lib.load()
    one = ctypes.c_void_p(16)             # a non-null pointer that is never dereferenced: validation comes first

    def fwd(pairs=1, n=8, m=12, kind=0, p=2.0, ptr=one):
        return lib.shw_emd_units_forward(ptr, ptr, pairs, n, m, kind, p, ptr, ptr, ptr, ptr, None)

    def bwd(pairs=1, n=8, m=12, kind=0, p=2.0, ptr=one):
        return lib.shw_emd_units_backward(ptr, ptr, ptr, ptr, pairs, n, m, kind, p, ptr, ptr, None)

    for f in (fwd, bwd):
        assert f(ptr=None) == 1                                               # null pointers
        assert f(n=1000, m=1024) == 1                                         # lcm 128 000
        assert f(n=1800, m=1200) == 1                                         # lcm 3600 <= 4096, but 180 000 bytes of LDS
        assert f(n=2049, m=2049) == 1 and f(n=2049, m=1) == 1 and f(n=1, m=2049) == 1
        assert f(m=0) == 1 and f(n=0) == 1 and f(n=-4, m=-4) == 1
        assert f(kind=2) == 1 and f(kind=-1) == 1
        assert f(p=0.5) == 1 and f(p=float("nan")) == 1
        assert f(pairs=65536) == 1 and f(pairs=-1) == 1
        assert f(pairs=0) == 0                                                # a no-op, not an error
        assert f(pairs=0, n=1000, m=1024) == 1                                # ... of a pair that is served only


def test_supported_agrees_with_the_size_rule_on_a_grid(shw):
    lib = shw._lib.load()
    sizes = sorted({1, 2, 3, 7, 8, 12, 13, 64, 65, 75, 96, 100, 128, 200, 256, 512, 700, 768, 819, 1000, 1024, 1050, 1200,
                    1365, 1536, 1700, 1800, 2047, 2048})
    served = 0
    for n in sizes:
        for m in sizes:
            want = cases.units(n, m)
            got = lib.shw_emd_units_supported(n, m)
            assert got == (want[0] if want else 0), (n, m)
            if want:
                served += 1
                U, ks, kt = want
                assert U == math.lcm(n, m) == n * ks == m * kt and shw.transport_units(n, m) == want
            if math.lcm(n, m) <= 2048:                                        # the required floor, n == m included
                assert got == math.lcm(n, m), (n, m)
    assert served > len(sizes)
    assert lib.shw_emd_units_supported(768, 1024) == lib.shw_emd_units_supported(1536, 1024) == 3072
    assert lib.shw_emd_units_supported(1700, 200) == 3400                     # 158 800 bytes: inside
    assert lib.shw_emd_units_supported(1800, 1200) == 0                       # 180 000 bytes: outside
    assert lib.shw_emd_units_supported(1365, 819) == 0                        # U = 4095, 163 840 + bytes
    assert lib.shw_emd_units_supported(1000, 1024) == 0
    for n, m in ((0, 5), (5, 0), (-1, 4), (2049, 2049), (1, 2049)):
        assert lib.shw_emd_units_supported(n, m) == 0 and cases.units(n, m) is None


def test_workspace_size_and_round_cap(shw):
    lib = shw._lib.load()
    # the target of each unit, the source of each slot (int32 each) and one flag per pair
    assert lib.shw_emd_units_workspace_bytes(3, 8, 12) == (2 * 3 * 24 + 3) * 4
    assert lib.shw_emd_units_workspace_bytes(5, 768, 1024) == (2 * 5 * 3072 + 5) * 4
    assert lib.shw_emd_units_workspace_bytes(0, 8, 12) == 0
    assert lib.shw_emd_units_workspace_bytes(3, 1000, 1024) == 0 and lib.shw_emd_units_workspace_bytes(-1, 8, 12) == 0
    assert lib.shw_emd_units_workspace_bytes(2, 65, 65) == lib.shw_emd_workspace_bytes(2, 65)
    src = open(os.path.join(os.path.dirname(shw.__file__), "csrc", "shw_emd_units.hip")).read()
    m = re.search(r"emd_units_round_cap\(int U\) \{ return (\d+) \* U \+ (\d+); \}", src)
    assert m and emd_cases.round_cap(3072) == int(m.group(1)) * 3072 + int(m.group(2))


def test_python_refusals(shw, monkeypatch):
    x, y = torch.zeros(2, 8, 3), torch.zeros(2, 12, 3)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        shw.transport_pair_costs(x, y)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        shw.Cos_disimilarity_W("cpu", p=2)(x, y)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        shw.wasserstein_distance(x[0], y[0], "cpu")
    with pytest.raises(TypeError, match="float32"):
        shw.transport_pair_costs(x.double(), y.double())
    with pytest.raises(TypeError):
        shw.transport_pair_costs(x.half(), y.half())
    with pytest.raises(TypeError):
        shw.transport_pair_costs(x, y, weights=None)                         # uniform weights only: no such argument
    # the size checks come after the device check: reached by letting that one pass; nothing is launched, every call
    # below raises before the library's forward is entered
    from importlib import import_module
    emd = import_module(shw.__name__ + ".emd")
    monkeypatch.setattr(emd, "_check_cloud", lambda name, t: None)
    with pytest.raises(ValueError, match=r"n = 1000, m = 1024.*lcm\(n, m\) = 128000.*limit of 4096"):
        shw.transport_pair_costs(torch.zeros(1, 1000, 3), torch.zeros(1, 1024, 3))
    with pytest.raises(ValueError, match=r"n = 1800, m = 1200.*lcm\(n, m\) = 3600.*180000 bytes.*limit of 162816"):
        shw.transport_units(1800, 1200)
    with pytest.raises(ValueError, match="limit.*2049"):
        shw.transport_units(2049, 4)
    with pytest.raises(ValueError, match="limit"):
        shw.transport_units(4, 0)
    with pytest.raises(ValueError, match="'lp' or 'geodesic'"):
        shw.transport_pair_costs(x, y, cost="cosine")
    with pytest.raises(ValueError, match="p must be >= 1"):
        shw.transport_pair_costs(x, y, p=0.5)
    with pytest.raises(ValueError, match="same B"):
        shw.transport_pair_costs(x, y[:1])
    with pytest.raises(ValueError, match="equal sizes"):                      # the equal-size entry keeps its refusal
        shw.emd_pair_costs(x, y)


# ------------------------------------------------------------------------------------------------------ restatement
def test_case_list_covers_the_shapes_the_kernel_distinguishes():
    shapes = {(c[1], c[2]) for c in cases.CASES}
    assert {(1, 2), (1, 7), (7, 1), (2, 3), (3, 2), (8, 12), (12, 8), (65, 13), (64, 96), (96, 64), (100, 75), (128, 256),
            (128, 512), (65, 65), (32, 48), (33, 66), (768, 1024)} == shapes
    assert all(cases.units(n, m) for n, m in shapes)
    assert max(cases.units(n, m)[0] for n, m in shapes) == 3072
    assert {c[4] for c in cases.CASES if c[3] == "lp"} == {1.0, 2.0, 3.0}
    assert ("zeros", 32, 48, "geodesic", 2.0) in cases.CASES and ("zeros", 32, 48, "lp", 2.0) in cases.CASES
    assert cases.lds_bytes(768, 1024) == 144384 and cases.lds_bytes(1024, 1536) == 153600 <= cases.LDS_LIMIT


@pytest.mark.parametrize("case", cases.CASES, ids=IDS)
def test_restatement_returns_a_feasible_unit_plan_within_the_bound_and_under_the_cap(case):
    cloud, n, m, kind, p = case
    ref, run = cases.reference(case), cases.restated(case)
    U, ks, kt = ref["U"], ref["ks"], ref["kt"]
    assert run["targets"] is not None, "round cap reached"
    assert run["targets"].shape == (U,) and cases.feasible(run["targets"], m, kt)
    assert cases.feasible(ref["targets"], m, kt)
    got = cases.mean_along(ref["x"], ref["y"], kind, p, run["targets"], ks)
    g = cases.eval_gap(ref["x"], ref["y"], kind, p, run["targets"], ks)
    gap, allowed = got - ref["opt"], emd_cases.value_bound(ref["K"], g)
    print(f"EMD units restatement {cases.case_id(case)}: U {U} K {ref['K']:g} optimum {ref['opt']:.9e} gap {gap:.3e} "
          f"allowed {allowed:.3e} rounds {run['rounds']} ({run['rounds'] / U:.1f} U) bids {run['bids'] / U:.1f} U")
    assert -allowed <= gap <= allowed
    assert run["rounds"] < emd_cases.round_cap(U) / 8
    assert ref["K"] == run["K"]
    assert emd_cases.cost_matrix(ref["x"], ref["y"], kind, p, np.float32).max() <= ref["K"]
    assert 0 <= run["c"].min() and run["c"].max() <= 2 ** emd_cases.FRAC_BITS


def test_doubled_target_has_one_plan_at_the_solver_resolution():
    """What the GPU test's `cost == 0.0` rests on: sending both units of source i to its two copies has integer cost 0,
    and every other (source, target) couple costs >= 2, so by eps-complementary slackness at eps = 1 (the argument of
    tests/test_emd_cpu.py's permuted cases, on units) no other plan can be returned."""
    case = ("doubled", 33, 66, "lp", 2.0)
    ref, run = cases.reference(case), cases.restated(case)
    c = run["c"].copy()
    own = np.arange(66) // 2
    assert np.all(c[own, np.arange(66)] == 0)
    c[own, np.arange(66)] = np.iinfo(np.int64).max
    assert c.min() >= 2
    assert ref["opt"] == 0.0
    assert np.array_equal(np.sort(run["targets"].reshape(33, 2), axis=1), np.arange(66).reshape(33, 2))


def test_all_zero_clouds_have_bound_zero_only_for_the_lp_cost():
    lp, geo = cases.restated(("zeros", 32, 48, "lp", 2.0)), cases.restated(("zeros", 32, 48, "geodesic", 2.0))
    assert lp["K"] == 0 and lp["rounds"] == 0 and cases.feasible(lp["targets"], 48, 2)
    assert geo["K"] == 16 and np.all(geo["c"] == geo["c"][0, 0])
    assert 8 * geo["rounds"] < emd_cases.round_cap(96)


def test_equal_sizes_restate_the_equal_size_problem():
    """ks = kt = 1: the expanded matrix is the matrix, so the unit solver and emd_pair_costs run one rule on one input"""
    case = ("sphere", 65, 65, "lp", 2.0)
    ref, run = cases.reference(case), cases.restated(case)
    assert (ref["U"], ref["ks"], ref["kt"]) == (65, 1, 1)
    assign, rounds, _ = emd_cases.auction(run["c"])
    assert np.array_equal(assign, run["targets"]) and rounds == run["rounds"]


def test_gradient_inputs_are_away_from_the_kinks_and_split_their_rows():
    """No matched couple can sit where the cost has no derivative, whatever the plan: no coordinate difference is 0 (lp,
    p = 1) and no two points are parallel (angle cost)."""
    for n, m, kind, p in cases.GRAD_CASES:
        assert cases.units(n, m)
        x, y = cases.grad_inputs(n, m)
        assert x.shape == (len(cases.GRAD_W), n, 3) and y.shape == (len(cases.GRAD_W), m, 3) and x.dtype == np.float32
        for b in range(x.shape[0]):
            assert np.abs(x[b][:, None, :] - y[b][None, :, :]).min() > 0
            theta = emd_cases.cost_matrix(x[b], y[b], "geodesic", 1.0)
            assert theta.min() > 1e-4 and theta.max() < np.pi - 1e-4
