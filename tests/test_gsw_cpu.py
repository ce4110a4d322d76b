"""CPU checks of the generalised sliced-W family (no GPU needed): the float64 restatement the GPU tests lean on
(tests/helpers/gsw_restatement.py) reproduces the single-evaluation cases of fixture G16 -- the notebook cell exec'd on
the CPU, tools/make_golden_gsw.py; the monomial table has the fixture's feature counts; the new names are exported; the
four C entries are declared, bound, and reject bad arguments before any HIP call."""
import ctypes
import os

import numpy as np
import pytest
import torch

from helpers import gsw_restatement as R
from helpers.compare import grad_close

NEW_SYMBOLS = ("shw_gsw_rows_forward", "shw_gsw_circular_forward", "shw_gsw_circular_backward_points",
               "shw_gsw_circular_backward_dirs")
NEW_NAMES = ("sorted_row_sums", "gsw_circular_slice_sums", "gsw_polynomial_slice_sums", "GSWD_circular",
             "max_GSWD_circular", "poly_degree", "GSWD_polynomial", "max_GSWD_polynomial_3", "max_GSWD_polynomial_5",
             "gsw_nn_1", "gsw_nn_3", "max_gsw_nn_1", "max_gsw_nn_3", "cosine_distance_torch",
             "distributional_sliced_wasserstein_distance")


@pytest.fixture(scope="module")
def shw():
    import shw_amd
    if not os.path.exists(shw_amd._lib.LIB_PATH):
        shw_amd._lib.build()
    return shw_amd


@pytest.fixture(scope="module")
def cases(golden):
    g = golden("g16_notebook_gsw.npz")
    g10 = golden("g10_notebook_flow.npz")
    return g, torch.from_numpy(g10["source"]).double(), torch.from_numpy(g10["target"]).double()


def T(a):
    return torch.from_numpy(np.asarray(a)).double()


def _against_the_cell(g, name, val, grad):
    """The fixture is the cell's float32 run: a sum of 1200 fp32 terms per slice whose sorted differences carry the
    rounding of keys of size 1 (6e-8 absolute on differences of 1e-2 .. 1e-1), so 1e-5 relative on the value; its
    gradient within 2e-4 of the largest entry, as the G9 GPU test allows a float32 run against the same cell."""
    assert abs(val.item() - float(g[f"{name}_value"])) < 1e-5 * abs(float(g[f"{name}_value"]))
    grad_close(grad.numpy(), g[f"{name}_grad_first"], strict=2e-4, label=f"g16 cpu {name}")


@pytest.mark.parametrize("name", ["circ_p2", "circ_p1"])
def test_restatement_reproduces_g16_gswd_circular(cases, name):
    g, source, target = cases
    first = source.clone().requires_grad_(True)
    val = R.gswd_circular(first, target, T(g[f"{name}_theta"]), float(g[f"{name}_r"]), float(g[f"{name}_p"]))
    val.backward()
    _against_the_cell(g, name, val, first.grad)
    # the circular cases stay away from the singular point
    assert R.circular_keys(source, T(g[f"{name}_theta"]), float(g[f"{name}_r"])).min().item() > 1e-3


@pytest.mark.parametrize("name,degree", [("poly3", 3), ("poly5", 5)])
def test_restatement_reproduces_g16_gswd_polynomial(cases, name, degree):
    g, source, target = cases
    first = source.clone().requires_grad_(True)
    val = R.gswd_polynomial(first, target, T(g[f"{name}_coefficient"]), degree, 2)
    val.backward()
    _against_the_cell(g, name, val, first.grad)


def test_restatement_reproduces_g16_gsw_nn_1(cases):
    g, source, target = cases
    net = R.SmallMLP(3, 4, 8, 2, [g[f"mlp_param0_{k}"] for k in range(6)], dtype=torch.float64)
    first = source.clone().requires_grad_(True)
    val = R.gsw_nn(first, target, net, 2)
    val.backward()
    _against_the_cell(g, "nn1", val, first.grad)


def test_fixture_holds_every_case_and_a_gap_for_every_ascent_loop(cases):
    g = cases[0]
    for name in ("circ_p2", "circ_p1", "maxcirc", "poly3", "poly5", "maxpoly3", "maxpoly5", "dswd", "nn1", "maxnn1"):
        assert np.isfinite(g[f"{name}_value"]) and np.isfinite(g[f"{name}_grad_first"]).all(), name
        assert g[f"{name}_grad_first"].shape == (1200, 3)
    for name in ("maxcirc", "maxpoly3", "maxpoly5", "dswd", "maxnn1"):
        for kind in ("f32_gap", "grad_f32_gap", "param_f32_gap"):
            assert 0 <= float(g[f"{name}_{kind}"]) < 0.1, (name, kind)


def test_poly_degree_matches_the_fixtures_feature_counts(shw, cases):
    g = cases[0]
    assert shw.poly_degree(3, 3).shape == (int(g["poly3_features"]), 3) == (10, 3)
    assert shw.poly_degree(5, 3).shape == (int(g["poly5_features"]), 3) == (21, 3)
    for degree, dim in ((3, 3), (5, 3), (2, 4), (4, 1)):
        e = shw.poly_degree(degree, dim)
        assert e.dtype == torch.float32 and (e.sum(1) == degree).all() and len({tuple(r) for r in e.tolist()}) == len(e)
        assert torch.equal(e.double(), R.monomial_exponents(degree, dim))
    assert shw.poly_degree(3, 3)[0].tolist() == [0, 0, 3] and shw.poly_degree(3, 3)[-1].tolist() == [3, 0, 0]


def test_new_names_are_exported_and_entries_declared_and_bound(shw):
    from test_capi_cpu import declared_symbols
    for name in NEW_NAMES:
        assert callable(getattr(shw, name)), name
        assert name in shw.__all__, name
    lib = shw._lib.load()
    for name in NEW_SYMBOLS:
        assert name in declared_symbols(), name
        assert name in shw._lib.EXPORTED_SYMBOLS, name
        assert hasattr(lib, name), name
    assert lib.shw_abi_version() == shw._lib.ABI_VERSION == 3


def _bufs(k):
    keep = [ctypes.create_string_buffer(16) for _ in range(k)]
    return keep, [ctypes.addressof(b) for b in keep]


def test_bad_arguments_are_rejected_without_a_gpu(shw):
    lib = shw._lib.load()
    _keep, (xs, xt, th, out, cs, ct, w) = _bufs(7)
    assert lib.shw_gsw_rows_forward(None, xt, 3, 8, 2.0, out, None, None, None) == 1
    assert lib.shw_gsw_rows_forward(xs, xt, 3, 8, 2.0, None, None, None, None) == 1
    assert lib.shw_gsw_rows_forward(xs, xt, 3, 8, 2.0, out, cs, None, None) == 1          # one coefficient row only
    assert lib.shw_gsw_rows_forward(xs, xt, 3, 0, 2.0, out, None, None, None) == 1
    assert lib.shw_gsw_rows_forward(xs, xt, 3, 4097, 2.0, out, None, None, None) == 1
    assert lib.shw_gsw_rows_forward(xs, xt, -1, 8, 2.0, out, None, None, None) == 1
    assert lib.shw_gsw_rows_forward(xs, xt, 3, 8, 0.5, out, None, None, None) == 1        # p < 1
    assert lib.shw_gsw_rows_forward(xs, xt, 0, 8, 2.0, out, None, None, None) == 0        # nothing to do
    for dim, n in ((0, 8), (65, 8), (-1, 8), (6, 4097), (6, 0)):
        assert lib.shw_gsw_circular_forward(xs, xt, th, 1, n, dim, 4, 0, 1.0, 2.0, out, cs, ct, None) == 1
        assert lib.shw_gsw_circular_backward_points(xs, xt, th, cs, ct, w, 1, n, dim, 4, 0, 1.0, xs, xt, None) == 1
        assert lib.shw_gsw_circular_backward_dirs(xs, xt, th, cs, ct, w, 1, n, dim, 4, 0, 1.0, out, None) == 1
    assert lib.shw_gsw_circular_forward(xs, xt, None, 1, 8, 6, 4, 0, 1.0, 2.0, out, None, None, None) == 1
    assert lib.shw_gsw_circular_forward(xs, xt, th, 1, 8, 6, 4, 0, 1.0, 2.0, out, cs, None, None) == 1
    assert lib.shw_gsw_circular_forward(xs, xt, th, 1, 8, 6, 4, 0, 1.0, 0.5, out, None, None, None) == 1
    assert lib.shw_gsw_circular_forward(xs, xt, th, 2, 8, 6, 4, 4 * 6 - 1, 1.0, 2.0, out, None, None, None) == 1
    assert lib.shw_gsw_circular_backward_points(xs, xt, th, cs, ct, None, 1, 8, 6, 4, 0, 1.0, xs, xt, None) == 1
    assert lib.shw_gsw_circular_backward_points(xs, xt, th, cs, ct, w, 65536, 8, 6, 4, 0, 1.0, xs, xt, None) == 1
    assert lib.shw_gsw_circular_backward_dirs(xs, xt, th, cs, ct, w, 1, 8, 6, 4, 0, 1.0, None, None) == 1
    assert lib.shw_gsw_circular_backward_dirs(xs, xt, th, cs, ct, w, 65536, 8, 6, 4, 0, 1.0, out, None) == 1


def test_cpu_tensors_and_oversized_polynomials_are_refused(shw):
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        shw.sorted_row_sums(torch.zeros(3, 8), torch.zeros(3, 8))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        shw.gsw_circular_slice_sums(torch.zeros(1, 8, 3), torch.zeros(1, 8, 3), torch.zeros(4, 3))
    with pytest.raises(ValueError, match="at most 64"):
        shw.gsw_polynomial_slice_sums(torch.zeros(1, 8, 3), torch.zeros(1, 8, 3), torch.zeros(66, 4), 10)


def _unit_rows(L):
    t = torch.randn((L, 3))
    return (t / torch.sqrt(torch.sum(t ** 2, dim=1, keepdim=True))).double()


@pytest.mark.parametrize("name", ["maxcirc", "maxpoly3", "maxpoly5", "dswd", "maxnn1"])
def test_restatement_ascent_loops_land_on_the_cells_values(cases, name):
    """The helper's ascent loops in float64 against the cell's float32 run: the value within 8 x the fixture's own
    float32 / float64 gap of the case, or the single-evaluation 1e-5 where that is larger."""
    g, source, target = cases
    iters = int(g["max_iter"])
    if name == "maxcirc":
        val, theta = R.max_gswd_circular(source, target, T(g["maxcirc_theta0"]), 1, 2, iters)
        assert np.abs(theta.numpy() - g["maxcirc_theta"]).max() < 1e-4
    elif name.startswith("maxpoly"):
        degree = int(name[-1])
        val, coef = R.max_gswd_polynomial(source, target, T(g[f"{name}_coefficient0"]), degree, 2, iters)
        assert np.abs(coef.numpy() - g[f"{name}_coefficient"]).max() < 1e-4
    elif name == "dswd":
        f = R.UnitLinear(3, g["dswd_weight0"], g["dswd_bias0"], dtype=torch.float64)
        f_op = torch.optim.Adam(f.parameters(), lr=0.005, betas=(0.999, 0.999))
        torch.manual_seed(int(g["dswd_seed"]))
        draws = torch.stack([_unit_rows(int(g["dswd_L"])) for _ in range(iters + 2)])[1:]   # the first is discarded
        val = R.dswd(source, target, draws, f, f_op, 2, iters, float(g["dswd_lam"]))
        assert np.abs(f.net[0].weight.detach().numpy() - g["dswd_weight"]).max() < 1e-4
    else:
        net = R.SmallMLP(3, 4, 8, 2, [g[f"mlp_param0_{k}"] for k in range(6)], dtype=torch.float64)
        val = R.max_gsw_nn(source, target, net, torch.optim.Adam(net.parameters(), lr=0.005), iters, 2)
    bound = max(8 * float(g[f"{name}_f32_gap"]), 1e-5)
    assert abs(val.item() - float(g[f"{name}_value"])) < bound * abs(float(g[f"{name}_value"])), (val.item(), bound)
