"""CPU checks behind tests/test_sinkhorn_chamfer_gpu.py (no GPU needed):
  * oracle/sinkhorn_mirror.sinkhorn_costs(history=True) returns the same first four values, bit for bit, as the default
    call on the G7 / G7b fixtures, and its extra values are what they claim to be;
  * every condition the GPU tests rely on holds on the seeded inputs of tests/helpers/sinkhorn_chamfer_cases.py, so a
    condition that fails is seen here and not as an unexplained GPU failure."""
import numpy as np
import pytest
import torch

from helpers import sinkhorn_chamfer_cases as cases
from oracle import sinkhorn_mirror


def T(a):
    return torch.from_numpy(np.ascontiguousarray(a))


# --------------------------------------------------------------------------------------- the mirror's history keyword
@pytest.mark.parametrize("eps,iters,kw", [(0.05, 60, {}), (0.01, 100, {}), (0.05, 60, dict(norm_p=1)),
                                          (0.05, 60, dict(cost_pow=2)), (0.5, 200, dict(thresh=1e-3))])
def test_history_keyword_leaves_the_g7_results_unchanged(golden, eps, iters, kw):
    g = golden("g7_sinkhorn.npz")
    x, y = T(g["x"]), T(g["y"])
    plain = sinkhorn_mirror.sinkhorn_costs(x, y, eps, iters, **kw)
    hist = sinkhorn_mirror.sinkhorn_costs(x, y, eps, iters, history=True, **kw)
    assert len(plain) == 4 and len(hist) == 6
    for a, b in zip(plain[:3], hist[:3]):
        assert torch.equal(a, b)
    assert plain[3] == hist[3]
    stats, (u, v) = hist[4], hist[5]
    assert len(stats) == hist[3] and all(isinstance(s, float) for s in stats)
    # the statistic of the last executed sweep is the one the stop was decided on
    thresh = kw.get("thresh", 1e-9)
    assert all(s >= thresh for s in stats[:-1]) and (hist[3] == iters or stats[-1] < thresh)
    # the duals are those of the returned plan
    assert torch.equal(torch.exp((-hist[2] + u.unsqueeze(-1) + v.unsqueeze(-2)) / eps), hist[1])
    if not kw:                                                  # still the fixture of the real class
        tag = f"eps{eps}_it{iters}"
        assert cases.relmax(hist[0].numpy(), g[f"cost_{tag}"]) < 2e-5


@pytest.mark.parametrize("tag,eps,iters,norm_p,cost_pow", [("eps0.05_it60", 0.05, 60, 2, 1), ("L1_eps0.05_it30", 0.05, 30, 1, 1),
                                                           ("N2_eps0.05_it30", 0.05, 30, 2, 2)])
def test_history_keyword_leaves_the_g7b_gradients_unchanged(golden, tag, eps, iters, norm_p, cost_pow):
    g = golden("g7b_sinkhorn_grad.npz")
    grads = []
    for history in (False, True):
        x, y = T(g["x"]).requires_grad_(True), T(g["y"]).requires_grad_(True)
        cost = sinkhorn_mirror.sinkhorn_costs(x, y, eps, iters, norm_p=norm_p, cost_pow=cost_pow, history=history)[0]
        cost.pow(1.0 / cost_pow).sum().backward()
        grads.append((cost.detach(), x.grad, y.grad))
    for a, b in zip(*grads):
        assert torch.equal(a, b)


def test_history_with_no_sweep():
    x, y = cases.forward_inputs(9, 7)
    cost, P, C, it, stats, (u, v) = sinkhorn_mirror.sinkhorn_costs(x, y, 0.05, 0, history=True)
    assert it == 0 and stats == [] and not u.any() and not v.any()
    assert torch.equal(P, torch.exp(-C / 0.05))


# ------------------------------------------------------------------------------- conditions of the GPU Sinkhorn tests
@pytest.mark.parametrize("n,m,eps,iters", cases.FORWARD_CASES)
def test_forward_cases_run_every_sweep_and_have_the_stated_gaps(n, m, eps, iters):
    """Both mirror runs execute the same sweeps, so their difference is rounding and not one sweep more or less; the gaps
    are of the size the bounds were reasoned for (cost ~1e-7, log P a few 1e-5), not inflated by some instability."""
    _, _, ref, g = cases.forward_case(n, m, eps, iters)
    assert ref["its"] == g["its32"]
    if (n, m) != (1, 1):
        assert ref["its"] == iters
        assert ref["mask"].mean() > 0.05                        # enough of the plan is above the underflow cut
    assert g["cost"] < 5e-7 and g["logP"] < 1e-4 and g["col"] < 1e-5 and g["row"] < 1e-5, g


@pytest.mark.parametrize("tag", list(cases.VARIANTS))
def test_variant_cases_run_every_sweep(tag):
    _, _, ref, g = cases.variant_case(tag)
    assert ref["its"] == g["its32"] == 25
    assert g["cost"] < 5e-7 and g["gx"] < 1e-5 and g["gy"] < 1e-5, g


def test_l1_lattice_has_exact_zero_differences():
    x, y, ref, g = cases.l1_lattice_case()
    zero = (x[:, :, None, :] - y[:, None, :, :]) == 0
    assert zero.float().mean().item() >= 0.05
    assert ref["its"] == g["its32"] == 25
    # torch's |.| has gradient 0 at 0: the reference this case pins the kernel's choice to
    t = torch.zeros(3, dtype=torch.float64, requires_grad=True)
    (t.abs() ** 1).sum().backward()
    assert not t.grad.any()


@pytest.mark.parametrize("B,n,m,own_copy", cases.STOP_CASES)
def test_early_stop_threshold_sits_between_two_sweeps(B, n, m, own_copy):
    """thresh is the geometric mean of the float64 statistic after sweeps T - 1 and T; with a ratio of at least 1.5
    between the two, float32 noise (1e-6 relative) cannot move the stop by a sweep."""
    T_ = cases.STOP_T
    x, y, w, thresh, free, ref, g = cases.stop_case(B, n, m, own_copy)
    assert free[T_ - 2] / free[T_ - 1] >= 1.5
    assert all(s > thresh for s in free[:T_ - 1]) and free[T_ - 1] < thresh
    assert ref["its"] == g["its32"] == T_
    assert np.allclose(g["stats32"], ref["stats"], rtol=1e-3)
    # one sweep more is far outside the bound the GPU test applies: that comparison does resolve where the run stopped
    longer = sinkhorn_mirror.sinkhorn_costs(x.double(), y.double(), 0.5, T_ + 1, thresh=0.0)[0]
    assert cases.relmax(longer.numpy(), ref["cost"]) > 100 * cases.bound(g["cost"])
    if (n, m) == (40, 300) and not own_copy:                    # the figures this case was designed on
        assert abs(free[7] - 4.40e-2) < 5e-5 and abs(free[8] - 2.36e-2) < 5e-5
    if B > 64:                                                  # without the pairs from 64 on the run would stop at sweep 3
        head = sinkhorn_mirror.sinkhorn_costs(x[:64].double(), y[:64].double(), 0.5, 40, thresh=0.0, history=True)[4]
        assert head[2] * 64 / B < thresh / 4 and free[2] > 10 * thresh
    if own_copy:                                                # pair 0 holds a copy of its own source, the others do not
        assert torch.equal(y[0, :n], x[0]) and not torch.equal(y[1, :n], x[1])


# -------------------------------------------------------------------------------- conditions of the GPU Chamfer tests
def test_lattice_distances_are_exact_in_float32():
    for n, m in cases.CHAMFER_SHAPES:
        x, y, ref = cases.chamfer_case("lattice", n, m)
        assert np.array_equal(cases.sqdist(x.numpy(), y.numpy(), np.float32).astype(np.float64), ref["d"])
        assert np.array_equal(ref["d"] * 64, np.round(ref["d"] * 64))
        assert ref["d"].max() * 64 * max(n, m) < 2 ** 24          # sums over a whole cloud stay exact too


def test_lattice_clouds_have_ties_across_groups_and_tiles():
    """Largest shape: at least 30 % of all queries have a tied minimum, and among them the first two minimisers lie in
    different groups of four / different 1024-candidate tiles at least 20 times each.  At (257, 1027) the x queries (1027
    candidates) are tied 46 % of the time; the y queries see only 257 candidates, too sparse on the 17^3 lattice for
    more than 24 %, so the 30 % is asked of the x direction there."""
    n, m = cases.CHAMFER_SHAPES[1]
    _, _, ref = cases.chamfer_case("lattice", n, m)
    a, b = cases.tie_counts(ref["d"]), cases.tie_counts(ref["d"].transpose(0, 2, 1))
    assert (a[1] + b[1]) >= 0.30 * (a[0] + b[0])
    assert a[2] + b[2] >= 20 and a[3] + b[3] >= 20
    assert a[3] >= 20                                             # ... and in the direction with three tiles alone
    n, m = cases.CHAMFER_SHAPES[0]
    _, _, ref = cases.chamfer_case("lattice", n, m)
    a = cases.tie_counts(ref["d"])
    assert a[1] >= 0.30 * a[0] and a[2] >= 20


def test_random_clouds_float32_argmin_stays_within_the_allowance():
    """The allowance of the GPU test (at most 0.5 % of the indices differ from the float64 argmin, each within 1e-6
    relative of the minimum) holds for the float32 evaluation of the same definition in numpy."""
    for n, m in cases.CHAMFER_SHAPES:
        x, y, ref = cases.chamfer_case("random", n, m)
        d32 = cases.sqdist(x.numpy(), y.numpy(), np.float32)
        for axis, key in ((2, "nn_xy"), (1, "nn_yx")):
            idx = d32.argmin(axis)
            differ = idx != ref[key]
            assert differ.mean() <= 0.005
            at = np.take_along_axis(ref["d"], np.expand_dims(idx, axis), axis).squeeze(axis)
            best = ref["d"].min(axis)
            assert np.all(at - best <= 1e-6 * best)


def test_clustered_cloud_has_one_owner_of_every_query_and_no_near_ties():
    n, m = cases.CLUSTERED_SHAPE
    x, y, ref, _, gaps = cases.chamfer_grad_case("clustered", n, m)
    for b in range(2):
        assert np.bincount(ref["nn_xy"][b]).max() == n            # one y point owns all n x points
    # float32 evaluates a squared distance to ~3 * 2^-24 relative: the runner-up is far enough not to be confused
    for axis in (2, 1):
        two = np.sort(ref["d"], axis=axis).take([0, 1], axis=axis)
        lo, hi = two.take(0, axis=axis), two.take(1, axis=axis)
        assert ((hi - lo) / lo).min() > 1e-6
    assert max(gaps) < 1e-4 / cases.K                             # the 1e-4 ceiling is not what binds
