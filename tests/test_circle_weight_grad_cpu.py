"""The definition of the circle's gradients with respect to the weights, checked in float64 on the CPU:
the references of tests/helpers/circle_weight_grad_cases.py against central differences of the exact minimum over all
kinks, the finding that the reference's fixed-cut autograd is NOT that gradient, and the identities the kernels rely on."""
import numpy as np
import pytest
import torch

from helpers.circle_weight_grad_cases import (POWERS_CPU, SIZES_CPU, bisect_with_cut, brute_min, closed_form, coords,
                                              dyadic_weights, fixed_cut, float_weights, lambda_mix, level_median_grads,
                                              max_dev, prepare, weight_grad_rows)
from oracle import ref_mirror


def _row(n, m, seed=0):
    u, v = coords(n, m, seed=500 + n + m + seed, rows=1)
    a, b = float_weights(n, m, 77 + seed, False)
    return u[0].double().numpy(), v[0].double().numpy(), a.double().numpy(), b.double().numpy()


def _directions(rng, n, m, count):
    for _ in range(count):
        da, db = rng.standard_normal(n), rng.standard_normal(m)
        yield da - da.mean(), db - db.mean()                    # the totals stay 1


def _central_difference(u, v, a, b, p, da, db, h=1e-6):
    return (brute_min(u, v, a + h * da, b + h * db, p)[0] - brute_min(u, v, a - h * da, b - h * db, p)[0]) / (2 * h)


@pytest.mark.parametrize("n,m", SIZES_CPU)
@pytest.mark.parametrize("p", POWERS_CPU)
def test_closed_form_and_mix_against_central_differences(n, m, p):
    """both forms of the gradient, at the exact minimising kink and at the bisection's cut, against central differences
    of the brute-force minimum along directions that keep the totals: 1e-6 relative (measured <= 1e-9)"""
    u, v, a, b = _row(n, m)
    S = prepare(u, v, a, b)
    w_min, kink = brute_min(u, v, a, b, p)
    cost, cut = bisect_with_cut(u[None], v[None], a, b, p)
    # (the bisection ends on the minimising kink.  The weights are normalised in float32, so the two totals differ from 1
    #  and from each other by up to 6e-8, and Cost clips the levels in between: the values agree to that, not to 1e-16)
    assert abs(float(cost[0]) - w_min) <= 1e-7 * w_min
    rng = np.random.default_rng(n * m)
    forms = {"closed@kink": closed_form(S, kink, p), "mix@kink": lambda_mix(S, kink, p),
             "closed@bisection": closed_form(S, float(cut[0]), p), "mix@bisection": lambda_mix(S, float(cut[0]), p)}
    for da, db in _directions(rng, n, m, 4):
        fd = _central_difference(u, v, a, b, p, da, db)
        for name, (ga, gb) in forms.items():
            got = ga @ da + gb @ db
            assert abs(got - fd) <= 1e-6 * max(abs(fd), np.abs(ga).max()), (name, got, fd)


def test_fixed_cut_autograd_is_not_the_gradient():
    """float64 autograd through oracle.ref_mirror.circular_ot_bisect differentiates Cost at a fixed cut: on at least one
    of the cases it misses the same central differences by more than 1 %"""
    worst = 0.0
    for n, m in SIZES_CPU:
        for p in (1.5, 2, 3):
            u, v, a, b = _row(n, m)
            at, bt = torch.from_numpy(a).requires_grad_(), torch.from_numpy(b).requires_grad_()
            ref_mirror.circular_ot_bisect(torch.from_numpy(u)[None], torch.from_numpy(v)[None], p, at, bt).sum().backward()
            rng = np.random.default_rng(n * m)
            for da, db in _directions(rng, n, m, 2):
                fd = _central_difference(u, v, a, b, p, da, db)
                got = float(at.grad.numpy() @ da + bt.grad.numpy() @ db)
                worst = max(worst, abs(got - fd) / abs(fd))
    assert worst > 0.01, worst


@pytest.mark.parametrize("n,m", SIZES_CPU)
def test_mix_equals_closed_form(n, m):
    for p in POWERS_CPU:
        u, v, a, b = _row(n, m, seed=1)
        _, cut = bisect_with_cut(u[None], v[None], a, b, p)
        S = prepare(u, v, a, b)
        for x, y in zip(closed_form(S, float(cut[0]), p), lambda_mix(S, float(cut[0]), p)):
            assert max_dev(y, x) <= 1e-9, (n, m, p, max_dev(y, x))


@pytest.mark.parametrize("n,m,heavy", [(8, 8, False), (4, 8, False), (5, 5, True), (6, 4, True)])
def test_subgradient_inequality_on_ties(n, m, heavy):
    """exactly tied levels (uniform weights with n | m, integer weights over a power-of-two total, zero weights, one heavy
    atom): W has no gradient; the mix is a subgradient of the convex W"""
    u, v = coords(n, m, seed=40 + n + m, rows=1)
    u, v = u[0].double().numpy(), v[0].double().numpy()
    if heavy:
        a, b = [x.astype(np.float64) for x in dyadic_weights(n, m, seed=n + m, heavy=True)]
    else:
        a, b = np.full(n, 1.0 / n), np.full(m, 1.0 / m)
    rng = np.random.default_rng(3 * n + m)
    for p in POWERS_CPU:
        _, cut = bisect_with_cut(u[None], v[None], a, b, p)
        ga, gb = lambda_mix(prepare(u, v, a, b), float(cut[0]), p)
        assert np.isfinite(ga).all() and np.isfinite(gb).all()
        w0 = brute_min(u, v, a, b, p)[0]
        for _ in range(50):
            a2, b2 = rng.random(n) * rng.integers(0, 2, n) + 1e-3, rng.random(m) * rng.integers(0, 2, m) + 1e-3
            a2, b2 = a2 / a2.sum(), b2 / b2.sum()
            slack = brute_min(u, v, a2, b2, p)[0] - w0 - ga @ (a2 - a) - gb @ (b2 - b)
            assert slack >= -1e-12, (n, m, p, slack)


@pytest.mark.parametrize("n,m", SIZES_CPU)
def test_level_median_closed_form_equals_autograd(n, m):
    """H_k - S [k <= k*] in merged order, negated for the target side, is what autograd gives for the level-median formula"""
    u, v, a, b = _row(n, m, seed=2)
    ref_a, ref_b = level_median_grads(u[None], v[None], a, b)
    merged = np.concatenate([u, v])
    order = np.argsort(merged, kind="stable")
    signed = np.concatenate([a, -b])[order]
    level = np.cumsum(signed)
    gaps = np.diff(merged[order], append=1.0)
    by_level = np.argsort(level, kind="stable")
    mass = np.cumsum(gaps[by_level]) - 0.5
    kstar = by_level[np.argmax(mass >= 0)] if (mass >= 0).any() else by_level[0]
    sigma = np.sign(level - level[kstar])
    H = np.cumsum((gaps * sigma)[::-1])[::-1]
    D = np.zeros(n + m)
    D[order] = H - H[0] * (np.arange(n + m) <= kstar)
    ga, gb = D[:n], -D[n:]
    assert max_dev(ga - a @ ga / a.sum(), ref_a[0]) <= 1e-12 and max_dev(gb - b @ gb / b.sum(), ref_b[0]) <= 1e-12


@pytest.mark.parametrize("n,m", [(5, 7), (1, 9), (12, 1)])
def test_gauge(n, m):
    """sum_i a_i G_i = 0 per side, a side of one atom is exactly 0, and an atom of weight 0 changes nothing else"""
    u, v, a, b = _row(n, m, seed=3)
    for p in POWERS_CPU:
        ga, gb = weight_grad_rows(u[None], v[None], a, b, p)
        assert abs(a @ ga[0]) <= 1e-14 and abs(b @ gb[0]) <= 1e-14
        if n == 1:
            assert not ga.any()
        if m == 1:
            assert not gb.any()
        up, ap = np.concatenate([u, [0.37]]), np.concatenate([a, [0.0]])
        gpa, gpb = weight_grad_rows(up[None], v[None], ap, b, p)
        assert max_dev(gpa[0][:n], ga[0]) <= 1e-9 and max_dev(gpb[0], gb[0]) <= 1e-9


def test_slope_is_minus_the_target_jumps():
    """fixed_cut's slope is the reference's dCost on the same side"""
    u, v, a, b = _row(9, 4, seed=4)
    S = prepare(u, v, a, b)
    t = lambda x: torch.from_numpy(x)[None]
    for theta in (0.137, -0.42, 0.8):
        dp, dm = ref_mirror.cut_slopes(torch.tensor([[theta]], dtype=torch.float64), t(S["us"]), t(S["vs"]), t(S["A"]), t(S["B"]), 2)
        assert abs(fixed_cut(S, theta, 2, True)[2] - float(dp)) <= 1e-12
        assert abs(fixed_cut(S, theta, 2, False)[2] - float(dm)) <= 1e-12
