"""CPU checks of the line transport's gradients with respect to the weights (csrc/shw_line_ot.hip line_ot_pot_kernel,
line_ot.py weight_grad=True): the two references of tests/helpers/line_weight_grad_cases.py agree where the gradient
exists, the walk's tie rule gives a subgradient where it does not, the boundary carries the new entries and they refuse
bad arguments without a GPU, and the default call still refuses a weight that requires grad."""
import inspect
import os
import re

import numpy as np
import pytest
import torch

from helpers.line_ot_cases import rows
from helpers.line_weight_grad_cases import (POWERS, SIZES_CPU, autograd_weight_grads, float_weights, max_dev,
                                            potentials_walk, quantile_merge_w, tie_weights)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ["shw_line_rows_forward_pot", "shw_line_esw_forward_pot", "shw_line_weight_grads",
           "shw_line_weight_grads_workspace_bytes"]
NAMES = ["line_ot_rows", "esw_slice_costs", "weighted_sliced_wasserstein_distance"]


@pytest.fixture(scope="module")
def shw():
    import shw_amd
    if not os.path.exists(shw_amd._lib.LIB_PATH):
        shw_amd._lib.build()
    return shw_amd


def one_row(n, m, seed):
    u, v = rows(n, m, seed=seed, count=1)
    a, b = float_weights(n, m, seed + 1, False)
    return u[0].double(), v[0].double(), a.double(), b.double()


@pytest.mark.parametrize("n,m", SIZES_CPU)
def test_walk_agrees_with_autograd_of_the_float64_merge(n, m):
    """tie-free float weights: max |error| / max |entry| over both sides <= 1e-12 (measured: 4e-16 at worst)"""
    u, v, a, b = one_row(n, m, seed=n * 11 + m)
    for p in POWERS:
        ra, rb = autograd_weight_grads(u, v, p, a, b, torch.float64)
        ga, gb, _, _ = potentials_walk(u.numpy(), v.numpy(), p, a.numpy(), b.numpy())
        scale = max(np.abs(ra).max(), np.abs(rb).max(), 1e-300)
        worst = max(np.abs(ga - ra).max(), np.abs(gb - rb).max()) / scale
        print(f"{n}x{m} p={p}: {worst:.1e}")
        assert worst <= 1e-12, (n, m, p, worst)


@pytest.mark.parametrize("n,m", SIZES_CPU)
def test_invariants_of_the_walk(n, m):
    """sum_i a_i grad_i = 0 on each side (degree 0 in each weight vector); sum abar f + sum bbar g + c_last = cost; a side
    of one atom gets exactly 0"""
    u, v, a, b = one_row(n, m, seed=n * 13 + m)
    for p in POWERS:
        ga, gb, dual, c_last = potentials_walk(u.numpy(), v.numpy(), p, a.numpy(), b.numpy())
        cost = quantile_merge_w(u, v, p, a, b).item()
        for w, g in ((a.numpy(), ga), (b.numpy(), gb)):
            assert abs((w * g).sum()) <= 1e-12 * max(np.abs(w * g).sum(), 1e-300) + 1e-15
        assert abs(dual + c_last - cost) <= 1e-12 * max(abs(cost), 1.0)
        if n == 1:
            assert ga[0] == 0.0
        if m == 1:
            assert gb[0] == 0.0


@pytest.mark.parametrize("n,m", [(2, 3), (7, 5), (48, 36), (65, 64), (257, 96)])
@pytest.mark.parametrize("heavy", [False, True])
def test_tie_rule_gives_a_subgradient(n, m, heavy):
    """integer weights 0..3 with equal totals (exact ties between the CDFs, atoms of weight 0):
    W(a', b') >= W(a, b) + <g_a, a' - a> + <g_b, b' - b> - 1e-9 for random a', b' >= 0 with the same totals"""
    rng = np.random.default_rng(n * 17 + m)
    u, v = rows(n, m, seed=n * 19 + m, count=1)
    u, v = u[0].double(), v[0].double()
    a, b = tie_weights(n, m, seed=n + m, heavy=heavy)
    for p in POWERS:
        ga, gb, _, _ = potentials_walk(u.numpy(), v.numpy(), p, a, b)
        w0 = quantile_merge_w(u, v, p, torch.from_numpy(a), torch.from_numpy(b)).item()
        for _ in range(12):
            a2 = rng.random(n) * rng.integers(0, 2, n) + 1e-3 * rng.random(n)
            b2 = rng.random(m) * rng.integers(0, 2, m) + 1e-3 * rng.random(m)
            a2 *= a.sum() / a2.sum()
            b2 *= b.sum() / b2.sum()
            w1 = quantile_merge_w(u, v, p, torch.from_numpy(a2), torch.from_numpy(b2)).item()
            slack = w1 - w0 - (ga * (a2 - a)).sum() - (gb * (b2 - b)).sum()
            assert slack >= -1e-9, (n, m, p, heavy, slack)


def test_zero_weight_atom_gets_the_right_derivative():
    """an atom of weight 0: its entry is the rate at which the cost changes when it gains mass"""
    u, v, a, b = one_row(48, 36, seed=77)
    a = a.clone()
    a[5] = 0.0
    for p in POWERS:
        ga, _, _, _ = potentials_walk(u.numpy(), v.numpy(), p, a.numpy(), b.numpy())
        eps = 1e-7
        a2 = a.clone()
        a2[5] = eps
        rate = (quantile_merge_w(u, v, p, a2, b).item() - quantile_merge_w(u, v, p, a, b).item()) / eps
        assert abs(rate - ga[5]) <= 1e-5 * max(np.abs(ga).max(), 1e-300), (p, rate, ga[5])


def test_float32_walk_is_close_to_the_float64_walk():
    """the float32 form of the walk (the tie tests' bound on the GPU comes from it) is the same walk: a potential is a
    running sum of at most n + m jumps, each of them two rounded costs, so it stays within 2 (n + m) 2^-24 of the scale"""
    n, m = 257, 96
    u, v, a, b = one_row(n, m, seed=5)
    for p in POWERS:
        r = potentials_walk(u.numpy(), v.numpy(), p, a.numpy(), b.numpy())
        f = potentials_walk(u.numpy(), v.numpy(), p, a.numpy(), b.numpy(), cost_dtype=np.float32)
        assert max(max_dev(f[0], r[0]), max_dev(f[1], r[1])) <= 2 * (n + m) * 2.0 ** -24


def test_header_loader_and_package_carry_the_new_names(shw):
    text = open(os.path.join(ROOT, "include", "shw.h")).read()
    assert "ON EQUAL LEVELS THE" in text and "weight 0 gets the potential" in text      # the tie and zero-weight rules
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(shw_[a-z0-9_]+)\s*\(", text))
    lib = shw._lib.load()
    for name in ENTRIES:
        assert name in declared, name
        assert name in shw._lib.EXPORTED_SYMBOLS, name
        assert hasattr(lib, name), name
    for name in NAMES:
        sig = inspect.signature(getattr(shw, name))
        assert sig.parameters["weight_grad"].default is False, name


def test_new_entries_refuse_bad_arguments_without_a_gpu(shw):
    lib = shw._lib.load()
    P = 4096            # any non-null value: every call below is refused before a pointer is read

    def rows_pot(u=P, v=P, rows=1, n=8, m=8, p=2.0, wu=P, wv=P, su=0, sv=0, cost=P, cu=None, cv=None, pu=P, pv=P):
        return lib.shw_line_rows_forward_pot(u, v, rows, n, m, p, wu, wv, su, sv, cost, cu, cv, pu, pv, None)

    def esw_pot(xs=P, xt=P, th=P, pairs=1, n=8, m=8, dim=3, slices=4, stride=0, p=2.0, wu=P, wv=P, su=0, sv=0, cost=P,
                cs=None, ct=None, pu=P, pv=P):
        return lib.shw_line_esw_forward_pot(xs, xt, th, pairs, n, m, dim, slices, stride, p, wu, wv, su, sv, cost, cs, ct,
                                            pu, pv, None)

    # a potential row asked for a side without weights
    assert rows_pot(wu=None) == 1 and rows_pot(wv=None) == 1
    assert esw_pot(wu=None) == 1 and esw_pot(wv=None) == 1
    # null required pointers
    assert rows_pot(u=None) == 1 and rows_pot(v=None) == 1 and rows_pot(cost=None) == 1
    assert esw_pot(xs=None) == 1 and esw_pot(xt=None) == 1 and esw_pot(th=None) == 1 and esw_pot(cost=None) == 1
    # the size limits of the entries without potentials
    for n, m in ((0, 8), (8, 0), (4097, 8), (8, 4097)):
        assert rows_pot(n=n, m=m) == 1 and esw_pot(n=n, m=m) == 1
    assert rows_pot(p=0.5) == 1 and rows_pot(rows=-1) == 1 and rows_pot(cu=P) == 1
    assert rows_pot(su=7) == 1 and rows_pot(wv=P, sv=7) == 1
    assert esw_pot(dim=0) == 1 and esw_pot(dim=65) == 1 and esw_pot(pairs=65536) == 1 and esw_pot(stride=11) == 1
    # nothing to do: no launch, success; one side's row alone is fine
    assert rows_pot(rows=0) == 0 and rows_pot(rows=0, wv=None, pv=None) == 0 and esw_pot(pairs=0) == 0
    # the reduction
    assert lib.shw_line_weight_grads(None, P, 1, 4, 8, 0, None, P, None) == 1
    assert lib.shw_line_weight_grads(P, None, 1, 4, 8, 0, None, P, None) == 1
    assert lib.shw_line_weight_grads(P, P, 1, 4, 8, 0, None, None, None) == 1
    for count in (0, 4097):
        assert lib.shw_line_weight_grads(P, P, 1, 4, count, 0, None, P, None) == 1
    assert lib.shw_line_weight_grads(P, P, 65536, 4, 8, 0, None, P, None) == 1
    assert lib.shw_line_weight_grads(P, P, -1, 4, 8, 0, None, P, None) == 1
    assert lib.shw_line_weight_grads(P, P, 2, 512, 8, 1, None, P, None) == 1          # shared, 16 groups: needs a workspace
    assert lib.shw_line_weight_grads(P, P, 0, 4, 8, 1, None, P, None) == 0
    assert lib.shw_line_weight_grads_workspace_bytes(2, 512, 8, 1) == 16 * 8 * 4
    assert lib.shw_line_weight_grads_workspace_bytes(1, 64, 8, 1) == 0                # one group goes straight to grad
    assert lib.shw_line_weight_grads_workspace_bytes(2, 512, 8, 0) == 0


def test_default_call_still_refuses_a_weight_that_requires_grad(shw):
    w = torch.ones(8, requires_grad=True)
    with pytest.raises(ValueError, match="no gradient with respect to the weights"):
        shw.line_ot._check_weights("u_weights", w, 8, (2,), "(2, 8)")
    with pytest.raises(ValueError, match="weight_grad=True"):
        shw.line_ot._check_weights("u_weights", w, 8, (2,), "(2, 8)", False)
    # asked for: the same tensor gets as far as the device check (there is no CPU path)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        shw.line_ot._check_weights("u_weights", w, 8, (2,), "(2, 8)", True)
    assert "weight_grad=True" in shw.line_ot.__doc__
