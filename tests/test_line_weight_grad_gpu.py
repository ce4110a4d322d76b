"""GPU checks of the line transport's gradients with respect to the weights (csrc/shw_line_ot.hip line_ot_pot_kernel and
line_weight_reduce_kernel; line_ot.py weight_grad=True) against the references of tests/helpers/line_weight_grad_cases.py.

Bounds.  A gradient is compared with the float64 reference on the same float32 inputs, per side, on
max |error| / max |reference entry|; the bound is 4 x the deviation of the FLOAT32 restatement from the float64 one on the
same inputs, computed here, with a floor of 1e-6.  With float weights (no two CDF ends coincide) the reference is autograd
of the weight-differentiable quantile merge; with integer weights (exact ties, zero weights) the gradient does not exist,
the kernel returns the subgradient of the documented tie rule, and the reference is the numpy walk with that rule, the
float32 restatement being the same walk with float32 costs and sums.  A side of one atom is exactly 0.

Every call here passes weight_grad=True, a keyword the functions did not have before: without the feature each of these
tests fails with a TypeError.

Measured on MI355X (worst over the size list, p in {1, 2, 3, 1.5}): rows form 2.7e-7 up to (1000,1536)
and 4.2e-7 at (4096,4095), where the float32 restatement itself is up to 1e-4 away; sides of one atom exactly 0; integer
weights with ties against the walk 3.8e-7 (bounds 1.0e-6 to 1.9e-6); sum a grad / sum |a grad| 3.6e-8; zero-weight padding
1.4e-7; fused form: weights 6.1e-7, values 9.6e-6 at D = 64 (bound 4e-5: key rounding).
"""
import functools

import numpy as np
import pytest
import torch

from helpers.compare import grad_close
from helpers.line_ot_cases import ROWS, rows
from helpers.line_weight_grad_cases import (FLOOR, POWERS, SIZES_GPU, TIE_SIZES, autograd_weight_grads, float_weights,
                                            max_dev, quantile_merge_w, row_case, tie_weights, walk_rows)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def shw():
    import shw_amd
    shw_amd._lib.load()
    return shw_amd


def gpu_row_weight_grads(shw, u, v, p, a, b):
    """gradients of sum_rows line_ot_rows w.r.t. the weights alone -> two float64 arrays"""
    ad, bd = a.to(DEV).requires_grad_(), b.to(DEV).requires_grad_()
    shw.line_ot_rows(u.to(DEV), v.to(DEV), p, ad, bd, weight_grad=True).sum().backward()
    assert ad.grad.shape == a.shape and bd.grad.shape == b.shape
    return ad.grad.cpu().double().numpy(), bd.grad.cpu().double().numpy()


@pytest.mark.parametrize("n,m", SIZES_GPU)
@pytest.mark.parametrize("per_row", [False, True])
def test_rows_weight_gradients(shw, n, m, per_row):
    for p in POWERS:
        u, v, a, b, ref, bounds = row_case(n, m, p, per_row)
        got = gpu_row_weight_grads(shw, u, v, p, a, b)
        for side, count, g, r, bound in zip("ab", (n, m), got, ref, bounds):
            worst = max_dev(g, r)
            print(f"rows {n}x{m} per_row={per_row} p={p} d{side}: gpu {worst:.2e} bound {bound:.2e}")
            if count == 1:
                assert not g.any(), (side, g)                 # one atom: its weight is all of the mass, whatever it is
            assert worst <= bound, (n, m, per_row, p, side, worst, bound)


@functools.lru_cache(maxsize=None)
def tie_case(n, m):
    u, v = rows(n, m, seed=7000 + n + m)
    ab = [tie_weights(n, m, seed=100 * r + n + m, heavy=True) for r in range(ROWS)]
    return u, v, np.stack([x[0] for x in ab]), np.stack([x[1] for x in ab])


@pytest.mark.parametrize("n,m", TIE_SIZES)
def test_integer_weights_with_ties_and_zeros(shw, n, m):
    """integer weights 0..3 with equal totals, one atom of v with 90 % of its side's mass: elementwise against the walk
    with the documented tie rule, and the subgradient inequality in float64 for random weights of the same totals with
    the tolerance bound * max |g| * ||a' - a||_1"""
    u, v, a, b = tie_case(n, m)
    assert (a == 0).any() and (b == 0).any()
    rng = np.random.default_rng(n + m)
    ud, vd = u.double(), v.double()
    at, bt = torch.from_numpy(a), torch.from_numpy(b)
    for p in POWERS:
        ref = walk_rows(u.numpy(), v.numpy(), p, a, b)
        f32 = walk_rows(u.numpy(), v.numpy(), p, a, b, cost_dtype=np.float32)
        got = gpu_row_weight_grads(shw, u, v, p, at.float(), bt.float())
        bounds = [max(4.0 * max_dev(f, r), FLOOR) for f, r in zip(f32, ref)]
        for side, g, r, bound in zip("ab", got, ref, bounds):
            print(f"ties {n}x{m} p={p} d{side}: gpu {max_dev(g, r):.2e} bound {bound:.2e}")
            assert max_dev(g, r) <= bound, (n, m, p, side, max_dev(g, r), bound)
        w0 = quantile_merge_w(ud, vd, p, at, bt)
        for _ in range(6):
            a2 = rng.random((ROWS, n)) * rng.integers(0, 2, (ROWS, n)) + 1e-3 * rng.random((ROWS, n))
            b2 = rng.random((ROWS, m)) * rng.integers(0, 2, (ROWS, m)) + 1e-3 * rng.random((ROWS, m))
            a2 *= a.sum(-1, keepdims=True) / a2.sum(-1, keepdims=True)
            b2 *= b.sum(-1, keepdims=True) / b2.sum(-1, keepdims=True)
            w1 = quantile_merge_w(ud, vd, p, torch.from_numpy(a2), torch.from_numpy(b2))
            lin = (got[0] * (a2 - a)).sum(-1) + (got[1] * (b2 - b)).sum(-1)
            tol = (bounds[0] * np.abs(got[0]).max(-1) * np.abs(a2 - a).sum(-1)
                   + bounds[1] * np.abs(got[1]).max(-1) * np.abs(b2 - b).sum(-1))
            slack = (w1 - w0).numpy() - lin
            assert (slack >= -tol).all(), (n, m, p, slack, tol)


@pytest.mark.parametrize("n,m", [(65, 64), (257, 96), (1000, 1536), (4096, 4095)])
def test_weights_times_gradient_sums_to_zero(shw, n, m):
    """the cost is homogeneous of degree 0 in each weight vector: sum_i a_i grad_i = 0, within the bound relative to
    sum_i |a_i grad_i|, per row and side"""
    for p in POWERS:
        u, v, a, b, _, bounds = row_case(n, m, p, True)
        got = gpu_row_weight_grads(shw, u, v, p, a, b)
        for w, g, bound in zip((a, b), got, bounds):
            prod = w.double().numpy() * g
            rel = np.abs(prod.sum(-1)) / np.abs(prod).sum(-1)
            print(f"euler {n}x{m} p={p}: {rel.max():.2e} bound {bound:.2e}")
            assert (rel <= bound).all(), (n, m, p, rel, bound)


def test_zero_weight_padding_leaves_the_other_gradients(shw):
    """atoms of weight 0 (any key) appended to both sides: the entries of the atoms that were there stay within the bound
    of the reference without padding.  The bound is the rule's, on the inputs the kernel sees: the padding keys lie up to
    three times as far out as the data, so costs up to 3^p as large pass through the sums, and the float32 restatement on
    the padded inputs deviates by up to 1.7e-6 on the entries compared here (3e-7 without the padding).  The kernel sums
    its jumps in double, where a padding atom's cost cancels exactly: 1.4e-7 measured."""
    n, m, pad_n, pad_m = 130, 129, 37, 11
    g = torch.Generator().manual_seed(8)
    for p in POWERS:
        u, v, a, b, ref, _ = row_case(n, m, p, True)
        up = torch.cat([u, torch.randn(ROWS, pad_n, generator=g) * 3], -1)
        vp = torch.cat([v, torch.randn(ROWS, pad_m, generator=g) * 3], -1)
        ap = torch.cat([a, torch.zeros(ROWS, pad_n)], -1)
        bp = torch.cat([b, torch.zeros(ROWS, pad_m)], -1)
        r64 = autograd_weight_grads(up, vp, p, ap, bp, torch.float64)
        f32 = autograd_weight_grads(up, vp, p, ap, bp, torch.float32)
        ga, gb = gpu_row_weight_grads(shw, up, vp, p, ap, bp)
        assert np.isfinite(ga).all() and np.isfinite(gb).all()
        for got, r, rp, fp in ((ga[:, :n], ref[0], r64[0][:, :n], f32[0][:, :n]),
                               (gb[:, :m], ref[1], r64[1][:, :m], f32[1][:, :m])):
            assert max_dev(rp, r) <= 1e-12                      # in float64 the padding changes nothing
            bound = max(4.0 * max_dev(fp, rp), FLOOR)
            print(f"padding p={p}: gpu {max_dev(got, r):.2e} bound {bound:.2e}")
            assert max_dev(got, r) <= bound, (p, max_dev(got, r), bound)


@pytest.mark.parametrize("n,m", [(130, 129), (257, 96), (2048, 1536), (4096, 4095)])
def test_cost_and_value_gradients_are_the_bits_of_the_call_without(shw, n, m):
    u, v = rows(n, m, seed=8000 + n + m)
    for per_row in (False, True):
        a, b = float_weights(n, m, 29, per_row)
        for p in (2, 1.5, 1):
            base = [t.to(DEV).requires_grad_() for t in (u, v)]
            c0 = shw.line_ot_rows(*base, p, a.to(DEV), b.to(DEV))
            c0.sum().backward()
            full = [t.to(DEV).requires_grad_() for t in (u, v, a, b)]
            c1 = shw.line_ot_rows(full[0], full[1], p, full[2], full[3], weight_grad=True)
            c1.sum().backward()
            assert torch.equal(c0.detach(), c1.detach())
            assert torch.equal(base[0].grad, full[0].grad) and torch.equal(base[1].grad, full[1].grad)
            # weights alone (no coefficient rows, pass V still runs) and one side alone: the same bits again
            ga, gb = gpu_row_weight_grads(shw, u, v, p, a, b)
            assert np.array_equal(ga, full[2].grad.cpu().double().numpy())
            assert np.array_equal(gb, full[3].grad.cpu().double().numpy())
            bd = b.to(DEV).requires_grad_()
            shw.line_ot_rows(u.to(DEV), v.to(DEV), p, a.to(DEV), bd, weight_grad=True).sum().backward()
            assert torch.equal(bd.grad, full[3].grad)
            # the keyword alone does nothing
            plain = shw.line_ot_rows(u.to(DEV), v.to(DEV), p, a.to(DEV), b.to(DEV), weight_grad=True)
            assert torch.equal(plain, c0.detach())


# ------------------------------------------------------------------------------------------------ fused projection
def fused_inputs(B, n, m, D, L, seed):
    g = torch.Generator().manual_seed(seed)
    xs = torch.randn(B, n, D, generator=g)
    xt = torch.randn(B, m, D, generator=g) + 0.5
    th = torch.randn(L, D, generator=g)
    th = th / th.norm(dim=-1, keepdim=True)
    wl = torch.rand(B, L, generator=g) + 0.5                    # upstream weights of the slices
    return xs, xt, th, wl


def fused_reference(xs, xt, th, p, a, b, dtype):
    ks = torch.einsum("bnd,ld->bln", xs.to(dtype), th.to(dtype))
    kt = torch.einsum("bmd,ld->blm", xt.to(dtype), th.to(dtype))
    return quantile_merge_w(ks, kt, p, a if a.dim() == 1 else a.unsqueeze(1), b if b.dim() == 1 else b.unsqueeze(1),
                            dtype=dtype)


def reference_grads(tensors, wl, p, dtype, which):
    """gradients of sum(wl * fused_reference) w.r.t. tensors[k] for k in `which` (xs, xt, th, a, b)"""
    leaves = [t.clone().requires_grad_(k in which) for k, t in enumerate(tensors)]
    (fused_reference(*leaves[:3], p, leaves[3], leaves[4], dtype) * wl.to(dtype)).sum().backward()
    return [leaves[k].grad.double().numpy() for k in which]


@pytest.mark.parametrize("D", [3, 64])
@pytest.mark.parametrize("n,m", [(130, 129), (257, 96)])
@pytest.mark.parametrize("per_pair", [False, True])
def test_fused_weight_gradients(shw, D, n, m, per_pair):
    B, L = 2, 5
    xs, xt, th, wl = fused_inputs(B, n, m, D, L, seed=90 + D + n)
    a, b = float_weights(n, m, 31, per_pair, count=B)
    tensors = (xs, xt, th, a, b)
    names = ("xs", "xt", "thetas", "a", "b")
    for p in (2, 3, 1.5, 1):
        for which in ((3, 4), (0, 1, 2, 3, 4)):                 # weights only; clouds, directions and weights together
            ref = reference_grads(tensors, wl, p, torch.float64, which)
            f32 = reference_grads(tensors, wl, p, torch.float32, which)
            ld = [t.to(DEV).requires_grad_(k in which) for k, t in enumerate(tensors)]
            cost = shw.esw_slice_costs(ld[0], ld[1], ld[2], p, ld[3], ld[4], weight_grad=True)
            assert cost.shape == (B, L)
            (cost * wl.to(DEV)).sum().backward()
            for k, r, f in zip(which, ref, f32):
                got = ld[k].grad.cpu().double().numpy()
                assert got.shape == tuple(tensors[k].shape)
                if p == 1 and k < 3:
                    grad_close(got, r, max_outside=0, label=f"weight_grad fused p=1 D={D} {names[k]}")
                    continue
                bound = max(4.0 * max_dev(f, r), FLOOR)
                print(f"fused D={D} {n}x{m} per_pair={per_pair} p={p} d{names[k]}: "
                      f"gpu {max_dev(got, r):.2e} bound {bound:.2e}")
                assert max_dev(got, r) <= bound, (names[k], p, which, max_dev(got, r), bound)
            if len(which) == 5:                                 # cost and value gradients: the bits of the call without
                l0 = [t.to(DEV).requires_grad_(k < 3) for k, t in enumerate(tensors)]
                c0 = shw.esw_slice_costs(l0[0], l0[1], l0[2], p, l0[3], l0[4])
                (c0 * wl.to(DEV)).sum().backward()
                assert torch.equal(c0.detach(), cost.detach())
                for k in range(3):
                    assert torch.equal(l0[k].grad, ld[k].grad), names[k]


def test_weighted_distance_passes_the_gradient_on(shw):
    n, m, D, L, p = 300, 200, 3, 16, 2
    g = torch.Generator().manual_seed(120)
    xs, xt = torch.randn(n, D, generator=g), torch.randn(m, D, generator=g) + 0.5
    a, b = float_weights(n, m, 13, False)
    torch.manual_seed(5)
    th = shw.rand_projections(D, L)
    leaves = [a.clone().requires_grad_(), b.clone().requires_grad_()]
    ref = fused_reference(xs[None], xt[None], th, p, *leaves, torch.float64).mean() ** (1.0 / p)
    ref.backward()
    l32 = [a.clone().requires_grad_(), b.clone().requires_grad_()]
    (fused_reference(xs[None], xt[None], th, p, *l32, torch.float32).mean() ** (1.0 / p)).backward()
    ad, bd = a.to(DEV).requires_grad_(), b.to(DEV).requires_grad_()
    torch.manual_seed(5)
    got = shw.weighted_sliced_wasserstein_distance(xs.to(DEV), xt.to(DEV), L, p, DEV, ad, bd, weight_grad=True)
    got.backward()
    assert abs(got.item() - ref.item()) <= 1e-5 * ref.item()
    for gd, r, f in zip((ad, bd), leaves, l32):
        bound = max(4.0 * max_dev(f.grad, r.grad), FLOOR)
        assert max_dev(gd.grad.cpu(), r.grad) <= bound, (max_dev(gd.grad.cpu(), r.grad), bound)


# ------------------------------------------------------------------------------------------------ determinism
@pytest.mark.parametrize("n,m", [(257, 96), (2048, 1536)])
def test_two_calls_give_the_same_bits(shw, n, m):
    u, v = rows(n, m, seed=130)
    xs, xt, th, wl = fused_inputs(2, n, m, 3, 4, seed=131)
    for per_row in (False, True):
        a, b = float_weights(n, m, 14, per_row, count=ROWS)
        outs = []
        for _ in range(2):
            lr = [t.to(DEV).requires_grad_() for t in (u, v, a, b)]
            shw.line_ot_rows(lr[0], lr[1], 1.5, lr[2], lr[3], weight_grad=True).sum().backward()
            lf = [t.to(DEV).requires_grad_() for t in (xs, xt, th, a[:2] if per_row else a, b[:2] if per_row else b)]
            (shw.esw_slice_costs(lf[0], lf[1], lf[2], 2, lf[3], lf[4], weight_grad=True) * wl.to(DEV)).sum().backward()
            outs.append([t.grad for t in lr + lf])
        for x, y in zip(*outs):
            assert torch.equal(x, y)


def test_shared_weights_over_many_rows_use_the_two_stage_reduction(shw):
    """200 rows with shared weights: four groups of 64 rows and a second stage; against the float64 reference"""
    n, m, count, p = 48, 36, 200, 2
    u, v = rows(n, m, seed=140, count=count)
    a, b = float_weights(n, m, 15, False)
    g = torch.Generator().manual_seed(16)
    up = torch.rand(count, generator=g) + 0.5
    leaves = [a.clone().requires_grad_(), b.clone().requires_grad_()]
    (quantile_merge_w(u, v, p, *leaves) * up).sum().backward()
    l32 = [a.clone().requires_grad_(), b.clone().requires_grad_()]
    (quantile_merge_w(u, v, p, *l32, dtype=torch.float32) * up).sum().backward()
    ad, bd = a.to(DEV).requires_grad_(), b.to(DEV).requires_grad_()
    (shw.line_ot_rows(u.to(DEV), v.to(DEV), p, ad, bd, weight_grad=True) * up.to(DEV)).sum().backward()
    for gd, r, f in zip((ad, bd), leaves, l32):
        bound = max(4.0 * max_dev(f.grad, r.grad), FLOOR)
        assert max_dev(gd.grad.cpu(), r.grad) <= bound, (max_dev(gd.grad.cpu(), r.grad), bound)
