"""GPU checks of the line transport (csrc/shw_line_ot.hip): line_ot_rows, esw_slice_costs and
weighted_sliced_wasserstein_distance against the float64 quantile merge of tests/helpers/line_ot_cases.py.

Bounds.  A value is compared with the float64 restatement on the same float32 inputs; the bound is 4 x the worst
relative deviation of the FLOAT32 CPU restatement from the float64 one over the same inputs, computed here, with a floor
of 1e-6 (16 ulp: the sum has non-negative terms with a handful of roundings each).  Gradients for p >= 2 use the same
rule on max |error| / max |reference entry|.  At p = 1 the gradient is a sum of +-delta and goes through grad_close with
the count outside the strict bound pinned: the rows' keys are the float32 inputs themselves, so no difference changes
sign between the kernel and float64, and the pinned count is 0.

Measured on MI355X (worst over the size list, p in {1, 2, 3, 1.5}): values 1.6e-7 uniform, 1.8e-7 with
float weights, 1.3e-7 with integer weights, 1.7e-6 fused (D = 64: key rounding); row gradients 2.2e-7 uniform, 1.9e-6
weighted; fused gradients 2.4e-6; p = 1: no gradient entry outside grad_close's strict bound, worst 1.9e-6 of the scale.
"""
import numpy as np
import pytest
import torch

from helpers.compare import grad_close
from helpers.line_ot_cases import POWERS, ROWS, SIZES, integer_weights, quantile_merge, rel_dev, replication, rows

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FLOOR = 1e-6


@pytest.fixture(scope="module")
def shw():
    import shw_amd
    shw_amd._lib.load()
    return shw_amd


def bound_from(f32, f64):
    return max(4.0 * rel_dev(f32, f64), FLOOR)


def float_weights(n, m, seed, per_row):
    g = torch.Generator().manual_seed(seed)
    shape = (ROWS,) if per_row else ()
    return torch.rand(shape + (n,), generator=g) + 0.05, torch.rand(shape + (m,), generator=g) + 0.05


def dev(t):
    return None if t is None else t.to(DEV)


def check_values(shw, u, v, a, b, label):
    for p in POWERS:
        ref = quantile_merge(u, v, p, a, b)
        bound = bound_from(quantile_merge(u, v, p, a, b, dtype=torch.float32), ref)
        got = shw.line_ot_rows(u.to(DEV), v.to(DEV), p, dev(a), dev(b)).cpu()
        worst = rel_dev(got, ref)
        print(f"{label} p={p}: gpu {worst:.2e} bound {bound:.2e}")
        assert worst <= bound, (label, p, worst, bound)


@pytest.mark.parametrize("n,m", SIZES)
def test_uniform_values(shw, n, m):
    u, v = rows(n, m, seed=1000 + n + m)
    check_values(shw, u, v, None, None, f"uniform {n}x{m}")


@pytest.mark.parametrize("n,m", SIZES)
@pytest.mark.parametrize("per_row", [False, True])
def test_weighted_values(shw, n, m, per_row):
    u, v = rows(n, m, seed=2000 + n + m)
    a, b = float_weights(n, m, 3, per_row)
    check_values(shw, u, v, a, b, f"weighted {n}x{m} per_row={per_row}")


@pytest.mark.parametrize("n,m", [(48, 36), (65, 64), (257, 96), (1000, 1536), (2048, 1536)])
@pytest.mark.parametrize("heavy", [False, True])
def test_integer_weights_against_replication(shw, n, m, heavy):
    """integer weights with equal totals; `heavy`: one v atom holds 90 % of the mass, so its owner's walk spans the u
    atoms of many lanes.  Checked against the restatement (value bound) and against replicated atoms (same bound)."""
    u, v = rows(n, m, seed=3000 + n + m)
    ku, kv = integer_weights(n, m, seed=17, heavy=heavy)
    a, b = torch.from_numpy(ku).float(), torch.from_numpy(kv).float()
    check_values(shw, u, v, a, b, f"integer {n}x{m} heavy={heavy}")
    for p in (1, 2):
        got = shw.line_ot_rows(u.to(DEV), v.to(DEV), p, a.to(DEV), b.to(DEV)).cpu().double().numpy()
        rep = np.array([replication(u[r].numpy(), v[r].numpy(), p, ku, kv) for r in range(u.shape[0])])
        bound = bound_from(quantile_merge(u, v, p, a, b, dtype=torch.float32), torch.from_numpy(rep))
        assert rel_dev(got, rep) <= bound, (p, rel_dev(got, rep), bound)


def rows_grads(shw, u, v, p, a, b):
    ud, vd = u.to(DEV).requires_grad_(), v.to(DEV).requires_grad_()
    shw.line_ot_rows(ud, vd, p, dev(a), dev(b)).sum().backward()
    return ud.grad.cpu(), vd.grad.cpu()


def ref_grads(u, v, p, a, b, dtype):
    ur, vr = u.clone().requires_grad_(), v.clone().requires_grad_()
    quantile_merge(ur, vr, p, a, b, dtype=dtype).sum().backward()
    return ur.grad, vr.grad


def grad_dev(got, ref):
    return float((got.double() - ref.double()).abs().max() / ref.double().abs().max())


@pytest.mark.parametrize("n,m", [(1, 1), (65, 64), (48, 36), (100, 1), (257, 96), (1000, 1536), (4096, 4095)])
@pytest.mark.parametrize("weighted", [False, True])
def test_row_gradients(shw, n, m, weighted):
    u, v = rows(n, m, seed=4000 + n + m)
    a, b = float_weights(n, m, 5, True) if weighted else (None, None)
    for p in (2, 3, 1.5, 1):
        got = rows_grads(shw, u, v, p, a, b)
        ref = ref_grads(u, v, p, a, b, torch.float64)
        if p == 1:
            for g, r in zip(got, ref):
                grad_close(g.numpy(), r.numpy(), max_outside=0, label=f"line_ot_rows p=1 {n}x{m} w={weighted}")
            continue
        f32 = ref_grads(u, v, p, a, b, torch.float32)
        for g, r, f in zip(got, ref, f32):
            bound = max(4.0 * grad_dev(f, r), FLOOR)
            print(f"grad {n}x{m} w={weighted} p={p}: gpu {grad_dev(g, r):.2e} bound {bound:.2e}")
            assert grad_dev(g, r) <= bound, (n, m, p, grad_dev(g, r), bound)


def test_zero_weight_tail_padding(shw):
    """padding atoms of weight 0 (any key) change neither cost nor gradients, and get exact zeros"""
    n, m, pad_n, pad_m = 130, 96, 37, 11
    u, v = rows(n, m, seed=51)
    a, b = float_weights(n, m, 7, True)
    g = torch.Generator().manual_seed(8)
    up = torch.cat([u, torch.randn(ROWS, pad_n, generator=g) * 3], -1)
    vp = torch.cat([v, torch.randn(ROWS, pad_m, generator=g) * 3], -1)
    for wa, wb in ((a, b), (torch.ones(n), torch.ones(ROWS, m))):
        ap = torch.cat([wa.expand(ROWS, n), torch.zeros(ROWS, pad_n)], -1)
        bp = torch.cat([wb.expand(ROWS, m), torch.zeros(ROWS, pad_m)], -1)
        for p in (2, 1.5, 1):
            ref = quantile_merge(u, v, p, wa, wb)
            bound = bound_from(quantile_merge(u, v, p, wa, wb, dtype=torch.float32), ref)
            got = shw.line_ot_rows(up.to(DEV), vp.to(DEV), p, ap.to(DEV), bp.to(DEV)).cpu()
            assert rel_dev(got, ref) <= bound, (p, rel_dev(got, ref), bound)
            gu, gv = rows_grads(shw, up, vp, p, ap, bp)
            assert torch.equal(gu[:, n:], torch.zeros(ROWS, pad_n)) and torch.equal(gv[:, m:], torch.zeros(ROWS, pad_m))
            ru, rv = ref_grads(u, v, p, wa, wb, torch.float64)
            fu, fv = ref_grads(u, v, p, wa, wb, torch.float32)
            for got_g, r, f in ((gu[:, :n], ru, fu), (gv[:, :m], rv, fv)):
                if p == 1:
                    grad_close(got_g.numpy(), r.numpy(), max_outside=0, label="line_ot_rows padding p=1")
                else:
                    assert grad_dev(got_g, r) <= max(4.0 * grad_dev(f, r), FLOOR)


def test_duplicated_keys_and_all_equal_rows(shw):
    n, m = 130, 96
    g = torch.Generator().manual_seed(61)
    u = torch.randint(0, 7, (ROWS, n), generator=g).float() * 0.25          # many exact duplicates
    v = torch.randint(0, 7, (ROWS, m), generator=g).float() * 0.25 + 0.5
    a, b = float_weights(n, m, 9, False)
    check_values(shw, u, v, None, None, "duplicates uniform")
    check_values(shw, u, v, a, b, "duplicates weighted")
    ue, ve = torch.full((ROWS, n), 0.75), torch.full((ROWS, m), -0.5)       # all equal: W_p^p = 1.25^p
    for wa, wb in ((None, None), (a, b)):
        for p in POWERS:
            got = shw.line_ot_rows(ue.to(DEV), ve.to(DEV), p, dev(wa), dev(wb)).cpu().double()
            assert rel_dev(got, np.full(ROWS, 1.25 ** p)) <= FLOOR
    gu, gv = rows_grads(shw, ue, ve, 2, None, None)                         # every atom: 2 * 1.25 * its mass
    assert torch.allclose(gu, torch.full((ROWS, n), 2.5 / n), rtol=1e-6, atol=0)
    assert torch.allclose(gv, torch.full((ROWS, m), -2.5 / m), rtol=1e-6, atol=0)


@pytest.mark.parametrize("n", [1, 64, 130, 1000, 4096])
def test_identical_clouds_give_exactly_zero(shw, n):
    u, _ = rows(n, n, seed=71)
    g = torch.Generator().manual_seed(72)
    shuffled = u[:, torch.randperm(n, generator=g)]
    for p in POWERS:
        got = shw.line_ot_rows(u.to(DEV), shuffled.to(DEV), p)
        assert torch.equal(got, torch.zeros(ROWS, device=DEV)), (n, p, got)


# ------------------------------------------------------------------------------------------------ fused projection
def fused_inputs(B, n, m, D, L, per_pair_dirs, seed):
    g = torch.Generator().manual_seed(seed)
    xs = torch.randn(B, n, D, generator=g)
    xt = torch.randn(B, m, D, generator=g) + 0.5
    th = torch.randn((B, L, D) if per_pair_dirs else (L, D), generator=g)
    th = th / th.norm(dim=-1, keepdim=True)
    return xs, xt, th


def fused_reference(xs, xt, th, p, a, b, dtype):
    """keys in `dtype` (a matmul: the float32 statement carries the key rounding of float32), then the quantile merge"""
    t = th.to(dtype)
    t = t if t.dim() == 3 else t.unsqueeze(0).expand(xs.shape[0], -1, -1)
    ks = torch.einsum("bnd,bld->bln", xs.to(dtype), t)
    kt = torch.einsum("bmd,bld->blm", xt.to(dtype), t)
    wa = None if a is None else (a if a.dim() == 1 else a.unsqueeze(1))
    wb = None if b is None else (b if b.dim() == 1 else b.unsqueeze(1))
    return quantile_merge(ks, kt, p, wa, wb, dtype=dtype)


@pytest.mark.parametrize("D", [1, 3, 6, 64])
@pytest.mark.parametrize("per_pair_dirs", [False, True])
@pytest.mark.parametrize("weights", ["none", "shared", "per_pair"])
def test_fused_values_and_gradients(shw, D, per_pair_dirs, weights):
    B, n, m, L = 2, 257, 96, 4
    xs, xt, th = fused_inputs(B, n, m, D, L, per_pair_dirs, seed=80 + D)
    g = torch.Generator().manual_seed(81)
    a = b = None
    if weights != "none":
        lead = (B,) if weights == "per_pair" else ()
        a, b = torch.rand(lead + (n,), generator=g) + 0.05, torch.rand(lead + (m,), generator=g) + 0.05
    wl = torch.rand(B, L, generator=g) + 0.5                    # upstream weights of the slices
    for p in (2, 3, 1.5, 1):
        leaves = [t.clone().requires_grad_() for t in (xs, xt, th)]
        ref = fused_reference(*leaves, p, a, b, torch.float64)
        (ref * wl).sum().backward()
        l32 = [t.clone().requires_grad_() for t in (xs, xt, th)]
        r32 = fused_reference(*l32, p, a, b, torch.float32)
        (r32 * wl).sum().backward()
        ld = [t.to(DEV).requires_grad_() for t in (xs, xt, th)]
        got = shw.esw_slice_costs(*ld, p, dev(a), dev(b))
        assert got.shape == (B, L)
        (got * wl.to(DEV)).sum().backward()
        bound = bound_from(r32.detach(), ref.detach())
        print(f"fused D={D} p={p}: value gpu {rel_dev(got.detach().cpu(), ref.detach()):.2e} bound {bound:.2e}")
        assert rel_dev(got.detach().cpu(), ref.detach()) <= bound, (p, bound)
        for name, gd, gr, g32 in zip(("xs", "xt", "thetas"), ld, leaves, l32):
            if p == 1:
                # (keys are computed here, so a near-tie could flip a sign: none does on these inputs -- measured 0)
                grad_close(gd.grad.cpu().numpy(), gr.grad.numpy(), max_outside=0, label=f"esw_slice_costs p=1 D={D} {name}")
                continue
            gb = max(4.0 * grad_dev(g32.grad, gr.grad), FLOOR)
            print(f"fused D={D} p={p} d{name}: gpu {grad_dev(gd.grad.cpu(), gr.grad):.2e} bound {gb:.2e}")
            assert grad_dev(gd.grad.cpu(), gr.grad) <= gb, (name, p, grad_dev(gd.grad.cpu(), gr.grad), gb)


def test_fused_equals_composed_rows(shw):
    """the fused keys are the projection's; with float32 torch keys the composed op sees keys that differ by a rounding,
    so the two agree within the value bound (not bit for bit)"""
    xs, xt, th = fused_inputs(2, 300, 200, 3, 8, False, seed=90)
    fused = shw.esw_slice_costs(xs.to(DEV), xt.to(DEV), th.to(DEV), 2)
    ks = torch.einsum("bnd,ld->bln", xs.to(DEV), th.to(DEV))
    kt = torch.einsum("bmd,ld->blm", xt.to(DEV), th.to(DEV))
    composed = shw.line_ot_rows(ks, kt, 2)
    assert rel_dev(fused.cpu(), composed.cpu()) <= 4e-6


# ------------------------------------------------------------------------------------------------ pinned neighbours
@pytest.mark.parametrize("n", [1, 64, 257, 1000, 2048, 4096])
def test_equal_uniform_rows_match_sorted_row_sums(shw, n):
    u, v = rows(n, n, seed=100 + n)
    for p in POWERS:
        want = shw.sorted_row_sums(u.to(DEV), v.to(DEV), p).cpu()
        got = n * shw.line_ot_rows(u.to(DEV), v.to(DEV), p).cpu()
        assert rel_dev(got, want) <= 1e-6, (n, p, rel_dev(got, want))


@pytest.mark.parametrize("n,D", [(257, 3), (1000, 6), (2048, 3), (64, 64)])
def test_equal_uniform_slices_match_esw_slice_sums(shw, n, D):
    xs, xt, th = fused_inputs(2, n, n, D, 4, False, seed=110 + n)
    for p in POWERS:
        want = shw.esw_slice_sums(xs.to(DEV), xt.to(DEV), th.to(DEV), p).cpu()
        got = n * shw.esw_slice_costs(xs.to(DEV), xt.to(DEV), th.to(DEV), p).cpu()
        assert rel_dev(got, want) <= 1e-6, (n, D, p, rel_dev(got, want))


def test_weighted_distance_is_the_mass_normalised_swd(shw):
    n, D, L, p = 300, 3, 16, 2
    xs, xt, _ = fused_inputs(1, n, n, D, L, False, seed=120)
    torch.manual_seed(5)
    want = shw.sliced_wasserstein_distance(xs[0].to(DEV), xt[0].to(DEV), L, p, DEV).item() / n ** (1.0 / p)
    torch.manual_seed(5)
    got = shw.weighted_sliced_wasserstein_distance(xs[0].to(DEV), xt[0].to(DEV), L, p, DEV).item()
    assert abs(got - want) <= 2e-6 * want
    # unequal sizes with weights: against the float64 restatement on the same draw
    torch.manual_seed(5)
    th = shw.rand_projections(D, L)
    a, b = float_weights(n, 200, 13, False)
    ref = fused_reference(xs, xt[:, :200], th, p, a, b, torch.float64).mean() ** (1.0 / p)
    torch.manual_seed(5)
    got = shw.weighted_sliced_wasserstein_distance(xs[0].to(DEV), xt[0, :200].to(DEV), L, p, DEV, a.to(DEV), b.to(DEV))
    assert abs(got.item() - ref.item()) <= 1e-5 * ref.item()


# ------------------------------------------------------------------------------------------------ determinism
@pytest.mark.parametrize("n,m", [(257, 96), (2048, 1536)])
def test_two_calls_give_the_same_bits(shw, n, m):
    u, v = rows(n, m, seed=130)
    a, b = float_weights(n, m, 14, True)
    xs, xt, th = fused_inputs(2, n, m, 3, 4, True, seed=131)
    for wa, wb in ((None, None), (a, b)):
        outs = []
        for _ in range(2):
            ud, vd = u.to(DEV).requires_grad_(), v.to(DEV).requires_grad_()
            c = shw.line_ot_rows(ud, vd, 1.5, dev(wa), dev(wb))
            c.sum().backward()
            # the value-only call (bare keys sorted, no indices) returns the training call's cost, bit for bit
            assert torch.equal(shw.line_ot_rows(u.to(DEV), v.to(DEV), 1.5, dev(wa), dev(wb)), c.detach())
            ld = [t.to(DEV).requires_grad_() for t in (xs, xt, th)]
            f = shw.esw_slice_costs(*ld, 2, dev(wa)[:2] if wa is not None else None, dev(wb)[:2] if wb is not None else None)
            f.sum().backward()
            outs.append([c.detach(), ud.grad, vd.grad, f.detach()] + [t.grad for t in ld])
        for x, y in zip(*outs):
            assert torch.equal(x, y)


# ------------------------------------------------------------------------------------------------ refusals
def test_refusals(shw):
    u, v = torch.zeros(2, 8, device=DEV), torch.zeros(2, 6, device=DEV)
    with pytest.raises(ValueError, match="4096"):
        shw.line_ot_rows(torch.zeros(2, 4097, device=DEV), v)
    with pytest.raises(ValueError, match="4096"):
        shw.esw_slice_costs(torch.zeros(1, 8, 3, device=DEV), torch.zeros(1, 4097, 3, device=DEV), torch.zeros(4, 3, device=DEV))
    with pytest.raises(ValueError, match="64"):
        shw.esw_slice_costs(torch.zeros(1, 8, 65, device=DEV), torch.zeros(1, 6, 65, device=DEV), torch.zeros(4, 65, device=DEV))
    with pytest.raises(TypeError, match="float32"):
        shw.line_ot_rows(u.double(), v.double())
    with pytest.raises(TypeError, match="float32"):
        shw.esw_slice_costs(torch.zeros(1, 8, 3, device=DEV, dtype=torch.float64), torch.zeros(1, 6, 3, device=DEV),
                            torch.zeros(4, 3, device=DEV))
    with pytest.raises(TypeError, match="float32"):
        shw.line_ot_rows(u, v, 2, torch.ones(8, device=DEV, dtype=torch.float64))
    with pytest.raises(ValueError, match=r"\(8,\)"):
        shw.line_ot_rows(u, v, 2, torch.ones(7, device=DEV))
    with pytest.raises(ValueError, match=r"\(6,\)"):
        shw.line_ot_rows(u, v, 2, None, torch.ones(3, 6, device=DEV))
    with pytest.raises(ValueError, match=r"\(1,8\)"):
        shw.esw_slice_costs(torch.zeros(1, 8, 3, device=DEV), torch.zeros(1, 6, 3, device=DEV), torch.zeros(4, 3, device=DEV),
                            2, torch.ones(2, 8, device=DEV))
    with pytest.raises(ValueError, match="no gradient with respect to the weights"):
        shw.line_ot_rows(u, v, 2, torch.ones(8, device=DEV, requires_grad=True))
    with pytest.raises(ValueError, match="no gradient with respect to the weights"):
        shw.esw_slice_costs(torch.zeros(1, 8, 3, device=DEV), torch.zeros(1, 6, 3, device=DEV), torch.zeros(4, 3, device=DEV),
                            2, None, torch.ones(6, device=DEV, requires_grad=True))
    with pytest.raises(ValueError, match="at least 1"):
        shw.line_ot_rows(u, v, 0.5)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        shw.line_ot_rows(u, v, 2, torch.ones(8))
    with pytest.raises(ValueError, match="leading shapes"):
        shw.line_ot_rows(u, torch.zeros(3, 6, device=DEV))
    # the sign and the sum of the weights are NOT checked on the device (line_ot.py's docstring says so): such a call
    # returns, in bounded time, a value that means nothing
    assert "NOT checked" in shw.line_ot.__doc__
    assert shw.line_ot_rows(u + 1, v, 2, torch.zeros(8, device=DEV)).shape == (2,)
