"""CPU checks behind tests/test_sinkhorn_plan_gpu.py: the oracle for gradients through the Sinkhorn plan is pinned to the
real classes (fixture G17, tools/make_golden_sinkhorn_plan.py), the closed-form seeds the kernels start the adjoint
recursion from equal float64 autograd, the float32 and float64 mirror runs execute the same sweeps on every GPU case
(so their gap is rounding, not a different stopping point), and the header declares the new entries."""
import os
import re

import pytest
import torch

from helpers import sinkhorn_chamfer_cases as cases
from helpers import sinkhorn_plan_cases as plan
from oracle import sinkhorn_mirror

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def within(what, gap, g, k=cases.K):
    r = cases.ratio(gap, g)
    print(f"GAP {what}: {gap:.3e} mirror {g:.3e} ratio {r:.2f}")
    assert gap < cases.bound(g, 1.0, k), f"{what}: gap {gap:.3e} = {r:.1f} x the fixture's own gap {g:.3e} (bound {k})"


@pytest.mark.parametrize("tag", list(plan.G17))
def test_mirror_autograd_reproduces_g17_plan_gradients(golden, tag):
    """cost, gx, gy of L = sum w cost + <WP, P> + <WC, C>: the mirror in float64 and in float32 against the real class in
    float64, within 16 x the real class's own float32-vs-float64 gap"""
    f = golden("g17_sinkhorn_plan.npz")
    kw = plan.G17[tag]
    x, y, WP, WC = (torch.from_numpy(f[k]) for k in ("x", "y", "WP", "WC"))
    for dtype in (torch.float64, torch.float32):
        got = plan.plan_mirror(x, y, kw["eps"], kw["max_iter"], f["w"], WP, WC, dtype, norm_p=kw["norm_p"],
                               cost_pow=kw["cost_pow"])
        within(f"G17 {tag} {dtype} cost", cases.relmax(got["cost"], f[f"cost_{tag}_f64"]), float(f[f"gap_cost_{tag}"]))
        for q in ("gx", "gy"):
            within(f"G17 {tag} {dtype} {q}", cases.of_largest(got[q], f[f"{q}_{tag}_f64"]), float(f[f"gap_{q}_{tag}"]))


def test_mirror_autograd_reproduces_g17_map_gradients(golden):
    """gx, gy of L = <G, P @ y / P.sum(-1)> (L2, eps 0.05, 60 iterations)"""
    f = golden("g17_sinkhorn_plan.npz")
    x, y, G = (torch.from_numpy(f[k]) for k in ("x", "y", "G"))
    for dtype in (torch.float64, torch.float32):
        xd, yd = x.to(dtype).requires_grad_(True), y.to(dtype).requires_grad_(True)
        _, P, _, _ = sinkhorn_mirror.sinkhorn_costs(xd, yd, 0.05, 60)
        (G.to(dtype) * (P @ yd / P.sum(-1, keepdim=True))).sum().backward()
        for q, t in (("gx", xd), ("gy", yd)):
            within(f"G17 map {dtype} {q}", cases.of_largest(t.grad.numpy(), f[f"{q}_map_f64"]), float(f[f"gap_{q}_map"]))


def test_g17_is_small_and_holds_arrays_only(golden):
    path = os.path.join(ROOT, "tests", "golden", "g17_sinkhorn_plan.npz")
    assert os.path.getsize(path) < 100 * 1024
    f = golden("g17_sinkhorn_plan.npz")
    assert f["WP"].shape == f["WC"].shape == (2, 48, 40) and f["G"].shape == (2, 48, 3)
    assert all(f[k].dtype.kind == "f" for k in f.files)


@pytest.mark.parametrize("norm_p,cost_pow", [(2, 1), (1, 1), (2, 2)])
def test_closed_form_seeds_equal_float64_autograd(norm_p, cost_pow):
    """With the final duals u, v as leaves, autograd of L = sum g cost + <GP, P> + <GC, C> gives the seeds the kernels
    compute: ubar, vbar from Ghat = g C + GP, and gx, gy from K = P (g (1 - C/eps) - GP/eps) + GC.  Then the same with the
    map's implicit cotangent GP_ij = G_i . (y_j - T_i) / r_i, GC = 0, the direct term on gy, and a zero ubar."""
    eps, n, m = 0.05, 23, 17
    gen = torch.Generator().manual_seed(160)
    x = cases.unit_cloud(gen, 2, n).double()
    y = (cases.unit_cloud(gen, 2, m) * 0.9 + 0.05).double()
    u, v = sinkhorn_mirror.sinkhorn_costs(x, y, eps, 20, norm_p=norm_p, cost_pow=cost_pow, history=True)[5]
    g = torch.tensor([1.0, -0.7], dtype=torch.float64)
    GP = torch.randn(2, n, m, generator=gen, dtype=torch.float64)
    GC = torch.randn(2, n, m, generator=gen, dtype=torch.float64)
    G = torch.randn(2, n, 3, generator=gen, dtype=torch.float64)

    def leaves():
        return [t.detach().clone().requires_grad_(True) for t in (x, y, u, v)]

    def plan_of(xd, yd, ud, vd):
        C = torch.sum(torch.abs(xd.unsqueeze(-2) - yd.unsqueeze(-3)) ** norm_p, -1) ** cost_pow
        return torch.exp((-C + ud.unsqueeze(-1) + vd.unsqueeze(-2)) / eps), C

    def seeds(P, C, GPm, GCm, gb):
        """(ubar, vbar, gx, gy) of the formulas; dC/dx by autograd of C alone (that part is pair_cost_grad's)"""
        Ghat = gb[:, None, None] * C + GPm
        K = P * (gb[:, None, None] * (1 - C / eps) - GPm / eps) + GCm
        xd, yd = x.detach().clone().requires_grad_(True), y.detach().clone().requires_grad_(True)
        Cd = torch.sum(torch.abs(xd.unsqueeze(-2) - yd.unsqueeze(-3)) ** norm_p, -1) ** cost_pow
        (K.detach() * Cd).sum().backward()
        return (P * Ghat).sum(-1) / eps, (P * Ghat).sum(-2) / eps, xd.grad, yd.grad

    def close(a, b, what):
        scale = max(float(b.abs().max()), 1e-300)
        assert float((a - b).abs().max()) < 1e-12 * scale, (what, float((a - b).abs().max()), scale)

    xd, yd, ud, vd = leaves()
    P, C = plan_of(xd, yd, ud, vd)
    ((g * (P * C).sum((-2, -1))).sum() + (GP * P).sum() + (GC * C).sum()).backward()
    ubar, vbar, gx, gy = seeds(P.detach(), C.detach(), GP, GC, g)
    for a, b, what in ((ubar, ud.grad, "ubar"), (vbar, vd.grad, "vbar"), (gx, xd.grad, "gx"), (gy, yd.grad, "gy")):
        close(a, b, "dense " + what)

    xd, yd, ud, vd = leaves()
    P, C = plan_of(xd, yd, ud, vd)
    r = P.sum(-1, keepdim=True)
    T = P @ yd / r
    (G * T).sum().backward()
    Pd, Td, rd = P.detach(), T.detach(), r.detach()
    GPi = ((G / rd).unsqueeze(-2) * (y.unsqueeze(-3) - Td.unsqueeze(-2))).sum(-1)
    ubar, vbar, gx, gy = seeds(Pd, C.detach(), GPi, torch.zeros_like(GPi), torch.zeros(2, dtype=torch.float64))
    gy = gy + (Pd.unsqueeze(-1) * (G / rd).unsqueeze(-2)).sum(-3)
    assert float(ubar.abs().max()) < 1e-12 * float(vbar.abs().max())              # sum_j P_ij GP_ij = 0
    assert float(ud.grad.abs().max()) < 1e-12 * float(vd.grad.abs().max())
    for a, b, what in ((vbar, vd.grad, "vbar"), (gx, xd.grad, "gx"), (gy, yd.grad, "gy")):
        close(a, b, "map " + what)


def test_float32_and_float64_mirror_runs_execute_the_same_sweeps():
    for c in plan.PLAN_CASES:
        ref, g = plan.plan_case(*c)[4:]
        assert g["its32"] == ref["its"], c           # ((1, 1) stops after 2 sweeps, in both)
        ref, g = plan.map_case(*c)[2:]
        assert g["its32"] == ref["its"], c
    ref, g = plan.stop_plan_case()[6:]
    assert g["its32"] == ref["its"] == cases.STOP_T
    ref, g = plan.no_sweep_plan_case()[4:]
    assert g["its32"] == ref["its"] == 0


def test_header_declares_the_plan_and_map_entries_and_abi_3():
    text = open(os.path.join(ROOT, "include", "shw.h")).read()
    assert re.search(r"#define\s+SHW_ABI_VERSION\s+3\b", text)
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in ("shw_sinkhorn_backward_plan", "shw_sinkhorn_map_forward", "shw_sinkhorn_map_backward"):
        assert re.search(r"SHW_API\s+int\s+%s\s*\(" % name, code), name
    import shw_amd
    for name in ("shw_sinkhorn_backward_plan", "shw_sinkhorn_map_forward", "shw_sinkhorn_map_backward"):
        assert name in shw_amd._lib.EXPORTED_SYMBOLS
    assert "sinkhorn_barycentric_map" in shw_amd.__all__


def test_plan_grad_without_a_plan_is_refused_before_any_device_work():
    import shw_amd
    x = torch.zeros(1, 4, 3)
    with pytest.raises(ValueError, match="plan_grad"):
        shw_amd.log_Sinkhorn_Distance_Loss(0.05, 5, return_plan=False, plan_grad=True)
    with pytest.raises(ValueError, match="plan_grad"):
        shw_amd.log_N_Sinkhorn_Distance_Loss(0.05, 5, return_plan=False, plan_grad=True)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        shw_amd.sinkhorn_barycentric_map(x, x, 0.05, 5)
