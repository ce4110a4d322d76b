"""Fixture G16 (tests/golden/g16_notebook_gsw.npz): the notebooks' generalised sliced-W family -- GSWD_circular,
max_GSWD_circular, GSWD_polynomial, max_GSWD_polynomial_3 / _5, distributional_sliced_wasserstein_distance, gsw_nn_1 and
max_gsw_nn_1 (Wasserstein_flow_problem/Flow_cube.ipynb, the cell that starts with `def rand_projections`), exec'd from
the .ipynb JSON on the CPU by oracle.make_golden.notebook_cell_namespace, as G9 and G11 are.

Needs the reference notebooks next to the repository, so it runs on a build machine only; the tests read the .npz.
Run:  python tools/make_golden_gsw.py [path/to/Flow_cube.ipynb]

Clouds: G10's (tests/golden/g10_notebook_flow.npz `source` / `target`, N = 1200 cube surfaces); they are not repeated
here.  Per case `<case>_seed`, `<case>_value`, `<case>_grad_first` (d value / d first_samples) and the parameters drawn
and reached:
  circ_p2, circ_p1       GSWD_circular (p=2, L=100, r=1) and (p=1, L=16, r=0.5): `_theta`, the unit directions drawn
  maxcirc                max_GSWD_circular, max_iter=10: `_theta0` (unit), `_theta` after the ascent
  poly3, poly5           GSWD_polynomial degree 3 / 5, L=100: `_coefficient`, the raw draw (before normalisation)
  maxpoly3, maxpoly5     max_GSWD_polynomial_3 / _5, max_iter=10: `_coefficient0` (raw draw), `_coefficient` after
  dswd                   TransformNet(3) from `dswd_weight0` / `dswd_bias0`, L=100, max_iter=10, lam=10, Adam lr 0.005
                         betas (0.999, 0.999): `_weight`, `_bias` after the call
  nn1, maxnn1            MLP(din=3, dout=4, num_filters=8, depth=2) from `mlp_param0_<k>`, Adam lr 0.005:
                         `maxnn1_param_<k>` after the ascent
The draws are recovered by re-seeding, as G11 does.  The cell's `polynomial_function` hard-codes device='cuda' as a
default; it is set to 'cpu' after the exec.

Every case with an ascent loop is run a second time with clouds, parameters and draws cast to float64 (the same
float32 draws, cast).  `<case>_f32_gap` = |value32 - value64| / |value64|, `<case>_grad_f32_gap` = max |grad32 -
grad64| / max |grad64| and `<case>_param_f32_gap` = max |param32 - param64| / max |param64| measure what the reference's
own float32 rounding, amplified through ten Adam steps, does to the result: the tests' tolerances for these cases are
multiples of them."""
from __future__ import annotations

import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle.make_golden import notebook_cell_namespace  # noqa: E402

NOTEBOOK = os.path.join(os.path.dirname(ROOT), "reference", "Wasserstein_flow_problem", "Flow_cube.ipynb")
OUT = os.path.join(ROOT, "tests", "golden", "g16_notebook_gsw.npz")
SEEDS = {"circ_p2": 16001, "circ_p1": 16002, "maxcirc": 16003, "poly3": 16004, "poly5": 16005, "maxpoly3": 16006,
         "maxpoly5": 16007, "dswd": 16008, "nn1": 16009, "maxnn1": 16010}
F_SEED, MLP_SEED = 16100, 16101
MAX_ITER, LAM, LR = 10, 10, 0.005


def _np(t):
    return t.detach().cpu().numpy()


class _Recorder:
    """stands in for the cell's `optim`: hands out real Adam optimisers and keeps the tensors they were given, which is
    how the theta / coefficient a max_* function ascended on is read back (the functions return only the value)"""

    def __init__(self):
        self.params = None

    def Adam(self, params, **kw):
        self.params = list(params)
        return torch.optim.Adam(self.params, **kw)


def _double_draws(real):
    """a stand-in for the cell's `torch` whose randn draws in float32 (the same stream) and casts to float64"""
    def randn(*size, **kw):
        leaf = kw.pop("requires_grad", False)
        return real.randn(*size, **kw).double().requires_grad_(leaf)

    class TorchDoubleDraws:
        def __getattr__(self, name):                 # everything but randn is torch's own
            return getattr(real, name)

    proxy = TorchDoubleDraws()
    proxy.randn = randn
    return proxy


def _gaps(out, name, v32, g32, v64, g64, p32=None, p64=None):
    out[f"{name}_f32_gap"] = np.float64(abs(v32.item() - v64.item()) / abs(v64.item()))
    out[f"{name}_grad_f32_gap"] = np.float64((g32.double() - g64).abs().max().item() / g64.abs().max().item())
    if p32 is not None:
        num = max((a.double() - b).abs().max().item() for a, b in zip(p32, p64))
        out[f"{name}_param_f32_gap"] = np.float64(num / max(b.abs().max().item() for b in p64))


def main(notebook=NOTEBOOK):
    ns = notebook_cell_namespace(notebook, "def rand_projections")
    ns["polynomial_function"].__defaults__ = ("cpu",)
    recorder = _Recorder()
    ns["optim"] = recorder
    g10 = np.load(os.path.join(ROOT, "tests", "golden", "g10_notebook_flow.npz"))
    source, target = torch.from_numpy(g10["source"]), torch.from_numpy(g10["target"])
    out = {}

    def run(fn, *args, double=False, **kw):
        """fn(first, target, ...) with a fresh differentiable copy of the source: (value, gradient)"""
        first = (source.double() if double else source).clone().requires_grad_(True)
        ns["torch"] = _double_draws(torch) if double else torch
        try:
            val = ns[fn](first, target.double() if double else target, *args, **kw)
        finally:
            ns["torch"] = torch
        val.backward()
        return val.detach(), first.grad

    def unit_rows(seed, L):
        torch.manual_seed(seed)
        t = torch.randn((L, 3))
        return t / torch.sqrt(torch.sum(t ** 2, dim=1, keepdim=True))

    # ---- circular
    for name, p, L, r in (("circ_p2", 2, 100, 1), ("circ_p1", 1, 16, 0.5)):
        torch.manual_seed(SEEDS[name])
        val, grad = run("GSWD_circular", p=p, num_projection=L, r=r, device="cpu")
        out.update({f"{name}_p": np.float64(p), f"{name}_L": np.int64(L), f"{name}_r": np.float64(r),
                    f"{name}_value": _np(val), f"{name}_grad_first": _np(grad),
                    f"{name}_theta": _np(unit_rows(SEEDS[name], L))})
    torch.manual_seed(SEEDS["maxcirc"])
    val, grad = run("max_GSWD_circular", p=2, r=1, device="cpu", max_iter=MAX_ITER)
    theta = recorder.params[0].detach().clone()
    torch.manual_seed(SEEDS["maxcirc"])
    val64, grad64 = run("max_GSWD_circular", p=2, r=1, device="cpu", max_iter=MAX_ITER, double=True)
    _gaps(out, "maxcirc", val, grad, val64, grad64, [theta], [recorder.params[0].detach()])
    out.update({"maxcirc_value": _np(val), "maxcirc_grad_first": _np(grad), "maxcirc_theta": _np(theta),
                "maxcirc_theta0": _np(unit_rows(SEEDS["maxcirc"], 1))})

    # ---- polynomial
    def raw(seed, count, L):
        torch.manual_seed(seed)
        return torch.randn((count, L), device="cpu")

    for name, degree, count in (("poly3", 3, 10), ("poly5", 5, 21)):
        assert ns["poly_degree"](degree, 3).shape[0] == count
        torch.manual_seed(SEEDS[name])
        val, grad = run("GSWD_polynomial", p=2, num_projection=100, degree=degree, device="cpu")
        out.update({f"{name}_value": _np(val), f"{name}_grad_first": _np(grad), f"{name}_features": np.int64(count),
                    f"{name}_coefficient": _np(raw(SEEDS[name], count, 100))})
    for name, fn, count in (("maxpoly3", "max_GSWD_polynomial_3", 10), ("maxpoly5", "max_GSWD_polynomial_5", 21)):
        torch.manual_seed(SEEDS[name])
        val, grad = run(fn, p=2, device="cpu", max_iter=MAX_ITER)
        coef = recorder.params[0].detach().clone()
        torch.manual_seed(SEEDS[name])
        val64, grad64 = run(fn, p=2, device="cpu", max_iter=MAX_ITER, double=True)
        _gaps(out, name, val, grad, val64, grad64, [coef], [recorder.params[0].detach()])
        out.update({f"{name}_value": _np(val), f"{name}_grad_first": _np(grad), f"{name}_coefficient": _np(coef),
                    f"{name}_coefficient0": _np(raw(SEEDS[name], count, 1))})

    # ---- DSWD
    torch.manual_seed(F_SEED)
    f0 = ns["TransformNet"](3)
    W0, b0 = f0.net[0].weight.detach().clone(), f0.net[0].bias.detach().clone()

    def fresh_f(double):
        f = ns["TransformNet"](3)
        with torch.no_grad():
            f.net[0].weight.copy_(W0)
            f.net[0].bias.copy_(b0)
        if double:
            f = f.double()
        return f, torch.optim.Adam(f.parameters(), lr=LR, betas=(0.999, 0.999))

    f, f_op = fresh_f(False)
    torch.manual_seed(SEEDS["dswd"])
    val, grad = run("distributional_sliced_wasserstein_distance", 100, f, f_op, p=2, max_iter=MAX_ITER, lam=LAM,
                    device="cpu")
    f64, f64_op = fresh_f(True)
    torch.manual_seed(SEEDS["dswd"])
    val64, grad64 = run("distributional_sliced_wasserstein_distance", 100, f64, f64_op, p=2, max_iter=MAX_ITER, lam=LAM,
                        device="cpu", double=True)
    _gaps(out, "dswd", val, grad, val64, grad64, [q.detach() for q in f.parameters()],
          [q.detach() for q in f64.parameters()])
    out.update({"dswd_weight0": _np(W0), "dswd_bias0": _np(b0), "dswd_value": _np(val), "dswd_grad_first": _np(grad),
                "dswd_weight": _np(f.net[0].weight), "dswd_bias": _np(f.net[0].bias), "dswd_L": np.int64(100),
                "dswd_lam": np.float64(LAM)})

    # ---- network-defined
    torch.manual_seed(MLP_SEED)
    params0 = [q.detach().clone() for q in ns["MLP"](din=3, dout=4, num_filters=8, depth=2).parameters()]

    def fresh_net(double):
        net = ns["MLP"](din=3, dout=4, num_filters=8, depth=2)
        with torch.no_grad():
            for mine, given in zip(net.parameters(), params0):
                mine.copy_(given)
        if double:
            net = net.double()
        return net, torch.optim.Adam(net.parameters(), lr=LR)

    for k, q in enumerate(params0):
        out[f"mlp_param0_{k}"] = _np(q)
    net, net_op = fresh_net(False)
    val, grad = run("gsw_nn_1", net, net_op, max_iter=MAX_ITER, p=2)
    out.update({"nn1_value": _np(val), "nn1_grad_first": _np(grad)})
    net, net_op = fresh_net(False)
    val, grad = run("max_gsw_nn_1", net, net_op, max_iter=MAX_ITER, p=2)
    net64, net64_op = fresh_net(True)
    val64, grad64 = run("max_gsw_nn_1", net64, net64_op, max_iter=MAX_ITER, p=2, double=True)
    _gaps(out, "maxnn1", val, grad, val64, grad64, [q.detach() for q in net.parameters()],
          [q.detach() for q in net64.parameters()])
    out.update({"maxnn1_value": _np(val), "maxnn1_grad_first": _np(grad)})
    for k, q in enumerate(net.parameters()):
        out[f"maxnn1_param_{k}"] = _np(q)

    for name, seed in SEEDS.items():
        out[f"{name}_seed"] = np.int64(seed)
    out["max_iter"] = np.int64(MAX_ITER)
    np.savez_compressed(OUT, **out)
    print(OUT, os.path.getsize(OUT))
    for k in sorted(out):
        if k.endswith("_gap") or k.endswith("_value"):
            print(f"  {k}: {float(out[k]):.6g}")


if __name__ == "__main__":
    torch.set_num_threads(8)
    main(*sys.argv[1:])
