"""Fixture G11 (tests/golden/g11_notebook_aswd.npz): the notebooks' ASWD baseline, `augmented_sliced_wassersten_distance`
with phi = Mapping(3) (Wasserstein_flow_problem/Flow_cube.ipynb, the cell that starts with `def rand_projections`),
exec'd from the .ipynb JSON on the CPU by oracle.make_golden.notebook_cell_namespace, as G9 is.

Needs the reference notebooks next to the repository, so it runs on a build machine only; the GPU tests read the .npz.
Run:  python tools/make_golden_aswd.py [path/to/Flow_cube.ipynb]

Contents: G10's clouds (N = 1200, the notebooks' cube surfaces); the initial weight and bias of a seeded Mapping(3);
per case (the final evaluation alone; the notebook's call, max_iter = 10 with lam = 0.05 / target.abs().mean(); a
p = 1 case with small L) the seed, the value, d value / d first_samples, phi's parameters after the call and the
directions every evaluation drew; and five outer steps of the notebook's ASWD flow loop (Adam, lr 0.01, on the
evolving cloud): the loss per step, the final cloud and phi's final parameters."""
from __future__ import annotations

import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle.make_golden import notebook_cell_namespace  # noqa: E402

NOTEBOOK = "/root/reference/Wasserstein_flow_problem/Flow_cube.ipynb"
OUT = os.path.join(ROOT, "tests", "golden", "g11_notebook_aswd.npz")
PHI_SEED = 20250112
CASES = (                          # name, p, L, max_iter, lam (None: the notebook's 0.05 / target.abs().mean()), seed
    ("it0_p2", 2, 100, 0, None, 11001),
    ("it10_p2", 2, 100, 10, None, 11002),
    ("it3_p1", 1, 16, 3, None, 11003),
)
FLOW_SEED, FLOW_STEPS, FLOW_LR = 11100, 5, 0.01


def _np(t):
    return t.detach().cpu().numpy()


def main(notebook=NOTEBOOK):
    ns = notebook_cell_namespace(notebook, "def rand_projections")
    aswd, Mapping, rand_projections = ns["augmented_sliced_wassersten_distance"], ns["Mapping"], ns["rand_projections"]
    g10 = np.load(os.path.join(ROOT, "tests", "golden", "g10_notebook_flow.npz"))
    source, target = torch.from_numpy(g10["source"]), torch.from_numpy(g10["target"])
    lam = 0.05 / target.abs().mean()                   # Flow_cube.ipynb, the ASWD branch of the flow loop
    torch.manual_seed(PHI_SEED)
    phi0 = Mapping(3)
    W0, b0 = phi0.net[0].weight.detach().clone(), phi0.net[0].bias.detach().clone()
    out = {"source": _np(source), "target": _np(target), "phi_weight0": _np(W0), "phi_bias0": _np(b0),
           "lam": np.float32(lam.item()), "flow_lr": np.float64(FLOW_LR)}

    def fresh_phi():
        phi = Mapping(3)
        with torch.no_grad():
            phi.net[0].weight.copy_(W0)
            phi.net[0].bias.copy_(b0)
        return phi, torch.optim.Adam(phi.parameters(), lr=0.005, betas=(0.999, 0.999))

    for name, p, L, max_iter, case_lam, seed in CASES:
        phi, phi_op = fresh_phi()
        first = source.clone().requires_grad_(True)
        torch.manual_seed(seed)
        val = aswd(first, target, L, phi, phi_op, p=p, max_iter=max_iter, lam=lam if case_lam is None else case_lam,
                   device="cpu")
        W, b = phi.net[0].weight.detach().clone(), phi.net[0].bias.detach().clone()
        val.backward()
        torch.manual_seed(seed)                        # nothing else draws from the generator between evaluations
        thetas = torch.stack([rand_projections(6, L) for _ in range(max_iter + 1)])
        out.update({f"{name}_p": np.float64(p), f"{name}_L": np.int64(L), f"{name}_max_iter": np.int64(max_iter),
                    f"{name}_seed": np.int64(seed), f"{name}_value": _np(val), f"{name}_grad_first": _np(first.grad),
                    f"{name}_phi_weight": _np(W), f"{name}_phi_bias": _np(b), f"{name}_thetas": _np(thetas)})

    phi, phi_op = fresh_phi()
    evolving = source.clone().requires_grad_(True)
    opt = torch.optim.Adam([evolving], lr=FLOW_LR, betas=(0.9, 0.999))
    torch.manual_seed(FLOW_SEED)
    trace = []
    for _ in range(FLOW_STEPS):
        opt.zero_grad()
        loss = aswd(evolving, target, 100, phi, phi_op, p=2, max_iter=10, lam=lam, device="cpu", net_type="fc")
        loss.backward(retain_graph=True)
        opt.step()
        trace.append(float(loss))
    out.update({"flow_seed": np.int64(FLOW_SEED), "flow_trace": np.asarray(trace, dtype=np.float64),
                "flow_evolved": _np(evolving), "flow_phi_weight": _np(phi.net[0].weight),
                "flow_phi_bias": _np(phi.net[0].bias)})
    np.savez_compressed(OUT, **out)
    print(OUT, os.path.getsize(OUT))


if __name__ == "__main__":
    torch.set_num_threads(8)
    main(*sys.argv[1:])
