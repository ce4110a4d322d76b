"""tools/make_golden_flows.py -- fixture G18 (tests/golden/g18_flows.npz): the reference's sphere maps, captured from the
REAL reference (it needs a checkout of it; the tests need only the fixture).

The reference's `Norm_Flow_structure` (losses/s2_wasserstein.py:134-163) cannot be imported here: the package __init__ of
its vendored normflows_ishikawa pulls in a module that is not installed.  The four files the structure needs --
flows/base.py, flows/planar.py, flows/residual.py, nets/lipschitz.py -- need only torch and numpy, so they are loaded by
file path behind empty stand-in packages, and the structure is restated below in a few lines from the classes they define.

Stored, for the cases `res` (Residual x 3, width 8, 7 linear layers: the trainers' default), `res53` (Residual x 3, width
5, 3 linear layers: Norm_Flow_structure_optuna) and `planar` (Planar x 3): the state dict as constructed (names, shapes
and dtypes in order, the values as one float64 vector), the ordered parameter names, and for the inputs `x3` (2, 70, 3)
and `x2` (70, 3) with the cotangents `c3`, `c2`: the output in train and in eval mode and the gradients of sum(out * c)
w.r.t. the input and every parameter that receives one (their names in order, the values as one vector).
tests/helpers/flow_cases.py reads it back.

    python tools/make_golden_flows.py --reference <reference checkout>/Point_Cloud_Resistration/losses
"""
import argparse
import copy
import importlib.util
import os
import sys
import types

import numpy as np
import torch
from torch import nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden", "g18_flows.npz")
CASES = {"res": ("Residual", 8, 7), "res53": ("Residual", 5, 3), "planar": ("Planar", 0, 0)}


def load_reference(losses_dir):
    """flows.base, flows.planar, flows.residual, nets.lipschitz of the vendored package, by path"""
    pkg_dir = os.path.join(losses_dir, "normflows_ishikawa")
    for name, sub in (("nf_ref", ""), ("nf_ref.flows", "flows"), ("nf_ref.nets", "nets")):
        pkg = types.ModuleType(name)
        pkg.__path__ = [os.path.join(pkg_dir, sub)]
        sys.modules[name] = pkg
    mods = {}
    for name, rel in (("nf_ref.flows.base", "flows/base.py"), ("nf_ref.flows.planar", "flows/planar.py"),
                      ("nf_ref.flows.residual", "flows/residual.py"), ("nf_ref.nets.lipschitz", "nets/lipschitz.py")):
        spec = importlib.util.spec_from_file_location(name, os.path.join(pkg_dir, rel))
        mod = importlib.util.module_from_spec(spec)
        sys.modules[name] = mod
        spec.loader.exec_module(mod)
        mods[name.rsplit(".", 1)[1]] = mod
    return mods


class Structure(nn.Module):
    """s2_wasserstein.py:134-201 restated: a ModuleList `net` of flows, forward keeps the points and drops the log-det"""

    def __init__(self, ref, flow_name, hidden, layers, n_flow_layer=3, dim=3):
        super().__init__()
        if flow_name == "Planar":
            flows = [ref["planar"].Planar((dim,)) for _ in range(n_flow_layer)]
        else:
            flows = [ref["residual"].Residual(
                ref["lipschitz"].LipschitzMLP([dim] + [hidden] * (layers - 1) + [dim], init_zeros=True, lipschitz_const=0.95),
                reverse=False, reduce_memory=True) for _ in range(n_flow_layer)]
        self.net = nn.ModuleList(flows)

    def forward(self, x):
        for flow in self.net:
            x, _ = flow(x)
        return x


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="the reference's Point_Cloud_Resistration/losses directory")
    args = ap.parse_args()
    ref = load_reference(args.reference)
    g = torch.Generator().manual_seed(18)
    data = {"x3": torch.randn(2, 70, 3, generator=g), "x2": torch.randn(70, 3, generator=g),
            "c3": torch.randn(2, 70, 3, generator=g), "c2": torch.randn(70, 3, generator=g)}
    out = {k: v.numpy() for k, v in data.items()}
    scales = []
    for case, (flow_name, hidden, layers) in CASES.items():
        torch.manual_seed(0)
        np.random.seed(0)
        phi = Structure(ref, flow_name, hidden, layers)
        state = copy.deepcopy(phi.state_dict())               # as constructed: the forward below rewrites some buffers
        out[f"{case}.state_names"] = np.array(list(state))
        out[f"{case}.param_names"] = np.array([n for n, _ in phi.named_parameters()])
        # one vector per case, not one array per tensor (hundreds of tiny archive members): float64 holds every entry exactly
        out[f"{case}.state_shapes"] = np.array(["x".join(map(str, t.shape)) for t in state.values()])
        out[f"{case}.state_dtypes"] = np.array([str(t.dtype).replace("torch.", "") for t in state.values()])
        out[f"{case}.state_values"] = np.concatenate([t.double().numpy().reshape(-1) for t in state.values()])
        scales += [float(t) for name, t in state.items() if name.endswith(".scale")]
        for xk, ck in (("x3", "c3"), ("x2", "c2")):
            phi.eval()
            with torch.no_grad():
                out[f"{case}.{xk}.eval"] = phi(data[xk].clone()).numpy()      # a copy: the reference marks its input
            phi.train()
            phi.zero_grad()
            x = data[xk].detach().clone().requires_grad_()
            y = phi(x)
            (y * data[ck]).sum().backward()
            out[f"{case}.{xk}.train"] = y.detach().numpy()
            out[f"{case}.{xk}.grad_x"] = x.grad.numpy()
            with_grad = [(name, p.grad) for name, p in phi.named_parameters() if p.grad is not None]
            out[f"{case}.{xk}.grad_names"] = np.array([name for name, _ in with_grad])
            out[f"{case}.{xk}.grad_values"] = np.concatenate([g.numpy().reshape(-1) for _, g in with_grad])
            print(case, xk, "train == eval:", np.array_equal(out[f"{case}.{xk}.train"], out[f"{case}.{xk}.eval"]),
                  "parameters with a gradient:", len(with_grad), "of", len(out[f"{case}.param_names"]))
    # both branches of max(1, sigma / 0.95) must be in the fixture
    assert any(s > 0.95 for s in scales) and any(s < 0.95 for s in scales), scales
    print("scales of the first flow:", [round(s, 3) for s in scales[:7]])
    np.savez_compressed(OUT, **out)
    size = os.path.getsize(OUT)
    assert size < 100 * 1024, size
    print("wrote", OUT, size, "bytes")


if __name__ == "__main__":
    main()
