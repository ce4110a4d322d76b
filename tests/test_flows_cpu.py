"""CPU checks of the sphere map phi (flows.py): the composed path and the modules against fixture G18, which holds what
the reference's own Norm_Flow_structure computes (tools/make_golden_flows.py), the state-dict contract, the Planar flow's
rank-dependent sum, construction, and the packing of the effective parameters the kernels read.

Every test uses shw.Norm_Flow_structure, shw.residual_flow_composed or the shw_flow_residual_* entries: without the
feature each fails on the missing attribute.

Float32 against the reference's float32, bound 1e-5 on max |error| / max |reference entry| per tensor.  Measured here:
values 0 (Residual, both shapes, and Planar), d/dx 1.1e-7, parameter gradients at most 3.7e-6 (a beta).
"""
import re

import numpy as np
import pytest
import torch

from helpers.flow_cases import (COEFF, g18_grads, g18_module, g18_param_names, g18_state, g18_tensor, max_dev)

BOUND = 1e-5
CASES = ["res", "res53", "planar"]


@pytest.fixture(scope="module")
def shw():
    import shw_amd
    return shw_amd


@pytest.mark.parametrize("xk,ck", [("x3", "c3"), ("x2", "c2")])
@pytest.mark.parametrize("case", CASES)
def test_fixture_parity_of_the_composed_path(shw, case, xk, ck):
    """values in train and in eval mode and every gradient against the reference's, (2, 70, 3) and (70, 3)"""
    phi = g18_module(shw, case)
    x0, cot = g18_tensor(xk), g18_tensor(ck)
    assert np.array_equal(g18_tensor(f"{case}.{xk}.train"), g18_tensor(f"{case}.{xk}.eval"))
    outs = {}
    for mode in ("train", "eval"):
        phi.train(mode == "train")
        phi.zero_grad()
        x = x0.clone().requires_grad_()
        y = phi(x)
        assert y.shape == x0.shape and y.dtype == torch.float32
        (y * cot).sum().backward()
        outs[mode] = y.detach()
        worst = max_dev(y.detach(), g18_tensor(f"{case}.{xk}.{mode}"))
        print(f"{case} {xk} {mode}: value {worst:.2e}")
        assert worst <= BOUND, (case, xk, mode, worst)
        worst = max_dev(x.grad, g18_tensor(f"{case}.{xk}.grad_x"))
        print(f"{case} {xk} {mode}: d/dx {worst:.2e}")
        assert worst <= BOUND, (case, xk, mode, worst)
        ref, worst_param = g18_grads(case, xk), 0.0
        for name, p in phi.named_parameters():
            if name not in ref:
                assert p.grad is None, name                    # geom_p, lamb: in no computation
                continue
            worst = max_dev(p.grad, ref[name])
            worst_param = max(worst_param, worst)
            assert worst <= BOUND, (case, xk, mode, name, worst)
        print(f"{case} {xk} {mode}: parameters {worst_param:.2e}")
        assert sorted(ref) == sorted(n for n, p in phi.named_parameters() if p.grad is not None)
    assert torch.equal(outs["train"], outs["eval"])


@pytest.mark.parametrize("case", CASES)
def test_state_dict_contract(shw, case):
    ref = g18_state(case)
    phi = g18_module(shw, case)                               # load_state_dict(strict=True) inside
    own = phi.state_dict()
    assert list(own) == list(ref)
    for name in ref:
        assert own[name].shape == ref[name].shape and own[name].dtype == ref[name].dtype, name
        assert torch.equal(own[name], ref[name]), name
    assert [n for n, _ in phi.named_parameters()] == g18_param_names(case)
    if case != "planar":
        assert "net.0.iresblock.geom_p" in ref and "net.0.iresblock.lamb" in ref
        assert ref["net.0.iresblock.nnet.net.1.weight"].shape == ((8, 3) if case == "res" else (5, 3))
        x = g18_tensor("x2").clone()
        phi(x).sum().backward()
        for i in range(3):
            assert phi.net[i].iresblock.geom_p.grad is None and phi.net[i].iresblock.lamb.grad is None
    else:
        assert [tuple(ref[f"net.0.{k}"].shape) for k in "uwb"] == [(1, 3), (1, 3), (1,)]


def test_construction_follows_the_reference(shw):
    """the same generator state gives the reference's initial state, bit for bit: kaiming-uniform weights, the last
    layer / 1000, uniform biases, u and v from 200 power iterations on a normal draw; Planar: uniform u then w, b = 0"""
    for case in CASES:
        torch.manual_seed(0)
        if case == "planar":
            phi = shw.Norm_Flow_structure(3, "Planar", 3)
        elif case == "res":
            phi = shw.Norm_Flow_structure(3, "Residual", 3)
        else:
            phi = shw.Norm_Flow_structure_optuna(3, "Residual", 3, 5, 3)
        for name, t in g18_state(case).items():
            assert torch.equal(phi.state_dict()[name], t), (case, name)
    with pytest.raises(ValueError, match="Flow name is not valid"):
        shw.Norm_Flow_structure(3, "Spline", 3)
    with pytest.raises(ValueError, match="Flow name is not valid"):
        shw.Norm_Flow_structure_optuna(3, "Spline", 3)
    sig = shw.Norm_Flow_structure_optuna(flow_name="Residual")
    assert (sig.Residual_hidden_units, sig.Residual_hidden_layers, len(sig.net)) == (8, 3, 3)
    assert len(shw.Norm_Flow_structure().net) == 3 and shw.Norm_Flow_structure().flow_name == "Planar"


def test_planar_sums_over_axis_one(shw):
    """(B, N, 3): axis 1 is the point axis, every cloud is translated as a whole; (N, 3): the usual planar flow"""
    phi = g18_module(shw, "planar")
    x3, x2 = g18_tensor("x3"), g18_tensor("x2")
    with torch.no_grad():
        shift, move = phi(x3) - x3, phi(x2) - x2
    assert float((shift - shift[:, :1]).abs().max()) <= 1e-6
    assert float(shift[:, 0].abs().max()) > 1e-3
    assert float((shift[0, 0] - shift[1, 0]).abs().max()) > 1e-4          # ... each cloud by its own vector
    assert float((move - move[:1]).abs().max()) > 1e-2


def test_fresh_residual_structure_is_lipschitz_normalised(shw):
    torch.manual_seed(3)
    phi = shw.Norm_Flow_structure(3, "Residual", 3)
    lins = [m for m in phi.modules() if hasattr(m, "compute_weight")]
    assert len(lins) == 21
    above = 0
    for m in lins:
        sigma = torch.dot(m.u, torch.mv(m.weight.detach(), m.v))
        assert float(m.scale) == float(sigma)
        if float(m.scale) > COEFF:
            above += 1
            top = float(torch.linalg.svdvals(m.compute_weight().detach())[0])
            assert top <= COEFF * (1 + 1e-3), (float(m.scale), top)     # the margin: power iteration's convergence
    assert 0 < above < len(lins)
    assert max(float(m.weight.abs().max()) for m in lins[6::7]) < 1e-3  # the last layer of each flow starts near zero
    with torch.no_grad():
        for m in lins:
            m.weight.mul_(1.5)
    phi.update_lipschitz(n_iterations=5)
    for m in lins:
        assert abs(float(m.u.norm()) - 1) <= 1e-6 and abs(float(m.v.norm()) - 1) <= 1e-6
        assert float(m.scale) == float(torch.dot(m.u, torch.mv(m.weight.detach(), m.v)))


@pytest.mark.parametrize("case", ["res", "res53"])
def test_packing(shw, case):
    """the composed op on the packed effective parameters is the layer-by-layer module path, and the gradient of the
    packed buffer, pushed through the packing, is the layer-by-layer gradient of every raw parameter"""
    phi = g18_module(shw, case)
    hidden, layers = phi.hidden_units, phi.hidden_layers
    x, cot = g18_tensor("x3"), g18_tensor("c3")
    phi.zero_grad()
    (phi.forward_layers(x) * cot).sum().backward()
    by_layer = {n: p.grad.clone() for n, p in phi.named_parameters() if p.grad is not None}
    y_layers = phi.forward_layers(x).detach()
    phi.zero_grad()
    packed = phi.packed_params()
    assert packed.shape == (3 * shw.residual_param_count(hidden, layers),)
    y = shw.residual_flow_composed(x, packed, hidden, layers, 3)
    assert max_dev(y.detach(), y_layers) <= BOUND
    (g_packed,) = torch.autograd.grad((y * cot).sum(), packed, retain_graph=True)
    packed.backward(g_packed)
    got = {n: p.grad for n, p in phi.named_parameters() if p.grad is not None}
    assert sorted(got) == sorted(by_layer)
    for name, ref in by_layer.items():
        assert max_dev(got[name], ref) <= BOUND, name
    # the layout: gamma, W_eff row-major, bias of the first layer of the first flow
    lin = phi.net[0].iresblock.nnet.net[1]
    beta = phi.net[0].iresblock.nnet.net[0].beta
    assert torch.allclose(packed[0], torch.nn.functional.softplus(beta)[0])
    assert torch.allclose(packed[1:1 + 3 * hidden].view(hidden, 3), lin.compute_weight())
    assert torch.allclose(packed[1 + 3 * hidden:1 + 4 * hidden], lin.bias)
    with pytest.raises(ValueError):
        shw.residual_flow_composed(x, packed[:-1], hidden, layers, 3)


def test_composed_path_is_what_the_module_runs_off_the_device(shw):
    """CPU and float64 inputs take the composed path, whatever `fused` says; a non-contiguous view is fine"""
    phi = g18_module(shw, "res")
    x = g18_tensor("x3")
    want = shw.residual_flow_composed(x, phi.packed_params(), 8, 7, 3)
    assert torch.equal(phi(x), want)
    wide = torch.randn(2, 70, 6)
    wide[..., ::2] = x
    assert torch.equal(phi(wide[..., ::2]), want)
    phi64 = g18_module(shw, "res").double()
    y64 = phi64(x.double())
    assert y64.dtype == torch.float64 and max_dev(want, y64) <= BOUND
    with pytest.raises((RuntimeError, TypeError)):
        shw.residual_flow(x, phi.packed_params(), 8, 7, 3)       # the fused op itself has no CPU form


def test_c_entries_and_envelope(shw):
    import os
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "shw.h")).read()
    for name in ("shw_flow_residual_supported", "shw_flow_residual_param_count", "shw_flow_residual_workspace_bytes",
                 "shw_flow_residual_forward", "shw_flow_residual_backward"):
        assert re.search(r"SHW_API\s+\w+\s+%s\s*\(" % name, header), name
        assert name in shw._lib.EXPORTED_SYMBOLS
    lib = shw._lib.load()
    for dim in (2, 3, 4):
        for hidden in (0, 1, 8, 32, 33):
            for layers in (1, 2, 7, 8, 9):
                for flows in (0, 1, 16, 17):
                    inside = dim == 3 and 1 <= hidden <= 32 and 2 <= layers <= 8 and 1 <= flows <= 16
                    assert lib.shw_flow_residual_supported(dim, hidden, layers, flows) == int(inside)
                    assert shw.residual_flow_supported(dim, hidden, layers, flows) == inside
                    if dim == 3 and not inside:             # refused before any HIP call
                        assert lib.shw_flow_residual_forward(8, 8, 64, hidden, layers, flows, 8, None) == 1
                        assert lib.shw_flow_residual_backward(8, 8, 8, 64, hidden, layers, flows, 8, 8, 8, None) == 1
                        assert lib.shw_flow_residual_workspace_bytes(64, hidden, layers, flows) == 0
    for hidden, layers in ((8, 7), (5, 3), (32, 8), (1, 2)):
        assert lib.shw_flow_residual_param_count(hidden, layers) == shw.residual_param_count(hidden, layers)
    assert shw.residual_param_count(8, 7) == 426
    assert lib.shw_flow_residual_param_count(33, 7) == 0
    # one partial vector per 64 points up to the cap; null pointers and a missing workspace are refused
    assert lib.shw_flow_residual_workspace_bytes(4099, 8, 7, 3) == 65 * 3 * 426 * 4
    assert lib.shw_flow_residual_workspace_bytes(1 << 24, 8, 7, 3) == 2048 * 3 * 426 * 4
    assert lib.shw_flow_residual_workspace_bytes(0, 8, 7, 3) == 0
    assert lib.shw_flow_residual_forward(None, 8, 64, 8, 7, 3, 8, None) == 1
    assert lib.shw_flow_residual_forward(8, 8, -1, 8, 7, 3, 8, None) == 1
    assert lib.shw_flow_residual_forward(8, 8, 0, 8, 7, 3, 8, None) == 0
    assert lib.shw_flow_residual_backward(8, 8, None, 64, 8, 7, 3, 8, 8, 8, None) == 1
    assert lib.shw_flow_residual_backward(8, 8, 8, 64, 8, 7, 3, 8, 8, None, None) == 1
    assert lib.shw_flow_residual_backward(8, 8, 8, 64, 8, 7, 3, None, None, None, None) == 0
