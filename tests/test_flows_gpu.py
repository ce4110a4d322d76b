"""GPU checks of the fused sphere map (csrc/shw_flow.hip flow_forward_kernel, flow_backward_kernel,
flow_param_reduce_kernel; flows.py residual_flow, Norm_Flow_structure) against the composed path in float64.

Bound (tests/helpers/flow_cases.py): a float32 result against the composed path in float64 on the same float32 parameters
and inputs, per tensor, on max |error| / max |reference entry|; the bound is 4 x the deviation of the FLOAT32 composed path
from the float64 one on the same data, computed here, with a floor of 1e-6.

Every test calls shw.residual_flow or shw.Norm_Flow_structure, which did not exist before: without the feature each fails.

Measured on MI355X (worst over the cases): sizes and shapes: values 4.3e-7, d/dx 3.3e-7, packed-parameter
gradient 3.2e-7 (bounds 1.0e-6 to 3.4e-6; the worst are all at hidden = 1, 16 flows); saturated inputs 1.1e-7 / 9.0e-8 /
2.7e-7; fixture on the device: every weight and bias tensor at most 6.9e-7 from float64 and 9.2e-7 from the reference's
own float32 gradients (bounds 1.0e-6 to 1.1e-6), the stacked betas 4.4e-7 / 7.9e-7; taken one by one, single betas are up
to 5.5e-6 off relative to themselves, as the float32 composed path's are (7.2e-6 on the CPU, 5.3e-6 on the device): see
`by_family`; criterion after 2 x 2 ascent steps: loss 4.8e-8, mapped clouds 1.3e-7 (composed path: 4.8e-8, 9.0e-8),
graphed run bit-identical to the eager one.
"""
import pytest
import torch

from helpers.flow_cases import (INPUT_SHAPES, SHAPES, bound_of, composed_reference, g18_grads, g18_module, g18_tensor,
                                max_dev, random_packed, references)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def shw():
    import shw_amd
    shw_amd._lib.load()
    return shw_amd


def fused(shw, x, packed, cot, hidden, layers, flows, want_x=True, want_p=True):
    """value, d/dx, d/dpacked of sum(residual_flow(x) * cot) on the device (None where not asked for)"""
    xd = x.to(DEV).requires_grad_(want_x)
    pd = packed.to(DEV).requires_grad_(want_p)
    y = shw.residual_flow(xd, pd, hidden, layers, flows)
    assert y.shape == x.shape and y.dtype == torch.float32 and y.is_contiguous()
    (y * cot.to(DEV)).sum().backward()
    return y.detach(), xd.grad, pd.grad


def check(label, got, f64, f32):
    for name, g, r, f in zip(("value", "d/dx", "d/dparams"), got, f64, f32):
        assert torch.isfinite(g).all(), (label, name)
        worst, bound = max_dev(g, r), bound_of(f, r)
        print(f"{label} {name}: gpu {worst:.2e} bound {bound:.2e}")
        assert worst <= bound, (label, name, worst, bound)


@pytest.mark.parametrize("shape", INPUT_SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("hidden,layers,flows", SHAPES)
def test_values_and_gradients_against_float64(shw, hidden, layers, flows, shape):
    x, packed, cot, f64, f32 = references(shw, shape, hidden, layers, flows)
    got = fused(shw, x, packed, cot, hidden, layers, flows)
    check(f"H={hidden} K={layers} F={flows} {shape}", got, f64, f32)


@pytest.mark.parametrize("hidden,layers,flows", [(8, 7, 3), (5, 2, 2), (32, 8, 2)])
@pytest.mark.parametrize("shape", [(65, 3), (3, 341, 3)], ids=lambda s: "x".join(map(str, s)))
def test_only_the_gradients_asked_for_and_the_same_bits(shw, hidden, layers, flows, shape):
    """x only, parameters only (the inner ascent's case), both: what a variant produces is, bit for bit, what `both`
    produces"""
    x, packed, cot, _, _ = references(shw, shape, hidden, layers, flows)
    y, gx, gp = fused(shw, x, packed, cot, hidden, layers, flows)
    y1, gx1, gp1 = fused(shw, x, packed, cot, hidden, layers, flows, want_p=False)
    y2, gx2, gp2 = fused(shw, x, packed, cot, hidden, layers, flows, want_x=False)
    assert gp1 is None and gx2 is None
    assert torch.equal(y, y1) and torch.equal(y, y2)
    assert torch.equal(gx, gx1) and torch.equal(gp, gp2)
    with torch.no_grad():
        assert torch.equal(shw.residual_flow(x.to(DEV), packed.to(DEV), hidden, layers, flows), y)


@pytest.mark.parametrize("hidden,layers,flows", [(8, 7, 3), (12, 4, 3)])
def test_saturated_activations_stay_finite(shw, hidden, layers, flows):
    """+-1e4, +-50, 0 and subnormal coordinates: sigmoid saturates to exactly 0 and 1, nothing becomes NaN or inf, and
    the results are within the bound of the float64 path"""
    special = torch.tensor([1e4, -1e4, 50.0, -50.0, 0.0, -0.0, 1e-40, -1e-40, 1.0, -1.0, 3e-39, 88.0, -88.0, 104.0, -104.0])
    g = torch.Generator().manual_seed(5)
    x = special[torch.randint(len(special), (130, 3), generator=g)]
    x[:len(special)] = special[:, None]
    cot = torch.randn(130, 3, generator=g)
    packed = random_packed(hidden, layers, flows)
    f64 = composed_reference(shw, x, packed, cot, hidden, layers, flows, torch.float64)
    f32 = composed_reference(shw, x, packed, cot, hidden, layers, flows, torch.float32)
    assert all(torch.isfinite(t).all() for t in f64)
    check(f"saturation H={hidden}", fused(shw, x, packed, cot, hidden, layers, flows), f64, f32)


def by_family(named):
    """[(name, tensor)] of gradients in parameter order -> the same with the (1,) gradients of the `beta`s stacked into one
    tensor `beta` at the end.  Weights and biases stay one tensor each.  Why: the rule measures an error against the largest
    entry of its tensor.  A beta's gradient is ONE number, a sum over all points and units whose terms cancel (here to
    1e-2 .. 1e-3 of their size), so any float32 evaluation of it carries a relative error of that cancellation times 6e-8
    -- the float32 composed path itself is 7.2e-6 off on one beta of this fixture on the CPU and 5.3e-6 on the device --
    and as a tensor of its own the rule would compare two independent draws of that rounding error.  Stacked, the betas
    are measured like every other tensor, against the largest gradient among them."""
    rest = [(n, t) for n, t in named if not n.endswith(".beta")]
    betas = [t.reshape(-1) for n, t in named if n.endswith(".beta")]
    return rest + [("beta", torch.cat(betas))]


@pytest.mark.parametrize("xk,ck", [("x3", "c3"), ("x2", "c2")])
@pytest.mark.parametrize("case", ["res", "res53"])
def test_fixture_on_the_device(shw, case, xk, ck):
    """the module loaded from the reference's snapshot, on the reference's inputs, fused path: output, d/dx and the
    gradient of every parameter (the betas as one tensor: `by_family`) against the float64 composed path evaluated on the
    fixture's data, and against what the reference itself stored (float32), both with the rule's bound"""
    x0, cot = g18_tensor(xk), g18_tensor(ck)
    results = {}
    for name, phi, x in (("gpu", g18_module(shw, case).to(DEV), x0.to(DEV)),
                         ("f64", g18_module(shw, case).double(), x0.double()),
                         ("f32", g18_module(shw, case), x0.clone())):
        phi.fused = name == "gpu"
        x.requires_grad_()
        y = phi(x)
        (y * cot.to(x.device, x.dtype)).sum().backward()
        grads = [(n, p.grad.detach().cpu()) for n, p in phi.named_parameters() if p.grad is not None]
        results[name] = [("value", y.detach().cpu()), ("d/dx", x.grad.cpu())] + by_family(grads)
    assert results["gpu"][0][1].dtype == torch.float32 and results["f64"][0][1].dtype == torch.float64
    ref = g18_grads(case, xk)
    assert [n for n, p in phi.named_parameters() if p.grad is not None] == list(ref)
    stored = [("value", g18_tensor(f"{case}.{xk}.train")), ("d/dx", g18_tensor(f"{case}.{xk}.grad_x"))]
    stored += by_family(list(ref.items()))
    missed = []
    for (name, g), (_, r), (_, f), (_, s) in zip(results["gpu"], results["f64"], results["f32"], stored):
        bound = bound_of(f, r)
        to64, to_ref = max_dev(g, r), max_dev(g, s)
        print(f"fixture {case} {xk} {name}: gpu to float64 {to64:.2e} to the reference {to_ref:.2e} bound {bound:.2e}")
        if to64 > bound or to_ref > bound:
            missed.append((name, to64, to_ref, bound))
    assert not missed, missed


def test_non_contiguous_input(shw):
    x, packed, cot, _, _ = references(shw, (3, 341, 3), 8, 7, 3)
    wide = torch.zeros(3, 682, 3)
    wide[:, ::2] = x
    wide = wide.to(DEV)
    view = wide[:, ::2]
    assert not view.is_contiguous()
    y, gx, gp = fused(shw, x, packed, cot, 8, 7, 3)
    leaf = wide.clone().requires_grad_()
    pd = packed.to(DEV).requires_grad_()
    yv = shw.residual_flow(leaf[:, ::2], pd, 8, 7, 3)
    (yv * cot.to(DEV)).sum().backward()
    assert torch.equal(yv.detach(), y) and torch.equal(pd.grad, gp)
    assert torch.equal(leaf.grad[:, ::2], gx) and not leaf.grad[:, 1::2].any()


@pytest.mark.parametrize("hidden,layers,flows", [(8, 7, 3), (32, 8, 2)])
def test_parameter_gradients_are_the_same_bits_on_every_run(shw, hidden, layers, flows):
    x, packed, cot, _, _ = references(shw, (4099, 3), hidden, layers, flows)
    first = fused(shw, x, packed, cot, hidden, layers, flows)
    second = fused(shw, x, packed, cot, hidden, layers, flows)
    for a, b in zip(first, second):
        assert torch.equal(a, b)


def test_envelope(shw):
    lib = shw._lib.load()
    x = torch.randn(65, 3, device=DEV)
    for hidden, layers, flows in ((33, 7, 3), (8, 9, 3), (8, 1, 3), (8, 7, 17), (0, 7, 3)):
        assert lib.shw_flow_residual_supported(3, hidden, layers, flows) == 0
        count = max(flows * shw.residual_param_count(max(hidden, 1), layers), 1)
        with pytest.raises(ValueError, match="hidden <= 32"):
            shw.residual_flow(x, torch.zeros(count, device=DEV), hidden, layers, flows)
    assert lib.shw_flow_residual_supported(3, 32, 8, 16) == 1
    with pytest.raises(ValueError, match="dimension 3"):
        shw.residual_flow(torch.randn(65, 4, device=DEV), torch.zeros(426, device=DEV), 8, 7, 1)
    with pytest.raises(ValueError):
        shw.residual_flow(x, torch.zeros(425, device=DEV), 8, 7, 1)
    with pytest.raises(TypeError):
        shw.residual_flow(x.double(), torch.zeros(426, device=DEV), 8, 7, 1)
    # a width outside the envelope: the module takes the composed path on the device
    torch.manual_seed(11)
    phi = shw.Norm_Flow_structure_optuna(3, "Residual", 2, Residual_hidden_units=33, Residual_hidden_layers=3).to(DEV)
    with torch.no_grad():
        want = shw.residual_flow_composed(x, phi.packed_params(), 33, 3, 2)
        assert torch.equal(phi(x), want)
    # ... and one inside takes the kernels: not the composed path's bits, but its values
    phi = shw.Norm_Flow_structure_optuna(3, "Residual", 2, Residual_hidden_units=32, Residual_hidden_layers=3).to(DEV)
    with torch.no_grad():
        want = shw.residual_flow_composed(x, phi.packed_params(), 32, 3, 2)
        assert torch.equal(phi(x), shw.residual_flow(x, phi.packed_params(), 32, 3, 2))
        assert max_dev(phi(x), want) <= 1e-5


def criterion_run(shw, x, y, frames, fused_path=True, graph=False, dtype=torch.float32):
    """two trainer-level calls of the phi-max criterion (max_iter=2) from the same start, on fixed direction frames ->
    the two losses and the mapped clouds of the second call"""

    class FixedDirections(shw.SlicedSphereW):                    # SlicedSphereW(dev, 2, 16) without the draw
        def forward(self, a, b):
            pair = shw.ssw_pair_losses(a, b, frames.to(a.dtype), self.p)
            return torch.pow(pair, 1.0 / self.p).sum() / a.shape[0]

    torch.manual_seed(21)
    phi = shw.Norm_Flow_structure(3, "Residual", 3)
    with torch.no_grad():                                         # off the near-identity start: the last layers at full scale
        for flow in phi.net:
            flow.iresblock.nnet.net[-1].weight.mul_(300.0)
    phi = phi.to(DEV, dtype)
    phi.fused = fused_path
    opt = torch.optim.Adam(phi.parameters(), lr=1e-3, capturable=True)
    crit = shw.max_cos_disimilarity_wassersten_distance(phi, FixedDirections(DEV, 2, 16), DEV, opt, max_iter=2, graph=graph)
    losses = []
    for _ in range(2):
        loss, a, b = crit(x.to(dtype), y.to(dtype), "train")
        losses.append(loss.detach().clone())
    return torch.stack(losses), a.detach(), b.detach()


def test_criterion_eager_composed_and_graphed(shw):
    """max_cos_disimilarity_wassersten_distance with phi = Norm_Flow_structure("Residual") at B = 2, N = 128, 16 fixed
    slices, max_iter = 2: the eager fused run against the same criterion with phi on the composed path -- both within the
    rule's bound of the composed float64 run, the bound taken from the float32 composed run -- and the graphed run (the
    first call warms up, the second captures and replays) against the eager one bit for bit"""
    g = torch.Generator().manual_seed(31)
    x = torch.nn.functional.normalize(torch.randn(2, 128, 3, generator=g), dim=-1).to(DEV)
    y = torch.nn.functional.normalize(torch.randn(2, 128, 3, generator=g), dim=-1).to(DEV)
    frames = torch.linalg.qr(torch.randn(2, 16, 3, 2, generator=g))[0].to(DEV)
    eager = criterion_run(shw, x, y, frames)
    composed = criterion_run(shw, x, y, frames, fused_path=False)
    previous = shw.enable_float64(True)
    try:
        exact = criterion_run(shw, x, y, frames, fused_path=False, dtype=torch.float64)
    finally:
        shw.enable_float64(previous)
    for name, e, c, r in zip(("losses", "phi(first)", "phi(second)"), eager, composed, exact):
        worst, bound = max_dev(e, r), bound_of(c, r)
        print(f"criterion {name}: fused {worst:.2e} composed {max_dev(c, r):.2e} bound {bound:.2e}")
        assert torch.isfinite(e).all() and worst <= bound, (name, worst, bound)
    graphed = criterion_run(shw, x, y, frames, graph=True)
    for e, r in zip(eager, graphed):
        assert torch.equal(e, r)
