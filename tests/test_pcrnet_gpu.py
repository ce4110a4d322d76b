"""Device checks of the fused PointNet trunk (csrc/shw_pointnet.hip through shw.pointnet_max_features) and of shw.PCRNet.

Every test goes through shw.pointnet_max_features, shw.MLP_Architecture or shw.PCRNet: without the feature each fails on
the missing name.

Bound (tests/helpers/pcrnet_cases.py): float32 on the device against the composed path in float64 on the same float32 data,
per tensor, on max |error| / max |reference entry|; 4 x the deviation of the float32 composed CPU path from the float64
one on the same case, floor 1e-6 (1e-5 for PCRNet).  Parameter gradients are compared tensor by tensor (W1, b1, ..., W5,
b5).  Every case asserts the margin condition in float64 first, so the arg-max is compared exactly and in every channel.

Measured on an MI355X, worst over the trunk cases: values 4.4e-7, point gradients 4.2e-7, parameter gradients 4.3e-7, at
most 0.42 of the bound (33 clouds at emb = 1024: 0.37); PCRNet 0.28 (k = 1) and 0.22 (k = 3) of its bound; fixture G19 on the device: trunk 4.3e-7, PCRNet
outputs at most 4.5e-6 (`r`), gradients 8.5e-7.  Each test prints its figures (pytest -s).
"""
import pytest
import torch

from helpers import pcrnet_cases as pc
from helpers.pcrnet_cases import bound_of, max_dev

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
P = pc.POINT_TILE
# (emb, B, N, seed): seeds for which the float64 reference meets the margin condition (pcrnet_cases.find_seed)
WIDTHS = [(32, 1, 70, 0), (32, 3, 70, 0), (96, 1, 70, 0), (96, 3, 70, 2), (1024, 1, 33, 37), (1024, 3, 17, 971)]
EDGES = [(96, 2, 1, 0), (96, 2, 33, 2), (96, 2, P - 1, 3), (96, 2, P, 4), (96, 2, P + 1, 1), (96, 2, 2 * P + 1, 2)]
MAIN = (96, 3, 70, 2)
DOUBLED = (96, 2, 130, 2)
DEAD = (96, 2, 70, 1)
PCRNET_SEED = 36


@pytest.fixture(scope="module")
def shw():
    import shw_amd
    shw_amd._lib.load()
    return shw_amd


def fused(shw, x, params, cot, emb, want_x=True, want_p=True):
    """(feat, argmax, d/dx, d/dparams) of sum(pointnet_max_features(x) * cot) on the device (None where not asked for)"""
    xd = x.to(DEV).requires_grad_(want_x)
    pd = params.to(DEV).requires_grad_(want_p)
    feat, argmax = shw.pointnet_max_features(xd, pd, emb, return_argmax=True)
    assert feat.shape == (x.shape[0], emb) and feat.dtype == torch.float32 and argmax.dtype == torch.int32
    (feat * cot.to(DEV)).sum().backward()
    return feat.detach(), argmax, xd.grad, pd.grad


def tensors(shw, emb, triple):
    """(feat, gx, gparams) -> name -> tensor, the parameter gradient split into its ten tensors"""
    out = {"value": triple[0], "d/dx": triple[1]}
    for n, (weight, bias) in enumerate(shw.unpack_pointnet_params(triple[2], emb), start=1):
        out[f"dW{n}"], out[f"db{n}"] = weight, bias
    return out


def check(shw, label, emb, got, f64, f32):
    worst = 0.0
    got, f64, f32 = tensors(shw, emb, got), tensors(shw, emb, f64), tensors(shw, emb, f32)
    for name in f64:
        bound, dev = bound_of(f32[name], f64[name]), max_dev(got[name], f64[name])
        worst = max(worst, dev / bound)
        print(f"{label} {name}: device {dev:.2e} bound {bound:.2e}")
        assert dev <= bound, (label, name, dev, bound)
    return worst


@pytest.mark.parametrize("emb,B,N,seed", WIDTHS + EDGES)
def test_parity_with_float64(shw, emb, B, N, seed):
    """values, arg-max and both gradients; WIDTHS: one, three and 32 row tiles of the last layer, one and three clouds;
    EDGES: one point, one partial 32-point tile, P - 1, P, P + 1 and 2 P + 1 points for the kernel's point tile P = 64"""
    c = pc.case(shw, emb, B, N, seed)
    feat, argmax, gx, gp = fused(shw, c["x"], c["params"], c["cot"], emb)
    assert torch.equal(argmax.cpu().long(), c["argmax"]), (argmax.cpu().long() != c["argmax"]).nonzero()[:8]
    assert int(argmax.min()) >= 0 and int(argmax.max()) < N
    worst = check(shw, f"emb={emb} B={B} N={N}", emb, (feat, gx, gp), c["f64"], c["f32"])
    print(f"emb={emb} B={B} N={N}: worst device / bound {worst:.2f}")


def test_several_clouds_per_backward_workgroup(shw):
    """emb = 1024 with 33 clouds: the backward's workgroups take two clouds each (32 ranges of clouds at most at this
    width), so dW5 and db5 add up in registers over a range and the hidden layers' partial vectors are added to, not only
    stored.  The clouds are the one-cloud case's points in 33 different orders, with 33 different cotangents."""
    emb, _, N, seed = WIDTHS[4]
    c = pc.case(shw, emb, 1, N, seed, copies=33)
    assert c["x"].shape == (33, N, 3) and len({tuple(row.tolist()) for row in c["argmax"][:, :8]}) > 1
    feat, argmax, gx, gp = fused(shw, c["x"], c["params"], c["cot"], emb)
    assert torch.equal(argmax.cpu().long(), c["argmax"])
    worst = check(shw, "33 clouds", emb, (feat, gx, gp), c["f64"], c["f32"])
    print(f"33 clouds: worst device / bound {worst:.2f}")


def test_doubled_cloud_takes_the_lower_copy(shw):
    """every point occurs at n and at n + N / 2 (other lanes, and for n < 64 another tile): the arg-max is the lower index,
    no gradient reaches the upper copies, and the sums over each pair equal the float64 reference's pair sums"""
    emb, B, N, seed = DOUBLED
    c = pc.case(shw, emb, B, N, seed, doubled=True)
    feat, argmax, gx, gp = fused(shw, c["x"], c["params"], c["cot"], emb)
    assert torch.equal(argmax.cpu().long(), c["argmax"]) and int(argmax.max()) < N // 2
    assert not gx[:, N // 2:].any()
    pairs = lambda g: g[:, :N // 2] + g[:, N // 2:]
    got, f64, f32 = ((t[0], pairs(t[1]), t[2]) for t in ((feat, gx.cpu(), gp), c["f64"], c["f32"]))
    check(shw, "doubled", emb, got, f64, f32)


def test_dead_channels_pass_nothing(shw):
    """the last bias at -10 on the upper half of the channels: their features are exactly 0, their dW5 rows and db5 entries
    exactly 0, and x and W1..W4 receive exactly what the live half alone sends"""
    emb, B, N, seed = DEAD
    c = pc.case(shw, emb, B, N, seed, dead_half=True)
    feat, argmax, gx, gp = fused(shw, c["x"], c["params"], c["cot"], emb)
    half = emb // 2
    assert not feat[:, half:].any() and bool((feat[:, :half] >= 0).all())
    assert int(argmax.min()) >= 0 and int(argmax.max()) < N
    assert torch.equal(argmax[:, :half].cpu().long(), c["argmax"][:, :half])
    dW5, db5 = shw.unpack_pointnet_params(gp, emb)[4]
    assert not dW5[half:].any() and not db5[half:].any()
    check(shw, "dead half", emb, (feat, gx, gp), c["f64"], c["f32"])
    # the same call with the dead half's cotangent set to 0 and to something else: bit-identical gradients
    other = c["cot"].clone()
    other[:, half:] = 7.0
    again = fused(shw, c["x"], c["params"], other, emb)
    assert torch.equal(again[2], gx) and torch.equal(again[3], gp)


def test_only_the_gradients_asked_for(shw):
    emb, B, N, seed = MAIN
    c = pc.case(shw, emb, B, N, seed)
    both = fused(shw, c["x"], c["params"], c["cot"], emb)
    only_x = fused(shw, c["x"], c["params"], c["cot"], emb, want_p=False)
    only_p = fused(shw, c["x"], c["params"], c["cot"], emb, want_x=False)
    assert only_x[3] is None and only_p[2] is None
    assert torch.equal(only_x[0], both[0]) and torch.equal(only_p[0], both[0])
    assert torch.equal(only_x[2], both[2]) and torch.equal(only_p[3], both[3])


def test_two_runs_give_the_same_bits(shw):
    for emb, B, N, seed in (MAIN, WIDTHS[-1]):
        c = pc.case(shw, emb, B, N, seed)
        a = fused(shw, c["x"], c["params"], c["cot"], emb)
        b = fused(shw, c["x"], c["params"], c["cot"], emb)
        assert all(torch.equal(s, t) for s, t in zip(a, b))


def test_graph_replay_equals_eager(shw):
    """forward and backward captured once, replayed on other points and cotangents: the eager bits"""
    emb, B, N, seed = MAIN
    c = pc.case(shw, emb, B, N, seed)
    xs = c["x"].to(DEV).requires_grad_()
    ps = c["params"].to(DEV).requires_grad_()
    cs = c["cot"].to(DEV).clone()

    def step():
        feat = shw.pointnet_max_features(xs, ps, emb)
        return (feat,) + torch.autograd.grad((feat * cs).sum(), (xs, ps))

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = step()
    g = torch.Generator().manual_seed(5)
    x2, cot2 = torch.randn(B, N, 3, generator=g), torch.randn(B, emb, generator=g)
    with torch.no_grad():
        xs.copy_(x2)
        cs.copy_(cot2)
    graph.replay()
    torch.cuda.synchronize()
    eager = fused(shw, x2, c["params"], cot2, emb)
    assert torch.equal(captured[0], eager[0]) and torch.equal(captured[1], eager[2]) and torch.equal(captured[2], eager[3])


@pytest.mark.parametrize("k", [1, 3])
def test_pcrnet_against_float64(shw, k):
    """shw.PCRNet fused on the device, emb = 64, B = 2, N = 130: the five outputs and the gradient of every parameter
    against the composed float64 CPU run, which asserts the margin condition on the input of every trunk call"""
    import copy
    model, template, source, cot, f64, f32 = pc.pcrnet_case(shw, k, PCRNET_SEED)
    device_model = copy.deepcopy(model).to(DEV)
    assert device_model.feature_model.fused
    seen = []
    original = shw.pcrnet.pointnet_max_features
    try:
        shw.pcrnet.pointnet_max_features = lambda *a, **kw: (seen.append(1), original(*a, **kw))[1]
        out, grads = pc.pcrnet_run(shw, device_model, template.to(DEV), source.to(DEV), cot.to(DEV), k)
    finally:
        shw.pcrnet.pointnet_max_features = original
    assert len(seen) == k + 1                          # the fused op ran: once for the template, once per iteration
    worst = 0.0
    for group, got, ref64, ref32 in (("out", out, f64[0], f32[0]), ("grad", grads, f64[1], f32[1])):
        assert list(got) == list(ref64)
        for name in ref64:
            bound, dev = bound_of(ref32[name], ref64[name], floor=1e-5), max_dev(got[name], ref64[name])
            worst = max(worst, dev / bound)
            assert dev <= bound, (k, group, name, dev, bound)
    print(f"PCRNet k={k}: worst device / bound {worst:.2f}")


@pytest.mark.parametrize("xk,ck", [("x270", "c270"), ("x11", "c11")])
def test_fixture_g19_trunk_on_the_device(shw, xk, ck):
    trunk = shw.MLP_Architecture(64)
    trunk.load_state_dict(pc.g19_trunk_state(), strict=True)
    trunk = trunk.to(DEV)
    x = pc.g19_tensor(xk).to(DEV).requires_grad_()
    y = trunk.pooled(x)
    (y * pc.g19_tensor(ck).to(DEV)).sum().backward()
    figures = {"value": max_dev(y.detach(), pc.g19_tensor(f"{xk}.pooled")),
               "d/dx": max_dev(x.grad, pc.g19_tensor(f"{xk}.grad_x")),
               "d/dtrunk": max_dev(torch.cat([p.grad.reshape(-1) for p in trunk.parameters()]),
                                   pc.g19_tensor(f"{xk}.grad_trunk"))}
    print(xk, {n: f"{v:.2e}" for n, v in figures.items()})
    assert all(v <= 1e-5 for v in figures.values()), figures


@pytest.mark.parametrize("k", [1, 3])
def test_fixture_g19_pcrnet_on_the_device(shw, k):
    model = pc.g19_model(shw).to(DEV)
    template, source = pc.g19_tensor("template").to(DEV).requires_grad_(), pc.g19_tensor("source").to(DEV).requires_grad_()
    out = model(template, source, k)
    (out["transformed_source"] * pc.g19_tensor("cot_source").to(DEV)).sum().backward()
    figures = {name: max_dev(value.detach(), pc.g19_tensor(f"pcrnet.k{k}.{name}")) for name, value in out.items()}
    figures["d/dtemplate"] = max_dev(template.grad, pc.g19_tensor(f"pcrnet.k{k}.grad_template"))
    figures["d/dsource"] = max_dev(source.grad, pc.g19_tensor(f"pcrnet.k{k}.grad_source"))
    figures["d/dtrunk"] = max_dev(torch.cat([p.grad.reshape(-1) for p in model.feature_model.parameters()]),
                                  pc.g19_tensor(f"pcrnet.k{k}.grad_trunk"))
    print(k, {n: f"{v:.2e}" for n, v in figures.items()})
    assert all(v <= 1e-5 for v in figures.values()), figures


def test_outside_the_envelope_takes_the_composed_path(shw):
    """emb = 48 is no multiple of 32: `pooled` computes what the composed path computes, bit for bit, and the fused op
    itself refuses"""
    torch.manual_seed(48)
    trunk = shw.MLP_Architecture(48).to(DEV)
    x = torch.randn(2, 70, 3, device=DEV)
    packed = trunk.packed_params()
    assert not trunk.uses_fused(x, packed)
    assert torch.equal(trunk.pooled(x), shw.pointnet_max_features_composed(x, packed, 48))
    with pytest.raises(ValueError):
        shw.pointnet_max_features(x, packed.detach(), 48)
    inside = shw.MLP_Architecture(64).to(DEV)
    assert inside.uses_fused(x, inside.packed_params())
    inside.fused = False
    assert not inside.uses_fused(x, inside.packed_params())
