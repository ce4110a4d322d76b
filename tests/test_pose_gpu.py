"""Device checks of the fused pose head and pose update (csrc/shw_pose.hip through shw.pose_head and shw.pose_update) and of
shw.PCRNet with `fused_head` / `fused_update` set.

Every test goes through shw.pose_head, shw.pose_update or a PCRNet flag: without the feature each fails on the missing name.

Bound (tests/helpers/pose_cases.py): float32 on the device against the composed path in float64 on the same float32 data,
per tensor, on max |error| / max |reference entry|; 4 x the deviation of the float32 composed CPU path from the float64
one on the same case, floor 1e-6 (1e-5 for PCRNet).  The head's parameter gradient is compared tensor by tensor (W1, b1,
..., W6, b6), and every head case asserts the margin condition in float64 first.  Each test prints its figures (pytest -s).

Measured on an MI355X, worst device error as a fraction of the bound: pose update 0.42 (N = 16 684, vectors x 1e-3), head
0.32 (B = 33), PCRNet with a flag or both 0.38 (k = 3, `fused_head`); fixture G19 with both flags: outputs at most 4.0e-6
(`r`), gradients 1.0e-6.
"""
import copy
import itertools

import pytest
import torch

from helpers import pcrnet_cases as pn
from helpers import pose_cases as pc
from helpers.pcrnet_cases import bound_of, max_dev

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BLOCK, MAX_BLOCKS = 256, 64                              # csrc/shw_pose.hip kPoseBlock, kPoseMaxBlocks
# (emb, widths, B, seed): seeds for which the float64 reference meets the margin condition (pose_cases.find_seed)
HEAD = [(32, pc.SMALL_WIDTHS, 1, 0), (32, pc.SMALL_WIDTHS, 33, 0), (32, pc.ALL_32, 65, 0),
        (96, pc.REFERENCE_WIDTHS, 3, 0), (1024, pc.REFERENCE_WIDTHS, 2, 0)]
HEAD_MAIN = HEAD[1]
UPDATE_SIZES = list(itertools.product((1, 3), (1, 63, 64, 65, 257, 4099))) + [(1, BLOCK * MAX_BLOCKS + 300)]
UPDATE_MAIN = (3, 257)
PCRNET_SEED = 36                                         # tests/test_pcrnet_gpu.py


@pytest.fixture(scope="module")
def shw():
    import shw_amd
    shw_amd._lib.load()
    return shw_amd


def compare(label, got, f64, f32, floor=1e-6):
    worst = 0.0
    for name in f64:
        bound, dev = bound_of(f32[name], f64[name], floor=floor), max_dev(got[name], f64[name])
        worst = max(worst, dev / bound)
        print(f"{label} {name}: device {dev:.2e} bound {bound:.2e}")
        assert dev <= bound, (label, name, dev, bound)
    return worst


# ------------------------------------------------------------------------------------------------ pose_update
def fused_update(shw, c, use=(True, True, True), want=(True, True, True, True)):
    return pc.run_update(shw.pose_update, c["inputs"], c["cots"], DEV, torch.float32, use, want)


def named_update(result):
    outs, grads = result
    named = {f"{n}'": t for n, t in zip(pc.UPDATE_OUTPUTS, outs)}
    named.update({f"d/d{n}": t for n, t in zip(pc.UPDATE_INPUTS, grads)})
    return named


@pytest.mark.parametrize("scale", [1.0, 1e-3, 1e3])
@pytest.mark.parametrize("B,N", UPDATE_SIZES)
def test_update_parity_with_float64(shw, B, N, scale):
    """values and all four gradients; one point, a partial wave, 64 +- 1, two workgroups, seventeen, and one size past the
    backward's cap of 64 workgroups per cloud; quaternion norms of about 1, 1e-3 and 1e3"""
    c = pc.update_case(shw, B, N, scale=scale)
    got = fused_update(shw, c)
    assert all(t.dtype == torch.float32 for t in got[0])
    worst = compare(f"B={B} N={N} scale={scale:g}", named_update(got), named_update(c["f64"]), named_update(c["f32"]))
    print(f"B={B} N={N} scale={scale:g}: worst device / bound {worst:.2f}")


def test_update_identity_quaternion_is_exact(shw):
    c = pc.update_case(shw, 3, 65, quaternion=(1.0, 0.0, 0.0, 0.0))
    (new_R, new_t, moved), _ = got = fused_update(shw, c)
    vector, est_R, est_t, source = (t.to(DEV) for t in c["inputs"])
    assert torch.equal(new_R, est_R) and torch.equal(new_t, est_t + vector[:, None, 4:])
    assert torch.equal(moved, source + vector[:, None, 4:])
    compare("identity", named_update(got), named_update(c["f64"]), named_update(c["f32"]))


def test_update_quaternion_without_real_part(shw):
    c = pc.update_case(shw, 3, 65, quaternion=(0.0, 0.6, -1.3, 0.4))
    compare("w = 0", named_update(fused_update(shw, c)), named_update(c["f64"]), named_update(c["f32"]))


def test_update_zero_quaternion_values(shw):
    """values only: R = I, source' = source + t (its gradient is F.normalize's 1e12-scaled one)"""
    inputs, _ = pc.update_inputs(3, 65, quaternion=(0.0, 0.0, 0.0, 0.0))
    vector, est_R, est_t, source = (t.to(DEV) for t in inputs)
    new_R, new_t, moved = shw.pose_update(vector, est_R, est_t, source)
    assert torch.equal(new_R, est_R) and torch.equal(new_t, est_t + vector[:, None, 4:])
    assert torch.equal(moved, source + vector[:, None, 4:])
    assert all(bool(torch.isfinite(t).all()) for t in (new_R, new_t, moved))


@pytest.mark.parametrize("use", [(False, False, True), (True, False, False), (False, True, False)])
def test_update_each_cotangent_on_its_own(shw, use):
    """only source', only est_R', only est_t': the absent cotangents are None in the backward, not zeros"""
    B, N = UPDATE_MAIN
    c = pc.update_case(shw, B, N)
    f64 = pc.run_update(shw.pose_update_composed, c["inputs"], c["cots"], "cpu", torch.float64, use)
    f32 = pc.run_update(shw.pose_update_composed, c["inputs"], c["cots"], "cpu", torch.float32, use)
    got = fused_update(shw, c, use)
    zero = lambda r: (r[0], [torch.zeros_like(t) if g is None else g for g, t in zip(r[1], c["inputs"])])
    compare(f"use={use}", named_update(zero(got)), named_update(zero(f64)), named_update(zero(f32)))
    if use == (True, False, False):
        assert not got[1][3].any()                      # nothing reaches the source through est_R'


def test_update_only_the_gradients_asked_for(shw):
    B, N = UPDATE_MAIN
    c = pc.update_case(shw, B, N)
    full = fused_update(shw, c)
    for k in range(4):
        want = tuple(j == k for j in range(4))
        outs, grads = fused_update(shw, c, want=want)
        assert all(torch.equal(a, b) for a, b in zip(outs, full[0]))
        assert all((g is None) != w for g, w in zip(grads, want))
        assert torch.equal(grads[k], full[1][k])


def test_update_two_runs_give_the_same_bits(shw):
    for B, N in (UPDATE_MAIN, UPDATE_SIZES[-1]):
        c = pc.update_case(shw, B, N)
        a, b = fused_update(shw, c), fused_update(shw, c)
        assert all(torch.equal(s, t) for s, t in zip(a[0] + a[1], b[0] + b[1]))


def capture(step):
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = step()
    return graph, captured


def test_update_graph_replay_equals_eager(shw):
    B, N = UPDATE_MAIN
    c = pc.update_case(shw, B, N)
    leaves = [t.to(DEV).requires_grad_() for t in c["inputs"]]
    cots = [t.to(DEV).clone() for t in c["cots"]]

    def step():
        outs = shw.pose_update(*leaves)
        return tuple(outs) + torch.autograd.grad(sum((o * k).sum() for o, k in zip(outs, cots)), leaves)

    graph, captured = capture(step)
    other = pc.update_case(shw, B, N, seed=1)
    with torch.no_grad():
        for dst, src in zip(leaves + cots, other["inputs"] + other["cots"]):
            dst.copy_(src)
    graph.replay()
    torch.cuda.synchronize()
    outs, grads = fused_update(shw, other)
    assert all(torch.equal(a, b) for a, b in zip(captured, outs + grads))


# ------------------------------------------------------------------------------------------------ pose_head
def fused_head(shw, c, widths, want=(True, True, True)):
    """(value, gtf, gsf, gparams) of sum(pose_head(...) * cot) on the device (None where not asked for)"""
    leaves = [c[n].to(DEV).requires_grad_(w) for n, w in zip(("tf", "sf", "params"), want)]
    y = shw.pose_head(*leaves, widths)
    assert y.shape == (c["tf"].shape[0], 7) and y.dtype == torch.float32
    (y * c["cot"].to(DEV)).sum().backward()
    return (y.detach(),) + tuple(t.grad for t in leaves)


@pytest.mark.parametrize("emb,widths,B,seed", HEAD)
def test_head_parity_with_float64(shw, emb, widths, B, seed):
    """values, both feature gradients and the twelve parameter gradients; one cloud, two and three batch tiles with a
    ragged last one, a width of three tiles, the reference's widths, and the trainer's K = 2048"""
    c = pc.head_case(shw, emb, widths, B, seed)
    got = fused_head(shw, c, widths)
    split = lambda t: pc.split_head_grads(shw, t, emb, widths)
    worst = compare(f"emb={emb} B={B}", split(got), split(c["f64"]), split(c["f32"]))
    print(f"emb={emb} widths={widths} B={B}: worst device / bound {worst:.2f}")


@pytest.mark.parametrize("layer", [1, 3, 5])
def test_head_dead_layer_passes_zeros(shw, layer):
    """all of one hidden layer's biases at -10: nothing is NaN, and what lies upstream of the layer -- both feature
    gradients, the layer's own and every earlier layer's parameters -- receives exactly 0"""
    emb, widths, B, seed = HEAD_MAIN
    c = pc.head_case(shw, emb, widths, B, seed, dead_layer=layer)
    got = fused_head(shw, c, widths)
    assert all(bool(torch.isfinite(t).all()) for t in got)
    named = pc.split_head_grads(shw, got, emb, widths)
    assert not named["d/dtemplate_features"].any() and not named["d/dsource_features"].any()
    for n in range(1, layer + 1):
        assert not named[f"dW{n}"].any() and not named[f"db{n}"].any(), n
    split = lambda t: pc.split_head_grads(shw, t, emb, widths)
    compare(f"dead layer {layer}", named, split(c["f64"]), split(c["f32"]))


def test_head_only_the_gradients_asked_for(shw):
    emb, widths, B, seed = HEAD_MAIN
    c = pc.head_case(shw, emb, widths, B, seed)
    full = fused_head(shw, c, widths)
    for want in ((True, False, False), (False, True, False), (False, False, True), (True, True, False)):
        got = fused_head(shw, c, widths, want)
        assert torch.equal(got[0], full[0])
        for g, f, w in zip(got[1:], full[1:], want):
            assert (g is None) != w and (g is None or torch.equal(g, f))


def test_head_two_runs_give_the_same_bits(shw):
    for emb, widths, B, seed in (HEAD_MAIN, HEAD[-1]):
        c = pc.head_case(shw, emb, widths, B, seed)
        a, b = fused_head(shw, c, widths), fused_head(shw, c, widths)
        assert all(torch.equal(s, t) for s, t in zip(a, b))


def test_head_graph_replay_equals_eager(shw):
    emb, widths, B, seed = HEAD_MAIN
    c = pc.head_case(shw, emb, widths, B, seed)
    leaves = [c[n].to(DEV).requires_grad_() for n in ("tf", "sf", "params")]
    cot = c["cot"].to(DEV).clone()

    def step():
        y = shw.pose_head(*leaves, widths)
        return (y,) + torch.autograd.grad((y * cot).sum(), leaves)

    graph, captured = capture(step)
    other = dict(c)
    other["tf"], other["sf"], _, other["cot"] = pc.head_inputs(emb, widths, B, seed + 1)
    with torch.no_grad():
        leaves[0].copy_(other["tf"])
        leaves[1].copy_(other["sf"])
        cot.copy_(other["cot"])
    graph.replay()
    torch.cuda.synchronize()
    eager = fused_head(shw, other, widths)
    assert all(torch.equal(a, b) for a, b in zip(captured, eager))


def test_head_outside_the_envelope_is_refused(shw):
    tf = torch.zeros(2, 48, device=DEV)
    with pytest.raises(ValueError):
        shw.pose_head(tf, tf, torch.zeros(shw.pose_head_param_count(48), device=DEV))
    tf = torch.zeros(2, 32, device=DEV)
    with pytest.raises(ValueError):
        shw.pose_head(tf, tf, torch.zeros(shw.pose_head_param_count(32, (40, 32, 32, 32, 32)), device=DEV), (40, 32, 32, 32, 32))
    with pytest.raises(ValueError):
        shw.pose_head(tf, tf, torch.zeros(5, device=DEV))
    with pytest.raises(TypeError):
        shw.pose_head(tf.double(), tf.double(), torch.zeros(shw.pose_head_param_count(32), device=DEV).double())


# ------------------------------------------------------------------------------------------------ the whole network
def count_calls(shw, name, seen):
    original = getattr(shw.pose, name)
    setattr(shw.pose, name, lambda *a, **kw: (seen.append(name), original(*a, **kw))[1])
    return original


@pytest.mark.parametrize("head,update", [(True, False), (False, True), (True, True)])
@pytest.mark.parametrize("k", [1, 3])
def test_pcrnet_with_the_flags_against_float64(shw, k, head, update):
    """shw.PCRNet on the device with either flag and with both, emb = 64, B = 2, N = 130: the five outputs and the gradient
    of every parameter against the composed float64 CPU run; the fused ops ran once per iteration"""
    model, template, source, cot, f64, f32 = pn.pcrnet_case(shw, k, PCRNET_SEED)
    device_model = copy.deepcopy(model).to(DEV)
    device_model.fused_head, device_model.fused_update = head, update
    seen = []
    originals = {name: count_calls(shw, name, seen) for name in ("pose_head", "pose_update")}
    try:
        out, grads = pn.pcrnet_run(shw, device_model, template.to(DEV), source.to(DEV), cot.to(DEV), k)
    finally:
        for name, fn in originals.items():
            setattr(shw.pose, name, fn)
    assert seen.count("pose_head") == (k if head else 0) and seen.count("pose_update") == (k if update else 0)
    worst = 0.0
    for group, got, ref64, ref32 in (("out", out, f64[0], f32[0]), ("grad", grads, f64[1], f32[1])):
        assert list(got) == list(ref64)
        worst = max(worst, compare(f"k={k} {group}", got, ref64, ref32, floor=1e-5))
    print(f"PCRNet k={k} fused_head={head} fused_update={update}: worst device / bound {worst:.2f}")


@pytest.mark.parametrize("k", [1, 3])
def test_fixture_g19_pcrnet_with_both_flags(shw, k):
    model = pn.g19_model(shw).to(DEV)
    model.fused_head = model.fused_update = True
    assert model.uses_fused_head(torch.zeros(2, 64, device=DEV))
    template, source = pn.g19_tensor("template").to(DEV).requires_grad_(), pn.g19_tensor("source").to(DEV).requires_grad_()
    out = model(template, source, k)
    (out["transformed_source"] * pn.g19_tensor("cot_source").to(DEV)).sum().backward()
    figures = {name: max_dev(value.detach(), pn.g19_tensor(f"pcrnet.k{k}.{name}")) for name, value in out.items()}
    figures["d/dtemplate"] = max_dev(template.grad, pn.g19_tensor(f"pcrnet.k{k}.grad_template"))
    figures["d/dsource"] = max_dev(source.grad, pn.g19_tensor(f"pcrnet.k{k}.grad_source"))
    figures["d/dtrunk"] = max_dev(torch.cat([p.grad.reshape(-1) for p in model.feature_model.parameters()]),
                                  pn.g19_tensor(f"pcrnet.k{k}.grad_trunk"))
    print(k, {n: f"{v:.2e}" for n, v in figures.items()})
    assert all(v <= 1e-5 for v in figures.values()), figures


def test_dropout_takes_the_composed_head(shw):
    """droput = 0.1 with the flags set: `linear` holds a Dropout, the head runs as `linear` itself, and in eval mode the
    model equals the flags-off one bit for bit in the head (the pose update is fused in one and composed in the other)"""
    model = pn.g19_model(shw, dropout=0.1).to(DEV).eval()
    template, source = pn.g19_tensor("template").to(DEV), pn.g19_tensor("source").to(DEV)
    assert model.head_shape() is None
    with torch.no_grad():
        off = model(template, source, 2)
        model.fused_head = True
        assert not model.uses_fused_head(torch.zeros(2, 64, device=DEV))
        seen = []
        original = count_calls(shw, "pose_head", seen)
        try:
            head_only = model(template, source, 2)
            model.fused_update = True
            both = model(template, source, 2)
        finally:
            shw.pose.pose_head = original
    assert not seen
    assert all(torch.equal(head_only[n], off[n]) for n in off)
    assert all(max_dev(both[n], off[n]) <= 1e-5 for n in off)
