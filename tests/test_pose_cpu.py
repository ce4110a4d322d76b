"""CPU checks of the pose head and the pose update (pose.py, pcrnet.py): the composed functions against the lines of
`PCRNet.Pose_estimation`, the `fused_head` / `fused_update` switches where the composed path is taken, fixture G19 with
the switches on, the packing of the head's parameters, the refusals of the fused ops and the host side of the
shw_pose_* entries.

Every test goes through shw.pose_head*, shw.pose_update*, a PCRNet flag, `packed_head_params` or a shw_pose_* entry:
without the feature each fails on the missing name.
"""
import os
import re

import pytest
import torch

from helpers import pcrnet_cases as pn
from helpers import pose_cases as pc
from helpers.pcrnet_cases import max_dev

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = pc.REFERENCE_WIDTHS
ENTRIES = ("shw_pose_head_supported", "shw_pose_head_param_count", "shw_pose_head_workspace_bytes", "shw_pose_head_forward",
           "shw_pose_head_backward", "shw_pose_update_backward_blocks", "shw_pose_update_workspace_bytes",
           "shw_pose_update_forward", "shw_pose_update_backward")


@pytest.fixture(scope="module")
def shw():
    import shw_amd
    return shw_amd


def todays_lines(shw_module, model, template_features, source_features, source, est_R, est_t):
    """what `Pose_estimation` runs after the trunk with both flags off, operation for operation"""
    batch_size = source.size(0)
    vector = model.linear(torch.cat([template_features, source_features], dim=1))
    pose_7d = shw_module.create_pose_7d(vector)
    identity = torch.eye(3).to(source).view(1, 3, 3).expand(batch_size, 3, 3).contiguous()
    est_R_temp = shw_module.quaternion_rotate(identity, pose_7d).permute(0, 2, 1)
    est_t_temp = shw_module.get_translation(pose_7d).view(-1, 1, 3)
    est_t = torch.bmm(est_R_temp, est_t.permute(0, 2, 1)).permute(0, 2, 1) + est_t_temp
    est_R = torch.bmm(est_R_temp, est_R)
    source = shw_module.quaternion_transform(source, pose_7d)
    return vector, est_R, est_t, source


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_composed_functions_equal_the_modules_lines(shw, dtype):
    model = pn.fill_head(shw.PCRNet(shw.MLP_Architecture(64))).to(dtype)
    g = torch.Generator().manual_seed(11)
    tf, sf = torch.randn(3, 64, generator=g).abs().to(dtype), torch.randn(3, 64, generator=g).abs().to(dtype)
    source, est_R, est_t = (torch.randn(*s, generator=g).to(dtype) for s in ((3, 70, 3), (3, 3, 3), (3, 1, 3)))
    vector, new_R, new_t, moved = todays_lines(shw, model, tf, sf, source, est_R, est_t)
    head = shw.pose_head_composed(tf, sf, model.packed_head_params(), REF)
    assert head.dtype == dtype and torch.equal(head, vector)
    got = shw.pose_update_composed(vector, est_R, est_t, source)
    assert all(torch.equal(a, b) and a.dtype == dtype for a, b in zip(got, (new_R, new_t, moved)))


@pytest.mark.parametrize("k", [1, 3])
def test_flags_on_equal_flags_off_on_the_cpu(shw, k):
    """the CPU takes the composed path: outputs and every gradient bit for bit, also through the keyword arguments"""
    model, template, source, cot, _, f32 = pn.pcrnet_case(shw, k, 36)
    import copy
    switched = copy.deepcopy(model)
    switched.fused_head = switched.fused_update = True
    assert not switched.uses_fused_head(torch.zeros(2, 64)) and switched.head_shape() == (64, REF)
    out, grads = pn.pcrnet_run(shw, switched, template, source, cot, k)
    assert all(torch.equal(out[n], f32[0][n]) for n in f32[0]) and all(torch.equal(grads[n], f32[1][n]) for n in f32[1])
    built = shw.PCRNet(shw.MLP_Architecture(64), 0.0, fused_head=True, fused_update=True)
    assert built.fused_head and built.fused_update
    plain = shw.PCRNet(shw.MLP_Architecture(64))
    assert plain.fused_head is False and plain.fused_update is False


@pytest.mark.parametrize("k", [1, 3])
def test_fixture_g19_with_the_flags_on(shw, k):
    model = pn.g19_model(shw)
    model.fused_head = model.fused_update = True
    template, source = pn.g19_tensor("template").requires_grad_(), pn.g19_tensor("source").requires_grad_()
    out = model(template, source, k)
    (out["transformed_source"] * pn.g19_tensor("cot_source")).sum().backward()
    figures = {name: max_dev(value.detach(), pn.g19_tensor(f"pcrnet.k{k}.{name}")) for name, value in out.items()}
    figures["d/dtemplate"] = max_dev(template.grad, pn.g19_tensor(f"pcrnet.k{k}.grad_template"))
    figures["d/dsource"] = max_dev(source.grad, pn.g19_tensor(f"pcrnet.k{k}.grad_source"))
    figures["d/dtrunk"] = max_dev(torch.cat([p.grad.reshape(-1) for p in model.feature_model.parameters()]),
                                  pn.g19_tensor(f"pcrnet.k{k}.grad_trunk"))
    print(k, {n: f"{v:.2e}" for n, v in figures.items()})
    assert all(v <= 1e-5 for v in figures.values()), figures


def test_packed_head_params_layout_and_gradient(shw):
    model = shw.PCRNet(shw.MLP_Architecture(64))
    packed = model.packed_head_params()
    count = 128 * 1024 + 1024 + 1024 * 1024 + 1024 + 1024 * 512 + 512 + 512 * 512 + 512 + 512 * 256 + 256 + 256 * 7 + 7
    assert packed.shape == (count,) and shw.pose_head_param_count(64) == count
    linears = [model.linear[n] for n in (0, 2, 4, 6, 8, 10)]
    assert torch.equal(packed.detach(), torch.cat([t.detach().reshape(-1) for m in linears for t in (m.weight, m.bias)]))
    for (weight, bias), m in zip(shw.unpack_pose_head_params(packed, 64), linears):
        assert torch.equal(weight, m.weight) and torch.equal(bias, m.bias)
    packed.sum().backward()
    assert all(p.grad is not None and bool((p.grad == 1).all()) for p in model.linear.parameters())
    assert all(p.grad is None for p in model.feature_model.parameters())
    with pytest.raises(ValueError):
        shw.unpack_pose_head_params(packed[:-1], 64)


def test_head_shape_follows_linear(shw):
    assert shw.PCRNet(shw.MLP_Architecture(64)).head_shape() == (64, REF)
    assert shw.PCRNet(shw.MLP_Architecture(64), droput=0.1).head_shape() is None
    edited = shw.PCRNet(shw.MLP_Architecture(64))
    edited.linear[10] = torch.nn.Linear(256, 6)
    assert edited.head_shape() is None
    assert shw.pose_head_supported(64) and shw.pose_head_supported(2048, (32, 2048, 64, 96, 32))
    for emb, widths in ((48, REF), (0, REF), (2080, REF), (64, (1024, 1024, 512, 512, 250)), (64, (1024, 1024, 512, 512))):
        assert not shw.pose_head_supported(emb, widths)


def test_fused_ops_refuse_host_tensors_wrong_dtypes_and_bad_shapes(shw):
    tf, params = torch.zeros(2, 64), torch.zeros(shw.pose_head_param_count(64))
    update = (torch.zeros(2, 7), torch.zeros(2, 3, 3), torch.zeros(2, 1, 3), torch.zeros(2, 5, 3))
    with pytest.raises(RuntimeError):
        shw.pose_head(tf, tf, params)
    with pytest.raises(RuntimeError):
        shw.pose_update(*update)
    with pytest.raises(TypeError):
        shw.pose_head(tf.double(), tf.double(), params.double())
    with pytest.raises(TypeError):
        shw.pose_update(*(t.double() for t in update))
    with pytest.raises(TypeError):
        shw.pose_update(update[0].numpy(), *update[1:])
    # shapes and widths are judged before the device: host tensors outside the envelope get the ValueError
    zeros = torch.zeros
    for bad in ((zeros(2, 48), zeros(2, 48), zeros(shw.pose_head_param_count(48)), REF),
                (zeros(2, 64), zeros(3, 64), params, REF),
                (zeros(64), zeros(64), params, REF),
                (tf, tf, params[:-1], REF),
                (tf, tf, zeros(shw.pose_head_param_count(64, (40, 32, 32, 32, 32))), (40, 32, 32, 32, 32)),
                (tf, tf, zeros(shw.pose_head_param_count(64, (4096, 32, 32, 32, 32))), (4096, 32, 32, 32, 32)),
                (tf, tf, zeros(10), (32, 32, 32, 32))):
        with pytest.raises(ValueError):
            shw.pose_head(*bad)
    for bad in ((zeros(2, 6), update[1], update[2], update[3]), (update[0], zeros(2, 3, 4), update[2], update[3]),
                (update[0], update[1], zeros(2, 3), update[3]), (update[0], update[1], update[2], zeros(2, 5, 2)),
                (update[0], update[1], update[2], zeros(2, 0, 3)), (update[0], update[1], update[2], zeros(3, 5, 3))):
        with pytest.raises(ValueError):
            shw.pose_update(*bad)
    with pytest.raises(ValueError):
        shw.pose_head_composed(tf, tf, params[:-1])


def test_envelope_entries_through_ctypes(shw):
    lib = shw._lib.load()
    for emb, widths in ((64, REF), (1024, REF), (32, pc.ALL_32), (2048, (2048, 32, 96, 64, 32))):
        assert lib.shw_pose_head_supported(emb, *widths) == 1 and shw.pose_head_supported(emb, widths)
        assert lib.shw_pose_head_param_count(emb, *widths) == shw.pose_head_param_count(emb, widths)
        for clouds in (1, 32, 33):
            padded = (clouds + 31) // 32 * 32
            assert lib.shw_pose_head_workspace_bytes(clouds, emb, *widths, 2) == 4 * padded * sum(widths)
            for which in (0, 1):
                assert lib.shw_pose_head_workspace_bytes(clouds, emb, *widths, which) >= 2 * 4 * padded * max(widths[:4])
    assert lib.shw_pose_head_workspace_bytes(32, 1024, *REF, 2) == 4 * 32 * 3328
    for emb, widths in ((48, REF), (31, REF), (2080, REF), (0, REF), (-32, REF), (64, (1024, 1024, 512, 512, 250)),
                        (64, (4096, 1024, 512, 512, 256))):
        assert lib.shw_pose_head_supported(emb, *widths) == 0 and not shw.pose_head_supported(emb, widths)
        assert lib.shw_pose_head_param_count(emb, *widths) == 0
        assert all(lib.shw_pose_head_workspace_bytes(4, emb, *widths, which) == 0 for which in (0, 1, 2))
    assert lib.shw_pose_head_workspace_bytes(0, 64, *REF, 0) == 0 and lib.shw_pose_head_workspace_bytes(4, 64, *REF, 3) == 0
    assert [lib.shw_pose_update_backward_blocks(n) for n in (-1, 0, 1, 256, 257, 64 * 256, 64 * 256 + 1, 10 ** 9)] == \
        [0, 0, 1, 1, 2, 64, 64, 64]
    assert lib.shw_pose_update_workspace_bytes(3, 257) == 3 * 2 * 12 * 4
    assert lib.shw_pose_update_workspace_bytes(0, 257) == 0 and lib.shw_pose_update_workspace_bytes(3, 0) == 0


def test_argument_checks_need_no_gpu(shw):
    """arguments outside the limits return hipErrorInvalidValue (1) before any HIP call"""
    lib = shw._lib.load()
    assert lib.shw_pose_head_forward(None, None, None, 1, 48, *REF, None, None, None, None) == 1
    assert lib.shw_pose_head_forward(None, None, None, 1, 64, *REF, None, None, None, None) == 1      # null pointers
    assert lib.shw_pose_head_backward(None, None, None, None, None, 0, 64, *REF, None, None, None, None, None) == 1
    assert lib.shw_pose_head_backward(None, None, None, None, None, 1, 64, 1024, 1024, 512, 512, 250, None, None, None, None,
                                      None) == 1
    assert lib.shw_pose_update_forward(None, None, None, None, 1, 1, None, None, None, None) == 1
    one = torch.zeros(64)
    p = one.data_ptr()
    assert lib.shw_pose_update_forward(p, p, p, p, 65536, 1, p, p, p, None) == 1                     # B rides on gridDim.y
    assert lib.shw_pose_update_forward(p, p, p, p, 1, 0, p, p, p, None) == 1
    assert lib.shw_pose_update_forward(p, p, p, p, 1, 2 ** 31, p, p, p, None) == 1
    assert lib.shw_pose_update_backward(p, p, p, p, None, None, p, 65536, 1, p, None, None, None, p, None) == 1
    assert lib.shw_pose_update_backward(p, p, p, p, None, None, p, 1, 1, p, None, None, None, None, None) == 1   # no workspace
    assert lib.shw_pose_update_backward(None, None, None, None, None, None, None, 1, 1, None, None, None, None, None,
                                        None) == 1


def test_header_declares_the_entries_and_keeps_the_abi_version(shw):
    text = open(os.path.join(ROOT, "include", "shw.h")).read()
    for name in ENTRIES:
        assert re.search(rf"SHW_API\s+\w+\s+{name}\(", text), name
        assert name in shw._lib.EXPORTED_SYMBOLS
    assert re.search(r"#define SHW_ABI_VERSION 3\b", text) and shw._lib.ABI_VERSION == 3
