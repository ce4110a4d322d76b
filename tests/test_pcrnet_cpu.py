"""CPU checks of the registration network (pcrnet.py): the composed trunk, the pose helpers and PCRNet against fixture
G19, which holds what the reference's own modules compute (tools/make_golden_pcrnet.py), the state-dict contract, the
packing of the parameters the kernels read, and the host side of the shw_pointnet_* entries.

Every test goes through shw.PCRNet, shw.MLP_Architecture, shw.pointnet_max_features_composed, a pose helper or a
shw_pointnet_* entry: without the feature each fails on the missing name.

Float32 against the reference's float32, bound 1e-5 on max |error| / max |reference entry| per tensor.  Measured here:
trunk values 3.1e-7 (linear layers against the reference's 1x1 convolutions), d/dx 0, trunk gradients 8.0e-8; PCRNet outputs
at most 3.5e-6 (`r`, a difference of features, k = 3; the others 6.8e-7) and gradients at most 8.5e-7; helpers 0.
"""
import os
import re

import numpy as np
import pytest
import torch

from helpers import pcrnet_cases as pc
from helpers.pcrnet_cases import max_dev

BOUND = 1e-5
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def shw():
    import shw_amd
    return shw_amd


def shapes_of(key):
    g = pc.g19()
    return {str(n): (tuple(int(v) for v in str(s).split("x")) if str(s) else ())
            for n, s in zip(g[f"{key}_names"], g[f"{key}_shapes"])}


@pytest.mark.parametrize("key,dropout", [("pcrnet.state", 0.0), ("pcrnet.state_dropout", 0.3)])
def test_state_dict_names_and_shapes_are_the_references(shw, key, dropout):
    model = shw.PCRNet(shw.MLP_Architecture(64), droput=dropout)
    state = model.state_dict()
    assert list(state) == [str(n) for n in pc.g19()[f"{key}_names"]]
    assert {n: tuple(t.shape) for n, t in state.items()} == shapes_of(key)
    last = "linear.11" if dropout else "linear.10"
    assert f"{last}.weight" in state and tuple(state[f"{last}.weight"].shape) == (7, 256)
    # a dict keyed by the reference's list loads strictly, and the values arrive
    g = torch.Generator().manual_seed(3)
    fresh = {n: torch.randn(s, generator=g) for n, s in shapes_of(key).items()}
    other = shw.PCRNet(shw.MLP_Architecture(64), droput=dropout)
    other.load_state_dict(fresh, strict=True)
    assert all(torch.equal(t, fresh[n]) for n, t in other.state_dict().items())


def test_default_construction(shw):
    """emb_dims = 1024 by default, Conv1d shapes, and every model built without a feature model gets its own trunk"""
    a, b = shw.PCRNet(), shw.PCRNet()
    assert a.feature_model is not b.feature_model
    assert a.feature_model.emb_dims == 1024 and tuple(a.feature_model.conv5.weight.shape) == (1024, 128, 1)
    assert a.linear[0].in_features == 2048
    assert tuple(shw.MLP_Architecture(64)(torch.zeros(2, 5, 3)).shape) == (2, 64, 5)


def test_packed_params_order(shw):
    trunk = shw.MLP_Architecture(64)
    packed = trunk.packed_params()
    assert packed.shape == (shw.pointnet_param_count(64),) and shw.pointnet_param_count(64) == 16896 + 129 * 64
    expected = torch.cat([t.detach().reshape(-1) for n in range(1, 6)
                          for t in (getattr(trunk, f"conv{n}").weight, getattr(trunk, f"conv{n}").bias)])
    assert torch.equal(packed.detach(), expected)
    for (weight, bias), n in zip(shw.unpack_pointnet_params(packed, 64), range(1, 6)):
        conv = getattr(trunk, f"conv{n}")
        assert torch.equal(weight, conv.weight[:, :, 0]) and torch.equal(bias, conv.bias)
    packed.sum().backward()
    assert all(p.grad is not None and bool((p.grad == 1).all()) for p in trunk.parameters())


@pytest.mark.parametrize("xk,ck", [("x270", "c270"), ("x11", "c11")])
def test_composed_trunk_matches_the_fixture(shw, xk, ck):
    trunk = shw.MLP_Architecture(64)
    trunk.load_state_dict(pc.g19_trunk_state(), strict=True)
    x = pc.g19_tensor(xk).requires_grad_()
    y = trunk.pooled(x)
    assert y.shape == (x.shape[0], 64) and y.dtype == torch.float32
    assert max_dev(y.detach(), shw.Pooling()(trunk(x)).detach()) <= 1e-6       # linear layers against 1x1 convolutions
    (y * pc.g19_tensor(ck)).sum().backward()
    figures = {"value": max_dev(y.detach(), pc.g19_tensor(f"{xk}.pooled")),
               "d/dx": max_dev(x.grad, pc.g19_tensor(f"{xk}.grad_x")),
               "d/dtrunk": max_dev(torch.cat([p.grad.reshape(-1) for p in trunk.parameters()]),
                                   pc.g19_tensor(f"{xk}.grad_trunk"))}
    print(xk, {k: f"{v:.2e}" for k, v in figures.items()})
    assert all(v <= BOUND for v in figures.values()), figures


@pytest.mark.parametrize("k", [1, 3])
def test_pcrnet_matches_the_fixture(shw, k):
    model = pc.g19_model(shw)
    template, source = pc.g19_tensor("template").requires_grad_(), pc.g19_tensor("source").requires_grad_()
    out = model(template, source, k)
    assert sorted(out) == ["est_R", "est_T", "est_t", "r", "transformed_source"]
    (out["transformed_source"] * pc.g19_tensor("cot_source")).sum().backward()
    figures = {name: max_dev(value.detach(), pc.g19_tensor(f"pcrnet.k{k}.{name}")) for name, value in out.items()}
    figures["d/dtemplate"] = max_dev(template.grad, pc.g19_tensor(f"pcrnet.k{k}.grad_template"))
    figures["d/dsource"] = max_dev(source.grad, pc.g19_tensor(f"pcrnet.k{k}.grad_source"))
    figures["d/dtrunk"] = max_dev(torch.cat([p.grad.reshape(-1) for p in model.feature_model.parameters()]),
                                  pc.g19_tensor(f"pcrnet.k{k}.grad_trunk"))
    print(k, {n: f"{v:.2e}" for n, v in figures.items()})
    assert all(v <= BOUND for v in figures.values()), figures


def test_pose_helpers_match_the_fixture(shw):
    raw, pts3, pts2 = pc.g19_tensor("pose.raw"), pc.g19_tensor("pose.points3"), pc.g19_tensor("pose.points2")
    pose = shw.create_pose_7d(raw)
    rotated_identity = shw.quaternion_rotate(torch.eye(3).expand(3, 3, 3).contiguous(), pose)
    got = {"create_pose_7d": pose, "qrot": shw.qrot(pose[:, None, :4].expand(3, 5, 4).contiguous(), pts3),
           "quaternion_rotate3": shw.quaternion_rotate(pts3, pose),
           "quaternion_rotate2": shw.quaternion_rotate(pts2, pose[1:2]),
           "quaternion_transform": shw.quaternion_transform(pts3, pose),
           "get_translation": shw.get_translation(pose),
           "convert2transformation": shw.convert2transformation(rotated_identity, pose[:, None, 4:])}
    figures = {name: max_dev(value, pc.g19_tensor(f"pose.{name}")) for name, value in got.items()}
    print({n: f"{v:.2e}" for n, v in figures.items()})
    assert all(v <= BOUND for v in figures.values()), figures
    assert torch.allclose(pose[:, :4].norm(dim=1), torch.ones(3), atol=1e-6)


def test_head_fill_is_exact_in_float32():
    values = pc.lcg_integers(3 * 4096 + 5, 7)
    slow, s = [], 7
    for _ in range(4096 + 3):
        s = (1664525 * s + 1013904223) & 0xFFFFFFFF
        slow.append((s >> 24) - 128)
    assert values[:4096 + 3].tolist() == slow and values.min() >= -128 and values.max() <= 127


def test_envelope_entries_through_ctypes(shw):
    lib = shw._lib.load()
    for emb in (32, 64, 96, 1024, 2048):
        assert lib.shw_pointnet_supported(3, emb) == 1 and shw.pointnet_supported(3, emb)
        assert lib.shw_pointnet_param_count(emb) == shw.pointnet_param_count(emb) == 16896 + 129 * emb
        tiles = (70 + pc.POINT_TILE - 1) // pc.POINT_TILE
        assert lib.shw_pointnet_workspace_bytes(3, 70, emb, 0) == 3 * tiles * emb * 8
        assert lib.shw_pointnet_workspace_bytes(3, 70, emb, 1) >= 4 * (3 * emb * 3 + 16896 + emb * 129)
    for dim, emb in ((3, 31), (3, 48), (3, 2080), (2, 64), (3, 0), (3, -32)):
        assert lib.shw_pointnet_supported(dim, emb) == 0 and not shw.pointnet_supported(dim, emb)
    for emb in (31, 48, 2080):
        assert lib.shw_pointnet_param_count(emb) == 0
        assert lib.shw_pointnet_workspace_bytes(3, 70, emb, 0) == 0 and lib.shw_pointnet_workspace_bytes(3, 70, emb, 1) == 0
    assert lib.shw_pointnet_workspace_bytes(0, 70, 64, 0) == 0 and lib.shw_pointnet_workspace_bytes(3, 0, 64, 1) == 0
    # outside the envelope the entries refuse before any HIP call (no device is needed to be told so)
    assert lib.shw_pointnet_forward(None, None, 1, 1, 48, None, None, None, None) == 1
    assert lib.shw_pointnet_backward(None, None, None, None, None, 1, 0, 64, None, None, None, None) == 1


def test_header_declares_the_entries_and_keeps_the_abi_version(shw):
    text = open(os.path.join(ROOT, "include", "shw.h")).read()
    for name in ("shw_pointnet_supported", "shw_pointnet_param_count", "shw_pointnet_workspace_bytes",
                 "shw_pointnet_forward", "shw_pointnet_backward"):
        assert re.search(rf"SHW_API\s+\w+\s+{name}\(", text), name
        assert name in shw._lib.EXPORTED_SYMBOLS
    assert re.search(r"#define SHW_ABI_VERSION 3\b", text) and shw._lib.ABI_VERSION == 3


def test_fused_op_refuses_host_tensors_and_bad_shapes(shw):
    params = torch.zeros(shw.pointnet_param_count(64))
    with pytest.raises(RuntimeError):
        shw.pointnet_max_features(torch.zeros(1, 4, 3), params, 64)
    with pytest.raises(ValueError):
        shw.pointnet_max_features_composed(torch.zeros(1, 4, 3), params[:-1], 64)
    # the module falls back to the composed path on the CPU, in float64 and outside the envelope
    for emb, dtype in ((64, torch.float64), (48, torch.float32)):
        trunk = shw.MLP_Architecture(emb).to(dtype)
        x = torch.randn(2, 9, 3, dtype=dtype)
        assert max_dev(trunk.pooled(x).detach(), trunk(x).max(dim=2)[0].detach()) <= 1e-6
