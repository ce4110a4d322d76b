"""tools/make_golden_pcrnet.py -- fixture G19 (tests/golden/g19_pcrnet.npz): the reference's registration network, captured
from the REAL reference on the CPU (it needs a checkout of it; the tests need only the fixture).

The reference's `models` package imports `data_utils.Data_set_transformation`, which imports torch_geometric at module
level (the dataset code; the pose helpers the network uses need only torch).  torch_geometric is not installed, so empty
stand-in modules take its place and the reference's files are loaded by path behind stand-in packages.

Stored: the state-dict names and shapes of `PCRNet(MLP_Architecture(64))` without and with dropout; the trunk's weights
(emb_dims = 64, as constructed under torch.manual_seed(19 + seed)); for the inputs `x270` (2, 70, 3) and `x11` (1, 1, 3)
with cotangents `c270`, `c11`: `Pooling()(MLP_Architecture(64)(x))` and the gradients of sum(out * c) w.r.t. x and every trunk
tensor; for `template`, `source` (2, 70, 3) and iteration_num 1 and 3: the five outputs of PCRNet and the gradients of
sum(transformed_source * cot) w.r.t. template, source and the trunk; and the pose helpers on three poses.  The head's 2.1 M
weights are not stored: tests/helpers/pcrnet_cases.py `fill_head` writes them, here and in the tests.  The seed is the
first for which every trunk call of the fixture meets the tests' margin condition (pcrnet_cases, module docstring).

    python tools/make_golden_pcrnet.py --reference <reference checkout>
"""
import argparse
import importlib.util
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
OUT = os.path.join(ROOT, "tests", "golden", "g19_pcrnet.npz")
LIMIT = 563 * 1024            # the largest fixture committed so far


def load_reference(checkout):
    """the reference's models.{MLP_Architecture, Pooling, PCRNet} and Dataset_Transformation, by path"""
    base = os.path.join(checkout, "Point_Cloud_Resistration")
    if not os.path.isdir(base):
        base = checkout
    for name, attrs in (("torch_geometric", ()), ("torch_geometric.datasets", ("ModelNet",)),
                        ("torch_geometric.transforms", ()), ("torch_geometric.data", ("Data",)),
                        ("torch_geometric.utils", ("to_networkx",))):
        stub = types.ModuleType(name)
        for attr in attrs:
            setattr(stub, attr, None)
        stub.__path__ = []
        sys.modules[name] = stub
    for name, sub in (("data_utils", "data_utils"), ("models", "models")):
        pkg = types.ModuleType(name)
        pkg.__path__ = [os.path.join(base, sub)]
        sys.modules[name] = pkg
    mods = {}
    for name, rel in (("data_utils.Data_set_transformation", "data_utils/Data_set_transformation.py"),
                      ("models.mlp_architecture", "models/mlp_architecture.py"), ("models.pooling", "models/pooling.py"),
                      ("models.pcrnet", "models/pcrnet.py")):
        spec = importlib.util.spec_from_file_location(name, os.path.join(base, rel))
        mod = importlib.util.module_from_spec(spec)
        sys.modules[name] = mod
        spec.loader.exec_module(mod)
        mods[name.rsplit(".", 1)[1]] = mod
    return mods


def flat(tensors):
    return np.concatenate([t.detach().numpy().reshape(-1) for t in tensors])


def capture(ref, seed):
    import shw_amd as shw
    from helpers import pcrnet_cases as pc

    MLP, Pool, Net = ref["mlp_architecture"].MLP_Architecture, ref["pooling"].Pooling, ref["pcrnet"].PCRNet
    tf = ref["Data_set_transformation"]
    T = tf.Dataset_Transformation
    out = {}
    for key, dropout in (("pcrnet.state", 0.0), ("pcrnet.state_dropout", 0.3)):
        state = Net(MLP(64), droput=dropout).state_dict()
        out[f"{key}_names"] = np.array(list(state))
        out[f"{key}_shapes"] = np.array(["x".join(map(str, t.shape)) for t in state.values()])
    torch.manual_seed(19 + seed)
    trunk = MLP(64)
    names = [n for n, _ in trunk.named_parameters()]
    out["trunk.names"] = np.array(names)
    for n, p in trunk.named_parameters():
        out[f"trunk.{n}"] = p.detach().numpy().copy()
    g = torch.Generator().manual_seed(1900 + seed)
    data = {"x270": torch.randn(2, 70, 3, generator=g), "x11": torch.randn(1, 1, 3, generator=g),
            "c270": torch.randn(2, 64, generator=g), "c11": torch.randn(1, 64, generator=g),
            "template": torch.randn(2, 70, 3, generator=g), "source": torch.randn(2, 70, 3, generator=g),
            "cot_source": torch.randn(2, 70, 3, generator=g)}
    out.update({k: v.numpy() for k, v in data.items()})
    # this package's trunk with the same weights: the margin condition is checked through it
    mine = shw.PCRNet(shw.MLP_Architecture(64))
    mine.feature_model.load_state_dict(trunk.state_dict(), strict=True)
    pc.fill_head(mine)
    packed = mine.feature_model.packed_params().detach()
    for xk, ck in (("x270", "c270"), ("x11", "c11")):
        pc.assert_margin(data[xk], packed, 64, shw, xk)
        trunk.zero_grad()
        x = data[xk].clone().requires_grad_()
        y = Pool()(trunk(x))
        (y * data[ck]).sum().backward()
        out[f"{xk}.pooled"] = y.detach().numpy()
        out[f"{xk}.grad_x"] = x.grad.numpy()
        out[f"{xk}.grad_trunk"] = flat([p.grad for p in trunk.parameters()])
    net = pc.fill_head(Net(trunk))
    for k in (1, 3):
        pc.run_pcrnet_checked(shw, mine.double(), data["template"].double(), data["source"].double(), k)
        net.zero_grad()
        template, source = data["template"].clone().requires_grad_(), data["source"].clone().requires_grad_()
        res = net(template, source, k)
        (res["transformed_source"] * data["cot_source"]).sum().backward()
        for name, value in res.items():
            out[f"pcrnet.k{k}.{name}"] = value.detach().numpy()
        out[f"pcrnet.k{k}.grad_template"] = template.grad.numpy()
        out[f"pcrnet.k{k}.grad_source"] = source.grad.numpy()
        out[f"pcrnet.k{k}.grad_trunk"] = flat([p.grad for p in trunk.parameters()])
    # the pose helpers: raw 7-vectors (one with a large and one with a tiny quaternion part), points of both ranks
    raw = torch.randn(3, 7, generator=g) * torch.tensor([[1.0], [40.0], [1e-3]])
    pts3, pts2 = torch.randn(3, 5, 3, generator=g), torch.randn(6, 3, generator=g)
    pose = T.create_pose_7d(raw)
    out.update({"pose.raw": raw.numpy(), "pose.points3": pts3.numpy(), "pose.points2": pts2.numpy(),
                "pose.create_pose_7d": pose.numpy(),
                "pose.qrot": tf.qrot(pose[:, None, :4].expand(3, 5, 4).contiguous(), pts3).numpy(),
                "pose.quaternion_rotate3": T.quaternion_rotate(pts3, pose).numpy(),
                "pose.quaternion_rotate2": T.quaternion_rotate(pts2, pose[1:2]).numpy(),
                "pose.quaternion_transform": T.quaternion_transform(pts3, pose).numpy(),
                "pose.get_translation": T.get_translation(pose).numpy(),
                "pose.convert2transformation": T.convert2transformation(
                    T.quaternion_rotate(torch.eye(3).expand(3, 3, 3).contiguous(), pose), pose[:, None, 4:]).numpy()})
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="a checkout of the reference (the directory that holds "
                                                       "Point_Cloud_Resistration, or that directory itself)")
    args = ap.parse_args()
    ref = load_reference(args.reference)
    for seed in range(200):
        try:
            out = capture(ref, seed)
        except AssertionError as err:                # the margin condition: try the next seed
            print("seed", seed, "rejected:", str(err)[:120])
            continue
        break
    else:
        raise SystemExit("no seed meets the margin condition")
    out["seed"] = np.array(seed)
    np.savez_compressed(OUT, **out)
    size = os.path.getsize(OUT)
    assert size <= LIMIT, size
    print("seed", seed, "wrote", OUT, size, "bytes")


if __name__ == "__main__":
    main()
