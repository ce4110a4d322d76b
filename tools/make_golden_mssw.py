"""tools/make_golden_mssw.py -- fixture G21 (tests/golden/g21_mssw.npz): the sphere encoder and the wrapper of the
reference's mini_batch_Residual_MSSW.py, captured from the REAL file (it needs a checkout of the reference; the tests need
only the fixture).  Arrays and names only.

The file imports `losses.normflows_ishikawa`, whose package __init__ pulls in a module that is not installed.  The seven
files it needs of that package -- flows/base.py, planar.py, residual.py, reshape.py, affine/coupling.py, normalization.py
and nets/lipschitz.py -- need only torch and numpy: they are loaded by file path behind empty stand-in packages (as
tools/make_golden_flows.py does), a stand-in `losses.normflows_ishikawa` offers `flows.{Planar, Residual, ActNorm}` and
`nets.LipschitzMLP`, and mini_batch_Residual_MSSW.py itself is then imported by path (it imports matplotlib:
MPLBACKEND=Agg).

(a) The module.  Cases `res2` ("Residual", n_flow_layer=2, the smoke program's), `res3` (the default 3), `planar3`, each
    built after torch.manual_seed(0).  Variant `init`: as constructed.  Variant `pert` (Residual only): the i-ResNet
    weights moved so that the blocks are no longer the identity they start as -- the last layer's / 1000 undone, the
    weights scaled by 2 and 0.6 in turn, every beta shifted -- and both branches of max(1, sigma / 0.9) are asserted to
    occur.  Per case and variant: `state_names`, `param_names`, and per dtype (`f32`, `f64`: the module converted with
    .to) the state before the first forward (`state0_shapes`, `state0`) and after it (`state1_shapes`, `state1`), values
    as one float64 vector; on the input `a.x` (5, 70, 3) with the cotangent `a.cot`, the output of the second forward in
    train mode and of a third in eval mode (`out_train`, `out_eval`), d/dx (`grad_x`) and every parameter gradient
    (`grad_names`, `grad_values`).
(b) The wrapper.  The real max_spherical_wassersten_distance_Residual with the real encoder (case res2, variant pert,
    initialised by one call on `b.first` as the smoke program does), SSW the reference's own sliced_cost on the fixed
    frames `b.U`, B=6, N=40, L=16, max_iter=3, psi_minibatch_size=2, Adam(lr=0.01, betas=(0.5, 0.999)), numpy and torch
    seeded, modes train and test, in float32 and float64: `ssw`, the printed `trace`, the minibatch `indices` drawn,
    `phi_first`, `phi_second`, every parameter after the call (`params`, in parameters() order), `g_first`, `g_second`.
    Asserted before writing: between the float32 and the float64 run at most 0.5 % of the entries of an input gradient
    differ by more than 2e-3 of its largest entry (else: try another --seed).

    python tools/make_golden_mssw.py --reference <reference checkout>/Point_Cloud_Resistration/losses
"""
import argparse
import contextlib
import copy
import importlib.util
import io
import os
import sys
import types

os.environ.setdefault("MPLBACKEND", "Agg")

import numpy as np  # noqa: E402
import torch  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden", "g21_mssw.npz")
CASES = {"res2": ("Residual", 2), "res3": ("Residual", 3), "planar3": ("Planar", 3)}
DTYPES = (("f32", torch.float32), ("f64", torch.float64))
B, N, L, ITERS, MINI, LR, BETAS = 6, 40, 16, 3, 2, 0.01, (0.5, 0.999)
COEFF = 0.9


def load_by_path(name, path):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    sys.modules[name] = mod
    spec.loader.exec_module(mod)
    return mod


def load_reference(losses_dir):
    """mini_batch_Residual_MSSW.py behind the stand-in packages"""
    pkg_dir = os.path.join(losses_dir, "normflows_ishikawa")
    for name, sub in (("nf_ref", ""), ("nf_ref.flows", "flows"), ("nf_ref.flows.affine", "flows/affine"),
                      ("nf_ref.nets", "nets")):
        pkg = types.ModuleType(name)
        pkg.__path__ = [os.path.join(pkg_dir, sub)]
        sys.modules[name] = pkg
    mods = {}
    for name, rel in (("nf_ref.flows.base", "flows/base.py"), ("nf_ref.flows.planar", "flows/planar.py"),
                      ("nf_ref.flows.residual", "flows/residual.py"), ("nf_ref.flows.reshape", "flows/reshape.py"),
                      ("nf_ref.flows.affine.coupling", "flows/affine/coupling.py"),
                      ("nf_ref.flows.normalization", "flows/normalization.py"),
                      ("nf_ref.nets.lipschitz", "nets/lipschitz.py")):
        mods[name.rsplit(".", 1)[1]] = load_by_path(name, os.path.join(pkg_dir, rel))
    nf = types.ModuleType("losses.normflows_ishikawa")
    nf.flows = types.SimpleNamespace(Planar=mods["planar"].Planar, Residual=mods["residual"].Residual,
                                     ActNorm=mods["normalization"].ActNorm)
    nf.nets = types.SimpleNamespace(LipschitzMLP=mods["lipschitz"].LipschitzMLP)
    losses = types.ModuleType("losses")
    losses.__path__ = []
    losses.normflows_ishikawa = nf
    sys.modules["losses"], sys.modules["losses.normflows_ishikawa"] = losses, nf
    return load_by_path("ref_mssw", os.path.join(losses_dir, "mini_batch_Residual_MSSW.py"))


def npy(t):
    return t.detach().cpu().numpy()


def flat64(tensors):
    return np.concatenate([npy(t).astype(np.float64).reshape(-1) for t in tensors] + [np.zeros(0)])


def shapes_of(tensors):
    return np.array(["x".join(map(str, t.shape)) for t in tensors])


def perturbed(state):
    """the i-ResNet weights moved away from the identity (module docstring)"""
    out, turn = {}, 0
    for k, v in state.items():
        v = v.clone()
        if ".iresblock.nnet.net." in k and k.endswith(".weight"):
            if k.endswith("net.3.weight"):
                v *= 1000.0                                   # the last layer starts at 1/1000 scale
            v *= 2.0 if turn % 2 == 0 else 0.6
            turn += 1
        elif k.endswith(".beta"):
            v += 0.3 if turn % 2 else -0.2
        out[k] = v
    return out


def module_cases(ref, out):
    g = torch.Generator().manual_seed(21)
    x, cot = torch.randn(5, 70, 3, generator=g), torch.randn(5, 70, 3, generator=g)
    out["a.x"], out["a.cot"] = npy(x), npy(cot)
    kept = {}
    for case, (flow_name, n_flow_layer) in CASES.items():
        torch.manual_seed(0)
        np.random.seed(0)
        built = copy.deepcopy(ref.transform_to_sphere(flow_name=flow_name, n_flow_layer=n_flow_layer).state_dict())
        variants = {"init": built}
        if flow_name == "Residual":
            variants["pert"] = perturbed(built)
        for var, state0 in variants.items():
            key = f"a.{case}.{var}."
            scales = []
            for dname, dtype in DTYPES:
                phi = ref.transform_to_sphere(flow_name=flow_name, n_flow_layer=n_flow_layer)
                phi.load_state_dict(state0, strict=True)
                phi = phi.to(dtype)
                out[key + "state_names"] = np.array(list(phi.state_dict()))
                out[key + "param_names"] = np.array([n for n, _ in phi.named_parameters()])
                before = copy.deepcopy(phi.state_dict())
                xd, cd = x.to(dtype), cot.to(dtype)
                phi.train()
                phi(xd.clone())                                # the first forward: data-dependent initialisation
                after = copy.deepcopy(phi.state_dict())
                assert list(after) == list(before)
                out[key + dname + ".state0_shapes"], out[key + dname + ".state0"] = shapes_of(before.values()), flat64(before.values())
                out[key + dname + ".state1_shapes"], out[key + dname + ".state1"] = shapes_of(after.values()), flat64(after.values())
                phi.zero_grad()
                xs = xd.clone().requires_grad_()
                y = phi(xs)
                (y * cd).sum().backward()
                phi.eval()
                with torch.no_grad():
                    out[key + dname + ".out_eval"] = npy(phi(xd.clone()))
                out[key + dname + ".out_train"], out[key + dname + ".grad_x"] = npy(y), npy(xs.grad)
                with_grad = [(n, p.grad) for n, p in phi.named_parameters() if p.grad is not None]
                out[key + dname + ".grad_names"] = np.array([n for n, _ in with_grad])
                out[key + dname + ".grad_values"] = np.concatenate([npy(t).reshape(-1) for _, t in with_grad])
                scales += [float(v) for k, v in phi.state_dict().items() if k.endswith(".scale")]
                print(f"(a) {case} {var} {dname}: train == eval:",
                      np.array_equal(out[key + dname + ".out_train"], out[key + dname + ".out_eval"]),
                      "parameters with a gradient:", len(with_grad), "of", len(out[key + "param_names"]))
            if var == "pert":
                assert any(s > COEFF for s in scales) and any(s < COEFF for s in scales), scales
            kept[(case, var)] = state0
    return kept[("res2", "pert")]


def wrapper_runs(ref, state0, out, seed):
    g = torch.Generator().manual_seed(seed)
    first = torch.randn(B, N, 3, generator=g)
    second = 0.6 * torch.randn(B, N, 3, generator=g) + torch.tensor([1.0, -0.7, 0.4])     # clearly another cloud
    U = torch.linalg.qr(torch.randn(L, 3, 2, generator=g))[0]
    out.update({"b.first": npy(first), "b.second": npy(second), "b.U": npy(U), "b.seed": np.int64(seed),
                "b.config": np.array([B, N, L, ITERS, MINI]), "b.lr": np.float64(LR), "b.betas": np.array(BETAS)})
    for dname, dtype in DTYPES:
        def ssw_pair(a, b, num_projections, device, p=2):
            return ref.sliced_cost(a, b, U.to(dtype), p=p)

        for mode in ("train", "test"):
            torch.manual_seed(seed)
            np.random.seed(seed)
            phi = ref.transform_to_sphere(flow_name="Residual", n_flow_layer=2)
            phi.load_state_dict(state0, strict=True)
            phi = phi.to(dtype)
            phi(first.to(dtype))                               # initialises, as the smoke program's psi(init_inputs1)
            opt = torch.optim.Adam(phi.parameters(), lr=LR, betas=BETAS)
            crit = ref.max_spherical_wassersten_distance_Residual(L, phi=phi, SSW=ssw_pair, phi_op=opt, p=2, max_iter=ITERS,
                                                                  psi_minibatch_size=MINI, device="cpu")
            a, b = first.to(dtype).clone().requires_grad_(), second.to(dtype).clone().requires_grad_()
            drawn, choice = [], np.random.choice

            def recording_choice(*args, **kwargs):
                drawn.append(choice(*args, **kwargs))
                return drawn[-1]

            buf = io.StringIO()
            np.random.choice = recording_choice
            try:
                with contextlib.redirect_stdout(buf):          # the wrapper prints ssw.item() per inner iteration
                    ssw, fa, fb = crit(a, b, train_or_test=mode)
            finally:
                np.random.choice = choice
            opt.zero_grad()
            ssw.sum().backward()
            key = f"b.{dname}.{mode}."
            out[key + "ssw"] = npy(ssw).reshape(-1)
            out[key + "trace"] = np.array([float(t) for t in buf.getvalue().split()], dtype=np.float64)
            out[key + "indices"] = np.array(drawn, dtype=np.int64).reshape(-1, MINI)
            out[key + "param_names"] = np.array([n for n, _ in phi.named_parameters()])
            out[key + "params"] = flat64([p for p in phi.parameters()])
            out[key + "phi_first"], out[key + "phi_second"] = npy(fa), npy(fb)
            out[key + "g_first"], out[key + "g_second"] = npy(a.grad), npy(b.grad)
            assert len(out[key + "trace"]) == len(drawn) == (ITERS if mode == "train" else 0)


def gaps(out):
    """the reference's own float32-versus-float64 differences per mode; returns the largest share of gradient entries over
    2e-3 of the largest entry"""
    worst = 0.0
    for mode in ("train", "test"):
        k32, k64 = f"b.f32.{mode}.", f"b.f64.{mode}."
        fig = {"ssw": float(np.max(np.abs(out[k32 + "ssw"] - out[k64 + "ssw"]) / np.abs(out[k64 + "ssw"])))}
        if len(out[k64 + "trace"]):
            fig["trace"] = float(np.max(np.abs(out[k32 + "trace"] - out[k64 + "trace"]) / np.abs(out[k64 + "trace"])))
        fig["params"] = float(np.abs(out[k32 + "params"] - out[k64 + "params"]).max())
        fig["maps"] = max(float(np.abs(out[k32 + n] - out[k64 + n]).max()) for n in ("phi_first", "phi_second"))
        for name in ("g_first", "g_second"):
            want = out[k64 + name]
            scale, err = np.abs(want).max(), np.abs(out[k32 + name] - want)
            fig[name + " max"] = float(err.max() / scale)
            fig[name + " share"] = float((err > 2e-3 * scale).mean())
            worst = max(worst, fig[name + " share"])
        assert np.array_equal(out[k32 + "indices"], out[k64 + "indices"])
        print(f"(b) {mode}: float32 against float64:", {k: f"{v:.1e}" for k, v in fig.items()})
    return worst


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="the reference's Point_Cloud_Resistration/losses directory")
    ap.add_argument("--seed", type=int, default=2021)
    args = ap.parse_args()
    ref = load_reference(args.reference)
    torch.set_num_threads(8)
    out = {}
    state0 = module_cases(ref, out)
    wrapper_runs(ref, state0, out, args.seed)
    share = gaps(out)
    assert share <= 0.005, f"{share:.2%} of an input gradient's entries differ by more than 2e-3: try another --seed"
    buf = io.BytesIO()
    np.savez_compressed(buf, **out)
    size = buf.getbuffer().nbytes
    assert size < 1024 * 1024, size
    with open(OUT, "wb") as f:
        f.write(buf.getbuffer())
    print("wrote", OUT, size, "bytes")


if __name__ == "__main__":
    main()
