"""tools/make_golden_sphere_map.py -- fixture G20 (tests/golden/g20_sphere_map.npz): the reference's sphere encoder
`transform_to_sphere` / `transform_to_sphere_fast` and the two phi-max wrappers driven with it, captured from the REAL
reference (it needs a checkout of it; the tests need only the fixture).  Arrays and names only.

max_spherical_sliced_w.py and max_spherical_sliced_w_fast.py are imported by file path, as oracle/make_golden.py does
(their package __init__ needs POT); they import matplotlib, so MPLBACKEND=Agg is set.

(a) The module alone.  `torch.manual_seed(0); transform_to_sphere()`: the state as constructed (`a.s1.params`) and the
    same state with every weight x 3 (`a.s3.params`; at initialisation all points land in a small patch of the sphere,
    x 3 spreads them over it and into the saturating part of tanh).  For the input `a.x` (2, 70, 3) and the cotangent
    `a.cot`, per scale: the output `a.<s>.out`, d/dx `a.<s>.grad_x`, and the six parameter gradients `a.<s>.grad_params`,
    in float32 as the reference computes them.  Parameters and their gradients are stored as one flat vector each: the six
    tensors `a.state_names` (shapes `a.state_shapes`) in order.  transform_to_sphere_fast is asserted to give the same bits.
(b) The real wrappers, max_spherical_wassersten_distance (`pair`) and max_spherical_wassersten_distance_fast (`fast`), phi
    the real encoder from the x 3 state, Adam(lr=0.01, betas=(0.5, 0.999)), max_iter=2, modes train and test, B=2, N=70,
    SSW the reference's own sliced_cost on 16 fixed stored frames (`b.U_pair`, `b.U_batch`), as fixture G8.  Per dtype
    (`f32`, `f64`: the reference takes its dtype from the input), wrapper and mode: the returned `ssw`, the printed
    `trace`, the final parameters `params`, both mapped clouds `phi_first`, `phi_second`, and the gradients of the
    returned value w.r.t. both inputs `g_first`, `g_second` -- as ONE vector `b.<dtype>.<tag>_<mode>`, the fields in the
    order `b.fields_<mode>` with the shapes `b.shapes_<mode>`.  In test mode nothing is printed, phi does not move and
    both wrappers return the same maps: those are stored once, as `b.<dtype>.test.phi_first` / `.phi_second`.
    Asserted before writing: the float32 run is at least 4 x inside each tolerance the device tests apply
    (tests/test_r2_gpu.py:66-98) of the float64 run.

    python tools/make_golden_sphere_map.py --reference <reference checkout>/Point_Cloud_Resistration/losses
"""
import argparse
import contextlib
import copy
import importlib.util
import io
import os

os.environ.setdefault("MPLBACKEND", "Agg")

import numpy as np  # noqa: E402
import torch  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden", "g20_sphere_map.npz")
MARGIN = 4.0
B, N, L, ITERS, LR, BETAS = 2, 70, 16, 2, 0.01, (0.5, 0.999)
FIELDS = {"train": ("ssw", "trace", "params", "phi_first", "phi_second", "g_first", "g_second"),
          "test": ("ssw", "params", "g_first", "g_second")}


def load(name, path):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def npy(t):
    return t.detach().cpu().numpy()


def flat(tensors):
    """tensors in state-dict order as one vector (one archive member, not six tiny ones)"""
    return np.concatenate([npy(t).reshape(-1) for t in tensors])


def times3(state):
    return {k: (v * 3 if k.endswith(".weight") else v.clone()) for k, v in state.items()}


def module_alone(ref, ref_fast, out):
    torch.manual_seed(0)
    phi = ref.transform_to_sphere()
    torch.manual_seed(0)
    phi_fast = ref_fast.transform_to_sphere_fast()
    s1 = copy.deepcopy(phi.state_dict())
    assert list(s1) == list(phi_fast.state_dict()) and all(torch.equal(s1[k], v) for k, v in phi_fast.state_dict().items())
    g = torch.Generator().manual_seed(20)
    x, cot = torch.randn(B, N, 3, generator=g), torch.randn(B, N, 3, generator=g)
    out.update({"a.state_names": np.array(list(s1)), "a.x": npy(x), "a.cot": npy(cot),
                "a.state_shapes": np.array(["x".join(map(str, t.shape)) for t in s1.values()])})
    for tag, state in (("s1", s1), ("s3", times3(s1))):
        results = []
        for net in (phi, phi_fast):
            net.load_state_dict(state, strict=True)
            net.zero_grad()
            xs = x.clone().requires_grad_()
            y = net(xs)
            (y * cot).sum().backward()
            results.append([y.detach(), xs.grad] + [p.grad.clone() for p in net.parameters()])
        assert all(torch.equal(a, b) for a, b in zip(*results)), "the two reference classes disagree"
        out[f"a.{tag}.params"] = flat(state.values())
        out[f"a.{tag}.out"], out[f"a.{tag}.grad_x"] = npy(results[0][0]), npy(results[0][1])
        out[f"a.{tag}.grad_params"] = flat(results[0][2:])
        spread = npy(results[0][0]).reshape(-1, 3)
        print(f"(a) {tag}: mapped points span", spread.min(0).round(2), spread.max(0).round(2))
    return times3(s1)


def wrappers(ref, ref_fast, state, out, seed):
    g = torch.Generator().manual_seed(seed)
    first = torch.randn(B, N, 3, generator=g)
    second = 0.6 * torch.randn(B, N, 3, generator=g) + torch.tensor([1.0, -0.7, 0.4])     # clearly another cloud
    U_pair = torch.linalg.qr(torch.randn(L, 3, 2, generator=g))[0]
    U_batch = torch.linalg.qr(torch.randn(B, L, 3, 2, generator=g))[0]
    out.update({"b.first": npy(first), "b.second": npy(second), "b.U_pair": npy(U_pair), "b.U_batch": npy(U_batch),
                "b.max_iter": np.int64(ITERS), "b.lr": np.float64(LR), "b.betas": np.array(BETAS)})
    for dname, dtype in (("f32", torch.float32), ("f64", torch.float64)):
        def ssw_pair(a, b, num_projections, device, p=2):
            return ref.sliced_cost(a, b, U_pair.to(dtype), p=p)

        def ssw_batch(a, b, num_projections, device, p=2):
            return ref_fast.sliced_cost(a, b, U_batch.to(dtype), p=p)

        for tag, phi_cls, cls, fn in (
                ("pair", ref.transform_to_sphere, ref.max_spherical_wassersten_distance, ssw_pair),
                ("fast", ref_fast.transform_to_sphere_fast, ref_fast.max_spherical_wassersten_distance_fast, ssw_batch)):
            for mode in ("train", "test"):
                phi = phi_cls()
                phi.load_state_dict(state, strict=True)
                phi = phi.to(dtype)
                opt = torch.optim.Adam(phi.parameters(), lr=LR, betas=BETAS)
                crit = cls(L, phi, fn, opt, p=2, max_iter=ITERS, device="cpu")
                a, b = first.to(dtype).clone().requires_grad_(), second.to(dtype).clone().requires_grad_()
                buf = io.StringIO()
                with contextlib.redirect_stdout(buf):             # the wrappers print ssw.item() per inner iteration
                    ssw, fa, fb = crit(a, b, train_or_test=mode)
                opt.zero_grad()
                ssw.sum().backward()
                key = f"b.{dname}.{tag}_{mode}."
                out[key + "ssw"] = npy(ssw).reshape(-1)
                out[key + "trace"] = np.array([float(t) for t in buf.getvalue().split()], dtype=np.float64)
                out[key + "params"] = flat(phi.state_dict().values())
                if mode == "test":                                # phi has not moved: both wrappers return the same maps
                    key_maps = f"b.{dname}.test."
                    assert tag == "pair" or (np.array_equal(out[key_maps + "phi_first"], npy(fa))
                                             and np.array_equal(out[key_maps + "phi_second"], npy(fb)))
                    out[key_maps + "phi_first"], out[key_maps + "phi_second"] = npy(fa), npy(fb)
                else:
                    out[key + "phi_first"], out[key + "phi_second"] = npy(fa), npy(fb)
                out[key + "g_first"], out[key + "g_second"] = npy(a.grad), npy(b.grad)


def check_margins(out):
    """the reference's own float32-versus-float64 discrepancy against the device tests' tolerances / MARGIN; returns the
    worst ratio discrepancy / tolerance (must be <= 1 / MARGIN)"""
    worst = 0.0
    for tag in ("pair", "fast"):
        for mode in ("train", "test"):
            k32, k64 = f"b.f32.{tag}_{mode}.", f"b.f64.{tag}_{mode}."
            ratios = {}
            for name in ("ssw", "trace"):
                if len(out[k64 + name]):
                    ratios[name] = float(np.max(np.abs(out[k32 + name] - out[k64 + name]) / np.abs(out[k64 + name]))) / 1e-4
            m32, m64 = (k32, k64) if mode == "train" else ("b.f32.test.", "b.f64.test.")
            ratios["params, maps"] = max([float(np.abs(out[k32 + "params"] - out[k64 + "params"]).max())]
                                         + [float(np.abs(out[m32 + n] - out[m64 + n]).max())
                                            for n in ("phi_first", "phi_second")]) / 1e-3
            for name in ("g_first", "g_second"):
                want = out[k64 + name]
                scale, err = np.abs(want).max(), np.abs(out[k32 + name] - want)
                ratios[name + " max"] = float(err.max() / scale) / 5e-2
                # the share of entries over the small threshold must stay under 2 % with the threshold MARGIN x lower
                ratios[name + " share"] = float((err > 2e-3 / MARGIN * scale).mean()) / 0.02 / MARGIN
            print(f"(b) {tag} {mode}: discrepancy / tolerance:", {k: f"{v:.2e}" for k, v in ratios.items()})
            worst = max(worst, max(ratios.values()))
    return worst


def pack_runs(out):
    """one vector per run, its fields in the order of `b.fields_<mode>` with the shapes `b.shapes_<mode>`, in the run's
    dtype (a float32 run's printed values are float32 values): an archive member costs a few hundred bytes"""
    for mode, fields in FIELDS.items():
        out[f"b.fields_{mode}"] = np.array(fields)
        out[f"b.shapes_{mode}"] = np.array(["x".join(map(str, out[f"b.f32.pair_{mode}.{f}"].shape)) for f in fields])
        for dname in ("f32", "f64"):
            for tag in ("pair", "fast"):
                key = f"b.{dname}.{tag}_{mode}"
                dtype = out[key + ".g_first"].dtype           # (the batched reference sums its value in float32 always)
                parts = [out.pop(f"{key}.{f}").astype(dtype).reshape(-1) for f in fields]
                assert mode == "train" or len(out.pop(key + ".trace")) == 0
                out[key] = np.concatenate(parts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="the reference's Point_Cloud_Resistration/losses directory")
    ap.add_argument("--seed", type=int, default=2020)
    args = ap.parse_args()
    ref = load("ref_ssw", os.path.join(args.reference, "max_spherical_sliced_w.py"))
    ref_fast = load("ref_ssw_fast", os.path.join(args.reference, "max_spherical_sliced_w_fast.py"))
    torch.set_num_threads(8)
    out = {}
    state3 = module_alone(ref, ref_fast, out)
    wrappers(ref, ref_fast, state3, out, args.seed)
    worst = check_margins(out)
    assert worst <= 1.0 / MARGIN, f"float32 against float64 is only {1 / worst:.1f} x inside a tolerance: try another --seed"
    out["b.seed"] = np.int64(args.seed)
    pack_runs(out)
    buf = io.BytesIO()
    np.savez_compressed(buf, **out)
    size = buf.getbuffer().nbytes
    assert size < 100 * 1024, size
    with open(OUT, "wb") as f:
        f.write(buf.getbuffer())
    print("wrote", OUT, size, "bytes; worst discrepancy / tolerance", f"{worst:.3f}")


if __name__ == "__main__":
    main()
