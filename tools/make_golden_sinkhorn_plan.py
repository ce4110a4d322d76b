"""G17: gradients of the REAL log_Sinkhorn_Distance_Loss / log_N_Sinkhorn_Distance_Loss through the plan P and the cost
matrix C they return (sinkhorn.py:46-60: both are autograd-visible), for tests/test_sinkhorn_plan_cpu.py (which pins
oracle/sinkhorn_mirror.py to them) and tests/test_sinkhorn_plan_gpu.py (the classes with plan_grad=True).

The reference module is loaded by file path, as oracle/make_golden.py does; run on a machine that has the reference
checkout:

    python tools/make_golden_sinkhorn_plan.py [path/to/losses/sinkhorn.py]

Writes tests/golden/g17_sinkhorn_plan.npz (arrays only).  Inputs x, y, w (B,), WP, WC (B, n, m), G (B, n, 3) are stored
explicitly.  For every setting: cost, gx, gy of  L = sum_b w_b cost_b + <WP, P> + <WC, C>  from the float32 run and
from the same inputs cast to float64, and the gap of the two per quantity (cost: largest relative difference; gradients:
largest difference in units of the largest entry) -- the g of the fixture tests.  For the first setting also gx, gy of
L = <G, P @ y / P.sum(-1)>."""
import importlib.util
import os
import sys

import numpy as np
import torch

REF = "/root/reference/Comparison_Wasserstein_with_Chamfer_distance/losses/sinkhorn.py"
OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests", "golden", "g17_sinkhorn_plan.npz")
B, N, M = 2, 48, 40
SETTINGS = {"L2": ("log_Sinkhorn_Distance_Loss", dict(eps=0.05, max_iter=60, type_of_cost_norm="L2")),
            "L1": ("log_Sinkhorn_Distance_Loss", dict(eps=0.05, max_iter=30, type_of_cost_norm="L1")),
            "N2": ("log_N_Sinkhorn_Distance_Loss", dict(eps=0.05, max_iter=30, type_of_cost_norm="L2",
                                                        type_of_Wasserstein_N="2"))}


def load(path):
    spec = importlib.util.spec_from_file_location("ref_sinkhorn", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def relmax(a, b):
    return float(np.max(np.abs(a - b) / np.maximum(np.abs(b), 1e-30)))


def of_largest(a, b):
    return float(np.abs(a - b).max() / np.abs(b).max())


def main():
    sk = load(sys.argv[1] if len(sys.argv) > 1 else REF)
    g = torch.Generator().manual_seed(20250117)
    x = torch.nn.functional.normalize(torch.randn(B, N, 3, generator=g), dim=-1)
    y = torch.nn.functional.normalize(torch.randn(B, M, 3, generator=g), dim=-1) * 0.9 + 0.05
    w = torch.tensor([1.0, -0.7])
    WP = torch.randn(B, N, M, generator=g)
    WC = torch.randn(B, N, M, generator=g) / (N * M)
    G = torch.randn(B, N, 3, generator=g)
    out = {"x": x.numpy(), "y": y.numpy(), "w": w.numpy(), "WP": WP.numpy(), "WC": WC.numpy(), "G": G.numpy()}

    def run(tag, dtype, map_loss):
        cls, kw = SETTINGS[tag]
        a, b = x.clone().to(dtype).requires_grad_(True), y.clone().to(dtype).requires_grad_(True)
        cost, P, C = getattr(sk, cls)(batch_reduction="none", **kw)(a, b, "cpu")
        if map_loss:
            loss = (G.to(dtype) * (P @ b / P.sum(-1, keepdim=True))).sum()
        else:
            loss = (cost * w.to(dtype)).sum() + (WP.to(dtype) * P).sum() + (WC.to(dtype) * C).sum()
        loss.backward()
        return {"cost": cost.detach().numpy(), "gx": a.grad.numpy(), "gy": b.grad.numpy()}

    for tag, map_loss in [(t, False) for t in SETTINGS] + [("L2", True)]:
        lo, hi = run(tag, torch.float32, map_loss), run(tag, torch.float64, map_loss)
        key = "map" if map_loss else tag
        for q in ("gx", "gy") if map_loss else ("cost", "gx", "gy"):
            out[f"{q}_{key}_f32"] = lo[q]
            out[f"{q}_{key}_f64"] = hi[q]
            out[f"gap_{q}_{key}"] = np.float64(relmax(lo[q], hi[q]) if q == "cost" else of_largest(lo[q], hi[q]))
    np.savez_compressed(OUT, **out)
    print(OUT, os.path.getsize(OUT), "bytes;", {k: float(v) for k, v in out.items() if k.startswith("gap_")})


if __name__ == "__main__":
    main()
