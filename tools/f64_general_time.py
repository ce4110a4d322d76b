"""Time of the general float64 path (weights and / or n != m) beside the float32 general kernels, in one process.

Shapes: B = 64, L = 512, p = 2 for weighted n = m = 2048 and for 2048 against 1536 points (uniform).  Per shape and
dtype: the loss (`ssw_pair_losses` under no_grad: slice kernel + reduction) and the training step (forward with
coefficient rows, reduction, `backward()` through the point-gradient kernel).  Timing as tools/f64_time.py: HIP events
around RUNS calls, REPEATS windows after a warm-up; the figure is the median window, with the smallest and largest beside
it.  Inputs are float32-representable so that both precisions see the same clouds and weights.

usage: python tools/f64_general_time.py [out.json]            (all shapes, events)
       python tools/f64_general_time.py trace                 (a few calls per shape, for rocprofv3 --kernel-trace --stats)"""
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import shw_amd as shw  # noqa: E402
from f64_time import measure  # noqa: E402

SHAPES = (("weighted_2048x2048", 64, 2048, 2048, 512, True), ("uniform_2048x1536", 64, 2048, 1536, 512, False))
P = 2


def inputs(B, n, m, L, weighted, dtype):
    g = torch.Generator().manual_seed(0)
    x = torch.nn.functional.normalize(torch.randn(B, n, 3, generator=g), dim=-1)
    y = torch.nn.functional.normalize(torch.randn(B, m, 3, generator=g), dim=-1)
    U = torch.linalg.qr(torch.randn(B, L, 3, 2, generator=g))[0]
    wu = wv = None
    if weighted:
        wu, wv = torch.rand(n, generator=g) + 0.25, torch.rand(m, generator=g) + 0.25
        wu, wv = (wu / wu.sum()).to(dtype).cuda(), (wv / wv.sum()).to(dtype).cuda()
    return x.to(dtype).cuda(), y.to(dtype).cuda(), U.to(dtype).cuda(), wu, wv


def loss_call(x, y, U, wu, wv):
    with torch.no_grad():
        return shw.ssw_pair_losses(x, y, U, p=P, u_weights=wu, v_weights=wv)


def train_call(x, y, U, wu, wv):
    x.grad = None
    shw.sliced_cost(x, y, U, p=P, u_weights=wu, v_weights=wv).backward()


def main():
    mode = sys.argv[1] if len(sys.argv) > 1 else None
    assert torch.cuda.is_available(), "needs a HIP device"
    shw.enable_float64()
    shw.enable_float64_general()
    result = {"device": torch.cuda.get_device_name(0), "p": P, "shapes": {}}
    for name, B, n, m, L, weighted in SHAPES:
        entry = {"B": B, "n": n, "m": m, "L": L, "weighted": weighted}
        for dtype, tag in ((torch.float32, "float32"), (torch.float64, "float64")):
            x, y, U, wu, wv = inputs(B, n, m, L, weighted, dtype)
            xg = x.clone().requires_grad_(True)
            if mode == "trace":
                for _ in range(2):
                    loss_call(x, y, U, wu, wv)
                    train_call(xg, y, U, wu, wv)
                torch.cuda.synchronize()
                continue
            entry[tag] = {"loss": measure(lambda: loss_call(x, y, U, wu, wv)),
                          "train": measure(lambda: train_call(xg, y, U, wu, wv))}
            del x, y, U, xg
            shw.ssw.SSWWorkspace.clear()
            torch.cuda.empty_cache()
        if mode != "trace":
            for what in ("loss", "train"):
                entry[f"{what}_ratio_f64_over_f32"] = entry["float64"][what]["median_ms"] / entry["float32"][what]["median_ms"]
            result["shapes"][name] = entry
            print(name, json.dumps(entry), flush=True)
    if mode not in (None, "trace"):
        with open(mode, "w") as fh:
            json.dump(result, fh, indent=1)


if __name__ == "__main__":
    main()
