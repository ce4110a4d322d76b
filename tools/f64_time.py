"""Time of the float64 path beside the float32 kernels, in one process.

Shapes: config 3 (B = 64, N = 2048, L = 512, p = 2) and the notebooks' shape (B = 1, N = 1200, L = 100, p = 2).
Per shape and dtype: the loss (`ssw_pair_losses` under no_grad: slice kernel + reduction) and the training step (forward
with coefficient rows, reduction, `backward()` through the point-gradient kernel).  HIP events around RUNS calls,
REPEATS windows after a warm-up of every shape; the figure is the median window, with the smallest and largest beside it.
Inputs are float32-representable so that both precisions see the same clouds.

usage: python tools/f64_time.py [out.json]            (all shapes, events)
       python tools/f64_time.py trace                 (a few calls per shape, for rocprofv3 --kernel-trace --stats)"""
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import shw_amd as shw  # noqa: E402

SHAPES = (("config3", 64, 2048, 512), ("notebook", 1, 1200, 100))
P = 2
WARMUP, REPEATS = 3, 7


def inputs(B, n, L, dtype):
    g = torch.Generator().manual_seed(0)
    x = torch.nn.functional.normalize(torch.randn(B, n, 3, generator=g), dim=-1)
    y = torch.nn.functional.normalize(torch.randn(B, n, 3, generator=g), dim=-1)
    U = torch.linalg.qr(torch.randn(B, L, 3, 2, generator=g))[0]
    return x.to(dtype).cuda(), y.to(dtype).cuda(), U.to(dtype).cuda()


def loss_call(x, y, U):
    with torch.no_grad():
        return shw.ssw_pair_losses(x, y, U, p=P)


def train_call(x, y, U):
    x.grad = None
    shw.sliced_cost(x, y, U, p=P).backward()


def window_ms(fn, runs):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(runs):
        fn()
    stop.record()
    torch.cuda.synchronize()
    return start.elapsed_time(stop) / runs


def measure(fn):
    for _ in range(WARMUP):
        fn()
    torch.cuda.synchronize()
    one = window_ms(fn, 1)
    runs = max(2, min(200, int(300.0 / max(one, 1e-3))))          # windows of about 0.3 s
    times = [window_ms(fn, runs) for _ in range(REPEATS)]
    return {"median_ms": statistics.median(times), "min_ms": min(times), "max_ms": max(times), "runs_per_window": runs}


def main():
    mode = sys.argv[1] if len(sys.argv) > 1 else None
    assert torch.cuda.is_available(), "needs a HIP device"
    shw.enable_float64()
    result = {"device": torch.cuda.get_device_name(0), "p": P, "warmup": WARMUP, "repeats": REPEATS, "shapes": {}}
    for name, B, n, L in SHAPES:
        entry = {"B": B, "N": n, "L": L}
        for dtype, tag in ((torch.float32, "float32"), (torch.float64, "float64")):
            x, y, U = inputs(B, n, L, dtype)
            xg = x.clone().requires_grad_(True)
            if mode == "trace":
                for _ in range(3):
                    loss_call(x, y, U)
                    train_call(xg, y, U)
                torch.cuda.synchronize()
                continue
            entry[tag] = {"loss": measure(lambda: loss_call(x, y, U)), "train": measure(lambda: train_call(xg, y, U))}
            del x, y, U, xg
            shw.ssw.SSWWorkspace.clear()
            torch.cuda.empty_cache()
        if mode != "trace":
            for what in ("loss", "train"):
                entry[f"{what}_ratio_f64_over_f32"] = entry["float64"][what]["median_ms"] / entry["float32"][what]["median_ms"]
            result["shapes"][name] = entry
            print(name, json.dumps(entry))
    if mode not in (None, "trace"):
        with open(mode, "w") as fh:
            json.dump(result, fh, indent=1)


if __name__ == "__main__":
    main()
