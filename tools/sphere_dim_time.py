"""Time of the D-generic spherical sliced-W path beside the R^3 kernels, in one process.

Shape: config 3 (B = 64, n = m = 2048, L = 512, p = 2) at d = 3 through the D-generic path (`_PairLossesDim`, forced), d = 8
and d = 64, and d = 3 through the R^3 kernels that every d = 3 call reaches.  Then the notebooks' shape (B = 1,
n = m = 1200, L = 100: a handful of workgroups for the two point kernels) at d = 6, a phi that lifts R^3 to R^6, beside
the R^3 kernels.  Per variant: the loss (`no_grad`: coordinates of both clouds, circle-level solve, reduction) and the
training step (the same with coefficient rows, then `backward()` through the point-gradient kernel); for the D-generic
variants also the coordinates kernel alone (both clouds) and the point-gradient kernel alone, as shares of the training
step.  Warm-up and event protocol of tools/f64_time.py: HIP events around RUNS calls, REPEATS windows after a warm-up; the
figure is the median window, smallest and largest beside it.

usage: python tools/sphere_dim_time.py [out.json]      (default profiles/r14_sphere_dim_time.json)"""
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import shw_amd as shw  # noqa: E402
from shw_amd import _lib, ssw  # noqa: E402

B, N, L, P = 64, 2048, 512, 2
NOTEBOOK = (1, 1200, 100)       # B, N, L
WARMUP, REPEATS = 3, 7


def inputs(d, B, N, L):
    g = torch.Generator().manual_seed(0)
    x = torch.nn.functional.normalize(torch.randn(B, N, d, generator=g), dim=-1)
    y = torch.nn.functional.normalize(torch.randn(B, N, d, generator=g), dim=-1)
    U = torch.linalg.qr(torch.randn(B, L, d, 2, generator=g))[0]
    return x.cuda(), y.cuda(), U.cuda()


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


def pair_losses(op, x, y, U, need_grad):
    return op.apply(x, y, U, float(P), False, None, None, need_grad, False)


def variant(op, d, generic, B=B, N=N, L=L):
    x, y, U = inputs(d, B, N, L)
    xg = x.clone().requires_grad_(True)

    def loss():
        with torch.no_grad():
            return pair_losses(op, x, y, U, False)[0]

    def train():
        xg.grad = None
        pair_losses(op, xg, y, U, True)[1].sum().backward()

    entry = {"d": d, "loss": measure(loss), "train": measure(train)}
    if generic:
        lib = _lib.load()
        stream = torch.cuda.current_stream().cuda_stream
        coords = torch.empty(2 * B * L * N, dtype=torch.float32, device="cuda")
        coef = torch.randn(2, B * L * N, dtype=torch.float32, device="cuda")
        gx, gy = torch.empty_like(x), torch.empty_like(y)

        def coords_both():
            for k, c in enumerate((x, y)):
                _lib.check(lib.shw_ssw_coords_dim(c.data_ptr(), U.data_ptr(), B, N, d, L, L * d * 2,
                                                  coords.data_ptr() + 4 * k * B * L * N, stream), "shw_ssw_coords_dim")

        def backward():
            _lib.check(lib.shw_ssw_backward_points_dim(x.data_ptr(), y.data_ptr(), U.data_ptr(), coef[0].data_ptr(),
                                                       coef[1].data_ptr(), B, N, N, d, L, L * d * 2, 1.0 / L, None, None,
                                                       gx.data_ptr(), gy.data_ptr(), stream), "shw_ssw_backward_points_dim")

        entry["coords_kernel"] = measure(coords_both)
        entry["backward_kernel"] = measure(backward)
        entry["coords_share_of_train"] = entry["coords_kernel"]["median_ms"] / entry["train"]["median_ms"]
        entry["backward_share_of_train"] = entry["backward_kernel"]["median_ms"] / entry["train"]["median_ms"]
        entry["coordinate_bytes_written_and_read"] = 4 * B * L * 2 * N
    ssw.SSWWorkspace.clear()
    torch.cuda.empty_cache()
    return entry


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "r14_sphere_dim_time.json")
    assert torch.cuda.is_available(), "needs a HIP device"
    result = {"device": torch.cuda.get_device_name(0), "B": B, "N": N, "L": L, "p": P, "warmup": WARMUP,
              "repeats": REPEATS, "variants": {}}
    base = variant(ssw._PairLosses, 3, False)
    result["variants"]["d3_r3_kernels"] = base
    print("d3_r3_kernels", json.dumps(base), flush=True)
    for name, d in (("d3_generic", 3), ("d8_generic", 8), ("d64_generic", 64)):
        entry = variant(ssw._PairLossesDim, d, True)
        for what in ("loss", "train"):
            entry[f"{what}_ratio_to_r3_kernels"] = entry[what]["median_ms"] / base[what]["median_ms"]
        result["variants"][name] = entry
        print(name, json.dumps(entry), flush=True)
    nb = dict(zip(("B", "N", "L"), NOTEBOOK))
    base = variant(ssw._PairLosses, 3, False, *NOTEBOOK)
    entry = variant(ssw._PairLossesDim, 6, True, *NOTEBOOK)
    for what in ("loss", "train"):
        entry[f"{what}_ratio_to_r3_kernels"] = entry[what]["median_ms"] / base[what]["median_ms"]
    result["notebook_shape"] = dict(nb, d3_r3_kernels=base, d6_generic=entry)
    print("notebook_shape", json.dumps(result["notebook_shape"]), flush=True)
    with open(out, "w") as fh:
        json.dump(result, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
