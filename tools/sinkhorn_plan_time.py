"""Times of the Sinkhorn plan-gradient paths (development aid, GPU): HIP events, warm-up, median of 7 windows, everything
in one process.  Shape of DESIGN.md 3.6: B = 64, n = m = 2048, eps = 0.01, 100 iterations.

    python tools/sinkhorn_plan_time.py [--parent path/to/parent/libshw_hip.so] [--out profiles/r16_sinkhorn_plan_time.json]
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/sinkhorn_plan_time.py --seeds-only     (seed kernel times)

  backward_cost_only : shw_sinkhorn_backward of this library and, with --parent, of the parent's, alternating window by window
  backward_dense     : shw_sinkhorn_backward_plan with dense GP and GC (2 GB of cotangents at this shape)
  map / composed     : sinkhorn_barycentric_map forward + backward of sum ||T - x||^2, against the same loss from the dense
                       P (plan_grad=True, P @ y in torch), with the peak of allocated memory of both
"""
import argparse
import ctypes
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import shw_amd as shw  # noqa: E402

B, N, M, EPS, ITERS = 64, 2048, 2048, 0.01, 100
WINDOWS, REPS = 7, 3


def bind(path):
    lib = ctypes.CDLL(path)
    for name in ("shw_sinkhorn_train_workspace_bytes", "shw_sinkhorn_forward_train", "shw_sinkhorn_backward"):
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = shw._lib._SIGNATURES[name]
    return lib


def window(fn):
    """ms per call over REPS calls between two events"""
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(REPS):
        fn()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) / REPS


def median_of(fns):
    """warm-up, then WINDOWS windows of every function in turn (alternating); medians"""
    for fn in fns.values():
        fn()
    torch.cuda.synchronize()
    times = {k: [] for k in fns}
    for _ in range(WINDOWS):
        for k, fn in fns.items():
            times[k].append(window(fn))
    return {k: {"median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v)} for k, v in times.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", default=None)
    ap.add_argument("--out", default=None)
    ap.add_argument("--seeds-only", action="store_true", help="five dense backward calls and nothing else (for a kernel trace)")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    g = torch.Generator().manual_seed(0)
    x = torch.nn.functional.normalize(torch.randn(B, N, 3, generator=g), dim=-1).to(dev)
    y = torch.nn.functional.normalize(torch.randn(B, M, 3, generator=g), dim=-1).to(dev)
    st = torch.cuda.current_stream().cuda_stream
    lib = shw._lib.load()
    gcost = torch.ones(B, device=dev)
    gx, gy = torch.empty_like(x), torch.empty_like(y)
    cost = torch.empty(B, device=dev)

    def trained(l):
        ws = torch.empty(l.shw_sinkhorn_train_workspace_bytes(B, N, M, ITERS), dtype=torch.uint8, device=dev)
        shw._lib.check(l.shw_sinkhorn_forward_train(x.data_ptr(), y.data_ptr(), B, N, M, EPS, ITERS, 2, 1, 1e-9, ws.data_ptr(),
                                                    cost.data_ptr(), None, None, st), "forward_train")
        return ws

    ws = trained(lib)
    GP = torch.randn(B, N, M, generator=torch.Generator(device=dev).manual_seed(1), device=dev)
    GC = torch.randn(B, N, M, generator=torch.Generator(device=dev).manual_seed(2), device=dev) / (N * M)

    def dense():
        shw._lib.check(lib.shw_sinkhorn_backward_plan(x.data_ptr(), y.data_ptr(), B, N, M, EPS, ITERS, 2, 1, ws.data_ptr(),
                                                      gcost.data_ptr(), GP.data_ptr(), GC.data_ptr(), gx.data_ptr(),
                                                      gy.data_ptr(), st), "backward_plan")

    if args.seeds_only:
        for _ in range(5):
            dense()
        torch.cuda.synchronize()
        return
    out = {"shape": {"B": B, "n": N, "m": M, "eps": EPS, "max_iter": ITERS}, "windows": WINDOWS, "reps_per_window": REPS,
           "device": torch.cuda.get_device_name(0)}

    def cost_only(l, w):
        return lambda: shw._lib.check(l.shw_sinkhorn_backward(x.data_ptr(), y.data_ptr(), B, N, M, EPS, ITERS, 2, 1, w.data_ptr(),
                                                              gcost.data_ptr(), gx.data_ptr(), gy.data_ptr(), st), "backward")

    fns = {"this": cost_only(lib, ws)}
    if args.parent:
        parent = bind(args.parent)
        fns["parent"] = cost_only(parent, trained(parent))
    out["backward_cost_only"] = median_of(fns)
    out["backward_dense"] = median_of({"this": dense})["this"]
    out["dense_cotangent_bytes_both_sides"] = 16 * B * N * M
    del GP, GC
    torch.cuda.empty_cache()

    def fused():
        xa, ya = x.clone().requires_grad_(True), y.clone().requires_grad_(True)
        T = shw.sinkhorn_barycentric_map(xa, ya, EPS, ITERS)
        ((T - xa) ** 2).sum().backward()

    def composed():
        xa, ya = x.clone().requires_grad_(True), y.clone().requires_grad_(True)
        _, P, _ = shw.sinkhorn_pair_costs(xa, ya, EPS, ITERS, return_plan=True, plan_grad=True)
        T = P @ ya / P.sum(-1, keepdim=True)
        ((T - xa) ** 2).sum().backward()

    for name, fn in (("map_forward_backward", fused), ("composed_forward_backward", composed)):
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.memory_allocated()
        out[name] = median_of({"this": fn})["this"]
        out[name]["peak_rise_bytes"] = torch.cuda.max_memory_allocated() - before
    text = json.dumps(out, indent=1)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
