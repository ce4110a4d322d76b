"""Timing of the sphere map phi (flows.py Norm_Flow_structure "Residual"; csrc/shw_flow.hip) through three paths:

    fused             the forward and backward kernels, parameters packed by torch operations
    composed          the same module forced onto its composed torch path, eager
    composed_graphed  the composed path replayed from a captured graph: the eager path without its launch overhead

each for the forward alone (no_grad) and for forward + backward to the points and to every parameter, at the trainer's
defaults Residual x 3 at (B, N) = (32, 1024), at (64, 2048), and Residual x 8 at (32, 1024).  One process, HIP events,
10 warm-ups and 50 timed calls; median and minimum are reported and every repetition kept.
usage: python tools/flow_time.py [out.json]      (default profiles/r25_flow_time.json)"""
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import shw_amd as shw  # noqa: E402

out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "r25_flow_time.json")
CASES = [(3, 32, 1024), (3, 64, 2048), (8, 32, 1024)]
WARMUP, REPS = 10, 50
DEV = torch.device("cuda", 0)


def events_ms(fn, warmup=WARMUP, reps=REPS):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b))
    return {"median_ms": statistics.median(times), "min_ms": min(times), "runs_ms": times}


def forward_only(phi, x):
    def run():
        with torch.no_grad():
            return phi(x)
    return run


def forward_backward(phi, x, cot):
    params = [p for p in phi.parameters()]

    def run():
        for p in params:
            p.grad = None
        xs = x.detach().requires_grad_()
        (phi(xs) * cot).sum().backward()
        return xs.grad
    return run


def graphed(fn):
    """fn captured once (after a side-stream warm-up) -> a callable that replays it"""
    side = torch.cuda.Stream(DEV)
    side.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(side):
        for _ in range(3):
            fn()
    torch.cuda.current_stream(DEV).wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        fn()
    return graph.replay


res = {"device": torch.cuda.get_device_name(0), "warmup": WARMUP, "reps": REPS, "cases": []}
for flows, B, N in CASES:
    torch.manual_seed(0)
    phi = shw.Norm_Flow_structure(3, "Residual", flows).to(DEV)
    g = torch.Generator().manual_seed(1)
    x = torch.nn.functional.normalize(torch.randn(B, N, 3, generator=g), dim=-1).to(DEV)
    cot = torch.randn(B, N, 3, generator=g).to(DEV)
    case = {"flows": flows, "B": B, "N": N}
    for path in ("fused", "composed", "composed_graphed"):
        phi.fused = path == "fused"
        fwd, fb = forward_only(phi, x), forward_backward(phi, x, cot)
        if path == "composed_graphed":
            fwd, fb = graphed(fwd), graphed(fb)
        case[path] = {"forward": events_ms(fwd), "forward_backward": events_ms(fb)}
    case["composed_graphed_over_fused"] = {k: case["composed_graphed"][k]["median_ms"] / case["fused"][k]["median_ms"]
                                           for k in ("forward", "forward_backward")}
    case["composed_over_fused"] = {k: case["composed"][k]["median_ms"] / case["fused"][k]["median_ms"]
                                   for k in ("forward", "forward_backward")}
    res["cases"].append(case)
    print(json.dumps({"flows": flows, "B": B, "N": N,
                      **{p: {k: round(case[p][k]["median_ms"], 4) for k in ("forward", "forward_backward")}
                         for p in ("fused", "composed", "composed_graphed")}}))
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "w") as fh:
    json.dump(res, fh, indent=1)
