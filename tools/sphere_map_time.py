"""Timing of the sphere encoder (sphere_map.py transform_to_sphere; csrc/shw_sphere_map.hip) through four paths:

    fused             the forward and backward kernels, the six parameter tensors concatenated by torch
    fused_graphed     the same replayed from a captured graph
    composed          the same module forced onto its composed torch path, eager
    composed_graphed  the composed path replayed from a captured graph: the eager path without its launch overhead

each for the forward alone (no_grad) and for forward + backward to the points and to every parameter, at (B, N) = (32, 512),
the shape of the reference's `__main__`, and at (64, 2048).  One process, HIP events, 10 warm-ups and 50 timed calls; median
and minimum are reported and every repetition kept.

Then one trainer-level call of max_spherical_wassersten_distance_fast in train mode -- 512 slices, max_iter = 10, B = 32,
N = 2048, Adam(lr=0.01, betas=(0.5, 0.999), capturable=True), directions drawn per iteration -- with the module fused and
forced composed, eager and with graph=True: 5 warm-up calls (the first captures), 20 timed calls, each from the same
parameters and a zeroed optimizer state (the loss kernels' time depends on where the ascent has moved the clouds), the
median call divided by max_iter (so each "inner iteration" carries a tenth of the call's final evaluation and of its two
input copies).
usage: python tools/sphere_map_time.py [out.json]      (default profiles/r29_sphere_map_time.json)"""
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import shw_amd as shw  # noqa: E402

out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "r29_sphere_map_time.json")
CASES = [(32, 512), (64, 2048)]
WARMUP, REPS = 10, 50
TRAINER = {"B": 32, "N": 2048, "L": 512, "max_iter": 10, "warmup_calls": 5, "timed_calls": 20}
DEV = torch.device("cuda", 0)
KINDS = ("forward", "forward_backward")


def events_ms(fn, warmup=WARMUP, reps=REPS, before=None):
    for _ in range(warmup):
        if before is not None:
            before()
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        if before is not None:
            before()
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
for B, N in CASES:
    torch.manual_seed(0)
    phi = shw.transform_to_sphere().to(DEV)
    g = torch.Generator().manual_seed(1)
    x = torch.randn(B, N, 3, generator=g).to(DEV)
    cot = torch.randn(B, N, 3, generator=g).to(DEV)
    case = {"B": B, "N": N}
    for path in ("fused", "fused_graphed", "composed", "composed_graphed"):
        phi.fused = path.startswith("fused")
        fwd, fb = forward_only(phi, x), forward_backward(phi, x, cot)
        if path.endswith("graphed"):
            fwd, fb = graphed(fwd), graphed(fb)
        case[path] = {"forward": events_ms(fwd), "forward_backward": events_ms(fb)}
    for other in ("composed_graphed", "composed"):
        case[other + "_over_fused"] = {k: case[other][k]["median_ms"] / case["fused"][k]["median_ms"] for k in KINDS}
    res["cases"].append(case)
    print(json.dumps({"B": B, "N": N, **{p: {k: round(case[p][k]["median_ms"], 4) for k in KINDS}
                                         for p in ("fused", "fused_graphed", "composed", "composed_graphed")}}))

# ------------------------------------------------------------------------------------------------ one trainer-level call
t = TRAINER
g = torch.Generator().manual_seed(2)
first = torch.randn(t["B"], t["N"], 3, generator=g).to(DEV)
second = (0.6 * torch.randn(t["B"], t["N"], 3, generator=g) + torch.tensor([1.0, -0.7, 0.4])).to(DEV)
trainer = dict(t)
for path in ("fused", "composed"):
    for mode in ("eager", "graph"):
        torch.manual_seed(0)
        phi = shw.transform_to_sphere_fast().to(DEV)
        phi.fused = path == "fused"
        opt = torch.optim.Adam(phi.parameters(), lr=0.01, betas=(0.5, 0.999), capturable=True)
        crit = shw.max_spherical_wassersten_distance_fast(t["L"], phi, shw.sliced_wasserstein_sphere_fast, opt, p=2,
                                                          max_iter=t["max_iter"], device=DEV, graph=mode == "graph")
        start = {k: v.clone() for k, v in phi.state_dict().items()}

        def restart():
            """every call from the same parameters and a fresh optimizer state, in place (the graph holds the addresses):
            the loss kernels' time depends on where the ascent has moved the clouds"""
            phi.load_state_dict(start)
            for state in opt.state.values():
                for v in state.values():
                    v.zero_()

        timing = events_ms(lambda: crit(first, second, "train")[0], warmup=t["warmup_calls"], reps=t["timed_calls"],
                           before=restart)
        timing["per_inner_iteration_ms"] = timing["median_ms"] / t["max_iter"]
        trainer[f"{path}_{mode}"] = timing
for mode in ("eager", "graph"):
    trainer[f"composed_over_fused_{mode}"] = trainer[f"composed_{mode}"]["median_ms"] / trainer[f"fused_{mode}"]["median_ms"]
res["trainer_call"] = trainer
print(json.dumps({"trainer_call per inner iteration, ms": {k: round(v["per_inner_iteration_ms"], 4)
                                                           for k, v in trainer.items() if isinstance(v, dict)}}))
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "w") as fh:
    json.dump(res, fh, indent=1)
