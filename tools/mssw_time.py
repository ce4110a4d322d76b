"""Timing of the Residual-MSSW sphere encoder (mssw.py transform_to_sphere; csrc/shw_mssw.hip) through five paths:

    reference         the reference's own direction (reverse=True: the fixed-point inverse of every block, composed torch,
                      one flag read back per step): eager only, a graph cannot hold its data-dependent loop
    fused             forward blocks (reverse=False): the forward and backward kernels on packed_params() / packed_affine()
    fused_graphed     the same replayed from a captured graph
    composed          forward blocks forced onto the composed torch path, eager
    composed_graphed  that path replayed from a captured graph: the eager path without its launch overhead

each for the forward alone (no_grad) and for forward + backward to the points and to every parameter, at (B, N, F) =
(32, 64, 2), the shape of the reference's `__main__`, (32, 2048, 2) and (32, 2048, 3).  Every module is initialised by one
call on its input first.  One process, HIP events, 10 warm-ups and 50 timed calls; median and minimum are reported and
every repetition kept.

Then one trainer-level call of max_spherical_wassersten_distance_Residual in train mode -- 512 slices, max_iter = 10,
B = 32, N = 2048, psi_minibatch_size = 5, F = 2, Adam(lr=0.01, betas=(0.5, 0.999)), SSW the package's per-pair function --
with the reference's direction, and with forward blocks fused and composed, the subset map on and forced off: 3 warm-up
calls, 10 timed calls, each from the same parameters and a zeroed optimizer state, the median call divided by max_iter (so
each "inner iteration" carries a tenth of the call's final evaluation).
usage: python tools/mssw_time.py [out.json]      (default profiles/r32_mssw_time.json)"""
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import shw_amd as shw  # noqa: E402

out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "r32_mssw_time.json")
CASES = [(32, 64, 2), (32, 2048, 2), (32, 2048, 3)]
WARMUP, REPS = 10, 50
TRAINER = {"B": 32, "N": 2048, "L": 512, "max_iter": 10, "psi_minibatch_size": 5, "flows": 2, "warmup_calls": 3,
           "timed_calls": 10}
DEV = torch.device("cuda", 0)
KINDS = ("forward", "forward_backward")
PATHS = ("reference", "fused", "fused_graphed", "composed", "composed_graphed")


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


def module(flows, reverse, x):
    torch.manual_seed(0)
    phi = shw.mssw.transform_to_sphere("Residual", n_flow_layer=flows, reverse=reverse).to(DEV)
    with torch.no_grad():
        phi(x)                                                   # the data-dependent initialisation
    return phi


res = {"device": torch.cuda.get_device_name(0), "warmup": WARMUP, "reps": REPS, "cases": []}
for B, N, F in CASES:
    g = torch.Generator().manual_seed(1)
    x = torch.randn(B, N, 3, generator=g).to(DEV)
    cot = torch.randn(B, N, 3, generator=g).to(DEV)
    case = {"B": B, "N": N, "flows": F}
    for path in PATHS:
        phi = module(F, path == "reference", x)
        phi.fused = path.startswith("fused")
        fwd, fb = forward_only(phi, x), forward_backward(phi, x, cot)
        if path.endswith("graphed"):
            fwd, fb = graphed(fwd), graphed(fb)
        case[path] = {"forward": events_ms(fwd), "forward_backward": events_ms(fb)}
    for other in ("reference", "composed_graphed", "composed"):
        case[other + "_over_fused"] = {k: case[other][k]["median_ms"] / case["fused"][k]["median_ms"] for k in KINDS}
    res["cases"].append(case)
    print(json.dumps({"B": B, "N": N, "flows": F, **{p: {k: round(case[p][k]["median_ms"], 4) for k in KINDS} for p in PATHS}}))

# ------------------------------------------------------------------------------------------------ one trainer-level call
t = TRAINER
g = torch.Generator().manual_seed(2)
first = torch.randn(t["B"], t["N"], 3, generator=g).to(DEV)
second = (0.6 * torch.randn(t["B"], t["N"], 3, generator=g) + torch.tensor([1.0, -0.7, 0.4])).to(DEV)
trainer = dict(t)
for name, reverse, fused, subset in (("reference", True, False, False), ("fused_subset", False, True, True),
                                     ("fused_full", False, True, False), ("composed_subset", False, False, True),
                                     ("composed_full", False, False, False)):
    phi = module(t["flows"], reverse, first)
    phi.fused = fused
    opt = torch.optim.Adam(phi.parameters(), lr=0.01, betas=(0.5, 0.999))
    crit = shw.max_spherical_wassersten_distance_Residual(t["L"], phi, opt, p=2, max_iter=t["max_iter"],
                                                          psi_minibatch_size=t["psi_minibatch_size"], device=DEV)
    crit.subset_map = subset
    start = {k: v.clone() for k, v in phi.state_dict().items()}

    def restart():
        """every call from the same parameters, minibatches and a fresh optimizer state"""
        phi.load_state_dict(start)
        opt.state.clear()
        np.random.seed(0)
        torch.manual_seed(0)

    timing = events_ms(lambda: crit(first, second, "train")[0], warmup=t["warmup_calls"], reps=t["timed_calls"],
                       before=restart)
    timing["per_inner_iteration_ms"] = timing["median_ms"] / t["max_iter"]
    trainer[name] = timing
res["trainer_call"] = trainer
print(json.dumps({"trainer_call per inner iteration, ms": {k: round(v["per_inner_iteration_ms"], 4)
                                                           for k, v in trainer.items() if isinstance(v, dict)}}))
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "w") as fh:
    json.dump(res, fh, indent=1)
