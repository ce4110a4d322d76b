"""Timing and peak memory of the registration network's trunk (pcrnet.py MLP_Architecture.pooled; csrc/shw_pointnet.hip):

    fused             the forward and backward kernels
    fused_graphed     the same replayed from a captured graph
    composed          the module forced onto its composed torch path (five linear layers, ReLU, max), eager
    composed_graphed  the composed path replayed from a captured graph: the eager path without its launch overhead

each for the forward alone (no_grad) and for forward + backward to the points and to every trunk parameter, at
(B, N, emb) = (32, 2048, 1024) -- one trunk pass of the config-5 step -- and (64, 1024, 1024).  Then
`torch.cuda.max_memory_allocated` of one PCRNet training step (forward with 8 iterations, backward, Adam) at B = 32,
N = 2048, fused and composed, and the config-5 step (examples/config5_train_step.py) with its three --model values.
One process, HIP events, 10 warm-ups and 50 timed calls; median and minimum are reported and every repetition kept.
usage: python tools/pcrnet_time.py [out.json]      (default profiles/r26_pcrnet_time.json)"""
import importlib.util
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import shw_amd as shw  # noqa: E402

out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "r26_pcrnet_time.json")
CASES = [(32, 2048, 1024), (64, 1024, 1024)]
WARMUP, REPS = 10, 50
DEV = torch.device("cuda", 0)
PATHS = ("fused", "fused_graphed", "composed", "composed_graphed")


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


def forward_only(trunk, x):
    def run():
        with torch.no_grad():
            return trunk.pooled(x)
    return run


def forward_backward(trunk, x, cot):
    params = list(trunk.parameters())

    def run():
        for p in params:
            p.grad = None
        xs = x.detach().requires_grad_()
        (trunk.pooled(xs) * cot).sum().backward()
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


def save(res):
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as fh:
        json.dump(res, fh, indent=1)


res = {"device": torch.cuda.get_device_name(0), "warmup": WARMUP, "reps": REPS, "cases": []}
for B, N, emb in CASES:
    torch.manual_seed(0)
    trunk = shw.MLP_Architecture(emb).to(DEV)
    g = torch.Generator().manual_seed(1)
    x = torch.randn(B, N, 3, generator=g).to(DEV)
    cot = torch.randn(B, emb, generator=g).to(DEV)
    case = {"B": B, "N": N, "emb": emb}
    for path in PATHS:
        trunk.fused = path.startswith("fused")
        fwd, fb = forward_only(trunk, x), forward_backward(trunk, x, cot)
        if path.endswith("graphed"):
            fwd, fb = graphed(fwd), graphed(fb)
        case[path] = {"forward": events_ms(fwd), "forward_backward": events_ms(fb)}
        del fwd, fb
        torch.cuda.empty_cache()
    for other in ("composed", "composed_graphed"):
        case[f"{other}_over_fused"] = {k: case[other][k]["median_ms"] / case["fused"][k]["median_ms"]
                                       for k in ("forward", "forward_backward")}
    res["cases"].append(case)
    print(json.dumps({"B": B, "N": N, "emb": emb,
                      **{p: {k: round(case[p][k]["median_ms"], 4) for k in ("forward", "forward_backward")}
                         for p in PATHS}}), flush=True)
    save(res)
    del trunk
    torch.cuda.empty_cache()

# peak memory of one training step of PCRNet at the config-5 shape
res["pcrnet_step_peak_bytes"] = {}
for path in ("fused", "composed"):
    torch.manual_seed(0)
    model = shw.PCRNet().to(DEV)
    model.feature_model.fused = path == "fused"
    opt = torch.optim.Adam(model.parameters(), lr=1e-3)
    g = torch.Generator().manual_seed(2)
    template, source = torch.randn(32, 2048, 3, generator=g).to(DEV), torch.randn(32, 2048, 3, generator=g).to(DEV)

    def step():
        opt.zero_grad()
        model(template, source, 8)["transformed_source"].square().mean().backward()
        opt.step()

    step()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats(DEV)
    before = torch.cuda.memory_allocated(DEV)
    step()
    torch.cuda.synchronize()
    res["pcrnet_step_peak_bytes"][path] = {"peak": torch.cuda.max_memory_allocated(DEV), "held_before_the_step": before}
    del model, opt, step
    torch.cuda.empty_cache()
print(json.dumps(res["pcrnet_step_peak_bytes"]), flush=True)
save(res)

# the config-5 step, median of REPS steps after 2
spec = importlib.util.spec_from_file_location("config5_train_step", os.path.join(ROOT, "examples", "config5_train_step.py"))
config5 = importlib.util.module_from_spec(spec)
spec.loader.exec_module(config5)
res["config5_step"] = {}
for model in ("shaped", "pcrnet", "pcrnet-composed"):
    _, times = config5.run(steps=REPS + 2, verbose=False, model=model)
    res["config5_step"][model] = {"median_ms": 1e3 * statistics.median(times[2:]), "min_ms": 1e3 * min(times[2:]),
                                  "runs_ms": [1e3 * t for t in times[2:]]}
    torch.cuda.empty_cache()
    print(json.dumps({model: round(res["config5_step"][model]["median_ms"], 3)}), flush=True)
save(res)
