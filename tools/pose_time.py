"""Timing of what PCRNet does after its trunk (pose.py pose_head, pose_update; csrc/shw_pose.hip), at the trainer's shape
(B, N, emb, iterations) = (32, 2048, 1024, 8).  One process, HIP events, 10 warm-ups and 50 timed calls per figure; median
and minimum are reported and every repetition kept.

    share    shw.PCRNet forward + backward with the flags off, and its three parts each alone: the nine trunk passes, the
             eight heads (`linear` on the concatenation), the eight pose updates (`pose_update_composed`, chained)
    ops      forward and forward + backward of each op: fused, fused replayed from a graph, composed eager, composed
             replayed from a graph (null for the composed pose update: its `torch.eye(3).to(source)` is a copy from host
             memory, which a capture refuses)
    module   forward + backward of the module, in this order: flags off, fused_update, fused_head, both, flags off again;
             the spread between the two flags-off medians is the noise, and a configuration counts as faster only if it
             beats the first flags-off median by more than that
    trainer  (--trainer) the config-5 step of examples/config5_train_step.py with --model pcrnet and pcrnet-fused-pose,
             10 steps, the median of the last 8; a parent build is timed by running the parent's example next to it

usage: python tools/pose_time.py [out.json] [--trainer]      (default profiles/r31_pcrnet_pose_time.json)"""
import json
import os
import statistics
import subprocess
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import shw_amd as shw  # noqa: E402

args = [a for a in sys.argv[1:] if not a.startswith("--")]
out_path = args[0] if args else os.path.join(ROOT, "profiles", "r31_pcrnet_pose_time.json")
B, N, EMB, ITERATIONS = 32, 2048, 1024, 8
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


def commit():
    try:
        return subprocess.run(["git", "-C", ROOT, "rev-parse", "HEAD"], capture_output=True, text=True).stdout.strip() or None
    except OSError:
        return None


torch.manual_seed(0)
g = torch.Generator().manual_seed(1)
template = torch.randn(B, N, 3, generator=g).to(DEV)
source = torch.randn(B, N, 3, generator=g).to(DEV)
cot = torch.randn(B, N, 3, generator=g).to(DEV)
model = shw.PCRNet(shw.MLP_Architecture(EMB)).to(DEV)
params = list(model.parameters())
res = {"device": torch.cuda.get_device_name(0), "commit": os.environ.get("SHW_COMMIT") or commit(), "B": B, "N": N,
       "emb": EMB, "iterations": ITERATIONS, "warmup": WARMUP, "reps": REPS}


def module_step():
    for p in params:
        p.grad = None
    (model(template, source, ITERATIONS)["transformed_source"] * cot).sum().backward()


# ------------------------------------------------------------------------------------------------ the share
with torch.no_grad():
    feats_t = model.features(template).clone()
    feats_s = model.features(source).clone()
    vectors = [torch.randn(B, 7, generator=g).to(DEV) for _ in range(ITERATIONS)]
feat_cot = torch.randn(B, EMB, generator=g).to(DEV)
vec_cot = torch.randn(B, 7, generator=g).to(DEV)
eye = torch.eye(3, device=DEV).repeat(B, 1, 1)
zero_t = torch.zeros(B, 1, 3, device=DEV)


def trunk_passes():
    for p in params:
        p.grad = None
    packed = model.feature_model.packed_params()
    total = sum((model.features(x, packed) * feat_cot).sum() for x in [template] + [source] * ITERATIONS)
    total.backward()


def heads(fn, pack):
    def run():
        for p in params:
            p.grad = None
        t, s = feats_t.detach().requires_grad_(), feats_s.detach().requires_grad_()
        packed = model.packed_head_params() if pack else None         # once per forward, as the module does
        sum((fn(t, s, packed) * vec_cot).sum() for _ in range(ITERATIONS)).backward()
    return run


def updates(fn):
    def run():
        leaves = [v.detach().requires_grad_() for v in vectors]
        est_R, est_t, moved = eye, zero_t, source.detach().requires_grad_()
        for v in leaves:
            est_R, est_t, moved = fn(v, est_R, est_t, moved)
        (moved * cot).sum().backward()
    return run


composed_head = lambda t, s, packed: model.linear(torch.cat([t, s], dim=1))
fused_head = lambda t, s, packed: shw.pose_head(t, s, packed)
share = {"module_flags_off": events_ms(module_step), "nine_trunk_passes": events_ms(trunk_passes),
         "eight_heads_composed": events_ms(heads(composed_head, False)),
         "eight_pose_updates_composed": events_ms(updates(shw.pose_update_composed)),
         "eight_heads_fused": events_ms(heads(fused_head, True)), "eight_pose_updates_fused": events_ms(updates(shw.pose_update))}
res["share"] = share
print(json.dumps({"share, median ms": {k: round(v["median_ms"], 4) for k, v in share.items()}}))

# ------------------------------------------------------------------------------------------------ the ops
packed_head = model.packed_head_params().detach()


def head_op(fn, backward):
    t, s, p = feats_t.detach().requires_grad_(backward), feats_s.detach().requires_grad_(backward), \
        packed_head.detach().requires_grad_(backward)

    def run():
        if not backward:
            with torch.no_grad():
                return fn(t, s, p)
        return torch.autograd.grad((fn(t, s, p) * vec_cot).sum(), (t, s, p))
    return run


def update_op(fn, backward):
    v, moved = vectors[0].detach().requires_grad_(backward), source.detach().requires_grad_(backward)

    def run():
        if not backward:
            with torch.no_grad():
                return fn(v, eye, zero_t, moved)
        return torch.autograd.grad((fn(v, eye, zero_t, moved)[2] * cot).sum(), (v, moved))
    return run


ops = {}
for name, make, fused_fn, composed_fn in (("pose_head", head_op, shw.pose_head, shw.pose_head_composed),
                                          ("pose_update", update_op, shw.pose_update, shw.pose_update_composed)):
    ops[name] = {}
    for path, fn in (("fused", fused_fn), ("composed", composed_fn)):
        for kind, backward in (("forward", False), ("forward_backward", True)):
            run = make(fn, backward)
            ops[name].setdefault(path, {})[kind] = events_ms(run)
            if (name, path) == ("pose_update", "composed"):
                # `torch.eye(3).to(source)` copies from host memory on every call: the composed pose update cannot be
                # captured (hipErrorStreamCaptureUnsupported), and neither can the module with `fused_update` off
                ops[name].setdefault(path + "_graphed", {})[kind] = None
                continue
            ops[name].setdefault(path + "_graphed", {})[kind] = events_ms(graphed(run))
    print(json.dumps({name: {p: {k: v and round(v["median_ms"], 4) for k, v in kinds.items()} for p, kinds in ops[name].items()}}))
res["ops"] = ops

# ------------------------------------------------------------------------------------------------ the module
module = []
for label, head, update in (("flags_off", False, False), ("fused_update", False, True), ("fused_head", True, False),
                            ("both", True, True), ("flags_off_again", False, False)):
    model.fused_head, model.fused_update = head, update
    module.append({"configuration": label, **events_ms(module_step)})
model.fused_head = model.fused_update = False
noise = abs(module[0]["median_ms"] - module[-1]["median_ms"])
for row in module:
    row["faster_than_flags_off_by_more_than_the_noise"] = module[0]["median_ms"] - row["median_ms"] > noise
res["module"] = {"noise_ms": noise, "runs": module}
print(json.dumps({"module, median ms": {r["configuration"]: round(r["median_ms"], 4) for r in module}, "noise_ms": round(noise, 4)}))

# ------------------------------------------------------------------------------------------------ the trainer
if "--trainer" in sys.argv:
    sys.path.insert(0, os.path.join(ROOT, "examples"))
    import config5_train_step as example  # noqa: E402
    trainer = {}
    for name in ("pcrnet", "pcrnet-fused-pose", "pcrnet"):
        losses, times = example.run(B, N, 512, 10, verbose=False, model=name)
        key = name if name not in trainer else name + "_again"
        trainer[key] = {"median_step_ms": 1e3 * statistics.median(times[2:]), "steps_ms": [1e3 * t for t in times],
                        "losses": losses}
    res["trainer"] = trainer
    print(json.dumps({"trainer, median step ms": {k: round(v["median_step_ms"], 3) for k, v in trainer.items()}}))

os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "w") as fh:
    json.dump(res, fh, indent=1)
