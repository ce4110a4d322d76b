"""Timing of the spherical sliced-W gradients with respect to the weights (csrc/shw_ssw_weights.hip) at B = 64, L = 512,
n = m = 2048 points on S^2, per-pair weights (B, n) and (B, m), p = 2 (the cut search) and p = 1 (the level median); one
process, HIP events, medians of 10 after 3 warm-ups, every repetition kept.

The training step (forward + backward of `sliced_cost`) with the gradient going to
    clouds        the two clouds only: the call as it was -- the yardstick
    weights       the two weight tensors only
    both          clouds and weights
    clouds_again  the yardstick once more after the others: the spread of the same call inside this process
and the weights step in eager float32 torch through oracle.ref_mirror (the bisection with autograd at its fixed cut for
p = 2, the level-median formula for p = 1; pair by pair, as that code takes one weight row).
`--parent-tree DIR` also times the yardstick in a child process that imports the package from DIR, a built checkout of the
parent commit: the kernels of that step are unchanged, so the two should agree within the spread.
usage: python tools/circle_weight_grad_time.py [--parent-tree DIR] [out.json]
       (default profiles/r27_circle_weight_grad_time.json)"""
import json
import os
import statistics
import subprocess
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def option(name):
    """--name VALUE taken out of sys.argv, or None"""
    if name not in sys.argv:
        return None
    at = sys.argv.index(name)
    value = sys.argv[at + 1]
    del sys.argv[at:at + 2]
    return value


parent_tree = option("--parent-tree")
tree = option("--tree") or ROOT              # the checkout the package is imported from (the child of --parent-tree)
clouds_only = "--clouds-only" in sys.argv
args = [a for a in sys.argv[1:] if a != "--clouds-only"]
out_path = args[0] if args else os.path.join(ROOT, "profiles", "r27_circle_weight_grad_time.json")
sys.path.insert(0, os.path.abspath(tree))
import shw_amd as shw  # noqa: E402
from oracle import ref_mirror  # noqa: E402

B, L, N, M = 64, 512, 2048, 2048
WARMUP, REPS = 3, 10


def inputs():
    g = torch.Generator().manual_seed(27)
    xs = torch.nn.functional.normalize(torch.randn(B, N, 3, generator=g), dim=-1).cuda()
    xt = torch.nn.functional.normalize(torch.randn(B, M, 3, generator=g) * torch.tensor([1.0, 0.7, 0.4]), dim=-1).cuda()
    U = shw.stiefel_frames(torch.randn(B, L, 3, 2, generator=g).cuda())
    a, b = torch.rand(B, N, generator=g) + 0.2, torch.rand(B, M, generator=g) + 0.2
    return xs, xt, U, (a / a.sum(-1, keepdim=True)).cuda(), (b / b.sum(-1, keepdim=True)).cuda()


def events_ms(fn, warmup=WARMUP, reps=REPS):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        fn()
        t1.record()
        t1.synchronize()
        times.append(t0.elapsed_time(t1))
    return {"median_ms": statistics.median(times), "min_ms": min(times), "runs_ms": times}


def fused(p):
    return lambda xs, xt, U, a, b: shw.sliced_cost(xs, xt, U, p, u_weights=a, v_weights=b)


def eager(p):
    def run(xs, xt, U, a, b):
        total = 0.0
        for i in range(B):
            total = total + ref_mirror.per_slice_costs(xs[i], xt[i], U[i], p, a[i], b[i]).mean()
        return total
    return run


def step(fn, xs, xt, U, a, b, clouds, weights):
    def run():
        x, y = xs.detach().requires_grad_(clouds), xt.detach().requires_grad_(clouds)
        wa, wb = a.detach().requires_grad_(weights), b.detach().requires_grad_(weights)
        fn(x, y, U, wa, wb).sum().backward()
        return x.grad, wa.grad, wb.grad
    return run


xs, xt, U, a, b = inputs()
res = {"device": torch.cuda.get_device_name(0), "B": B, "L": L, "n": N, "m": M}
for p in (2, 1):
    key = f"p{p}"
    res[key] = {"clouds": events_ms(step(fused(p), xs, xt, U, a, b, True, False))}
    if clouds_only:
        continue
    res[key]["weights"] = events_ms(step(fused(p), xs, xt, U, a, b, False, True))
    res[key]["both"] = events_ms(step(fused(p), xs, xt, U, a, b, True, True))
    res[key]["clouds_again"] = events_ms(step(fused(p), xs, xt, U, a, b, True, False))
    torch.cuda.empty_cache()
    res[key]["eager_weights"] = events_ms(step(eager(p), xs, xt, U, a, b, False, True))
    torch.cuda.empty_cache()
    base = res[key]["clouds"]["median_ms"]
    res[key]["ratios"] = {k + "_over_clouds": res[key][k]["median_ms"] / base for k in ("weights", "both", "clouds_again")}
    res[key]["ratios"]["eager_over_fused_weights"] = res[key]["eager_weights"]["median_ms"] / res[key]["weights"]["median_ms"]
if clouds_only:
    print(json.dumps(res))
    sys.exit(0)
if parent_tree:
    # a fresh process that imports the package, and loads its library, from a built checkout of the parent commit
    child = subprocess.run([sys.executable, os.path.abspath(__file__), "--clouds-only", "--tree", parent_tree],
                           capture_output=True, text=True)
    if child.returncode != 0:
        raise RuntimeError("timing the parent's checkout failed:\n" + child.stderr)
    parent = json.loads(child.stdout.strip().splitlines()[-1])
    for p in (2, 1):
        res[f"p{p}"]["clouds_parent_commit"] = parent[f"p{p}"]["clouds"]
        res[f"p{p}"]["ratios"]["clouds_over_parent"] = (res[f"p{p}"]["clouds"]["median_ms"]
                                                       / parent[f"p{p}"]["clouds"]["median_ms"])
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "w") as fh:
    json.dump(res, fh, indent=1)
print(json.dumps({k: {q: (v["median_ms"] if isinstance(v, dict) and "median_ms" in v else v) for q, v in res[k].items()}
                  for k in ("p2", "p1")}))
