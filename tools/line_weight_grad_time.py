"""Timing of the line transport's gradients with respect to the weights (csrc/shw_line_ot.hip line_ot_pot_kernel,
line_weight_reduce_kernel) at B = 64, L = 512, D = 3, p = 2, weighted, 2048 against 2048 points, weights (B, n) and (B, m)
(one process, the warm-up and the HIP events of tools/line_ot_time.py; the median is reported and every repetition kept).

The training step (forward + backward of the summed slice costs) of `esw_slice_costs` with the gradient going to
    points    the source cloud only: the call as it was, weight_grad left at False -- the yardstick
    weights   the two weight tensors only (weight_grad=True)
    both      the source cloud and the two weight tensors
and, for both of the last two, the same step in eager torch through the weight-differentiable quantile merge
(sort, cumsum, searchsorted, gather).
usage: python tools/line_weight_grad_time.py [out.json]      (default profiles/r24_line_weight_grad_time.json)"""
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import shw_amd as shw  # noqa: E402

out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "r24_line_weight_grad_time.json")
B, L, D, P, N, M = 64, 512, 3, 2, 2048, 2048
WARMUP, REPS = 3, 10


def inputs():
    g = torch.Generator().manual_seed(17)
    xs = torch.randn(B, N, D, generator=g).cuda()
    xt = (torch.randn(B, M, D, generator=g) * 0.7 + 0.5).cuda()
    torch.manual_seed(17)
    th = shw.rand_projections(D, L).cuda()
    a, b = (torch.rand(B, N, generator=g) + 0.05).cuda(), (torch.rand(B, M, generator=g) + 0.05).cuda()
    return xs, xt, th, a, b


def eager(xs, xt, th, a, b):
    """the quantile merge in float32 torch ops, the weights in the graph"""
    ku, kv = torch.einsum("bnd,ld->bln", xs, th), torch.einsum("bnd,ld->bln", xt, th)
    n, m = ku.shape[-1], kv.shape[-1]
    us, iu = torch.sort(ku, dim=-1)
    vs, iv = torch.sort(kv, dim=-1)
    wa = (a / a.sum(-1, keepdim=True)).unsqueeze(1).expand(-1, L, -1)
    wb = (b / b.sum(-1, keepdim=True)).unsqueeze(1).expand(-1, L, -1)
    A = torch.cumsum(torch.gather(wa, -1, iu), -1)
    Bc = torch.cumsum(torch.gather(wb, -1, iv), -1)
    A = torch.cat([A[..., :-1], torch.ones_like(A[..., :1])], -1)
    Bc = torch.cat([Bc[..., :-1], torch.ones_like(Bc[..., :1])], -1)
    t = torch.sort(torch.cat([A, Bc], -1), dim=-1).values
    delta = torch.diff(t, dim=-1, prepend=torch.zeros_like(t[..., :1]))
    i = torch.searchsorted(A.detach().contiguous(), t.detach(), right=False).clamp(max=n - 1)
    j = torch.searchsorted(Bc.detach().contiguous(), t.detach(), right=False).clamp(max=m - 1)
    d = torch.gather(us, -1, i) - torch.gather(vs, -1, j)
    return (delta * d.abs() ** P).sum(-1)


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


def step(fn, xs, xt, th, a, b, points, weights):
    def run():
        x = xs.detach().requires_grad_(points)
        wa, wb = a.detach().requires_grad_(weights), b.detach().requires_grad_(weights)
        fn(x, xt, th, wa, wb).sum().backward()
        return x.grad, wa.grad, wb.grad
    return run


def fused(weight_grad):
    return lambda xs, xt, th, a, b: shw.esw_slice_costs(xs, xt, th, P, a, b, weight_grad=weight_grad)


xs, xt, th, a, b = inputs()
res = {"device": torch.cuda.get_device_name(0), "B": B, "L": L, "D": D, "p": P, "n": N, "m": M}
res["fused"] = {
    "points": events_ms(step(fused(False), xs, xt, th, a, b, True, False)),
    "weights": events_ms(step(fused(True), xs, xt, th, a, b, False, True)),
    "both": events_ms(step(fused(True), xs, xt, th, a, b, True, True)),
    # the yardstick once more, after the others: the spread of the same call inside this process
    "points_again": events_ms(step(fused(False), xs, xt, th, a, b, True, False)),
}
torch.cuda.empty_cache()
res["eager"] = {"weights": events_ms(step(eager, xs, xt, th, a, b, False, True)),
                "both": events_ms(step(eager, xs, xt, th, a, b, True, True))}
torch.cuda.empty_cache()
ga = step(fused(True), xs, xt, th, a, b, False, True)()[1]
ge = step(eager, xs, xt, th, a, b, False, True)()[1]
res["fused_vs_eager_weight_grad_max_dev"] = ((ga - ge).abs().max() / ge.abs().max()).item()
base = res["fused"]["points"]["median_ms"]
res["ratios"] = {"weights_over_points": res["fused"]["weights"]["median_ms"] / base,
                 "both_over_points": res["fused"]["both"]["median_ms"] / base,
                 "points_again_over_points": res["fused"]["points_again"]["median_ms"] / base,
                 "eager_over_fused": {k: res["eager"][k]["median_ms"] / res["fused"][k]["median_ms"]
                                      for k in ("weights", "both")}}
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "w") as fh:
    json.dump(res, fh, indent=1)
print(json.dumps({"fused_ms": {k: v["median_ms"] for k, v in res["fused"].items()},
                  "eager_ms": {k: v["median_ms"] for k, v in res["eager"].items()}, "ratios": res["ratios"],
                  "fused_vs_eager_weight_grad_max_dev": res["fused_vs_eager_weight_grad_max_dev"]}))
