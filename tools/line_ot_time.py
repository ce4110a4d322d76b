"""Timing of the line transport (csrc/shw_line_ot.hip) at B = 64, L = 512, D = 3, p = 2 (one process, the warm-up and the
HIP events of tools/gsw_time.py; the median is reported and every repetition kept).

    uniform   2048 against 1536 points, no weights
    weighted  2048 against 2048 points, weights (B, n) and (B, m)
each as loss (no gradient) and training step (forward + backward to the source cloud) of
    fused      esw_slice_costs                                   (keys formed inside the kernel)
    composed   torch forms the (B, L, n) keys, line_ot_rows sorts and merges them
    eager      the same in plain torch: sort, cumsum, searchsorted, gather
and `esw_slice_sums` at 2048 against 2048 as the equal-size floor.
usage: python tools/line_ot_time.py [out.json]      (default profiles/r17_line_ot_time.json)"""
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import shw_amd as shw  # noqa: E402

out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "r17_line_ot_time.json")
B, L, D, P = 64, 512, 3, 2
WARMUP, REPS = 3, 10


def inputs(n, m, weighted):
    g = torch.Generator().manual_seed(17)
    xs = torch.randn(B, n, D, generator=g).cuda()
    xt = (torch.randn(B, m, D, generator=g) * 0.7 + 0.5).cuda()
    torch.manual_seed(17)
    th = shw.rand_projections(D, L).cuda()
    a = b = None
    if weighted:
        a, b = (torch.rand(B, n, generator=g) + 0.05).cuda(), (torch.rand(B, m, generator=g) + 0.05).cuda()
    return xs, xt, th, a, b


def keys(x, th):
    return torch.einsum("bnd,ld->bln", x, th)


def fused(xs, xt, th, a, b):
    return shw.esw_slice_costs(xs, xt, th, P, a, b)


def composed(xs, xt, th, a, b):
    wa = None if a is None else a.unsqueeze(1).expand(-1, L, -1)
    wb = None if b is None else b.unsqueeze(1).expand(-1, L, -1)
    return shw.line_ot_rows(keys(xs, th), keys(xt, th), P, wa, wb)


def eager(xs, xt, th, a, b):
    """the quantile merge in float32 torch ops"""
    ku, kv = keys(xs, th), keys(xt, th)
    n, m = ku.shape[-1], kv.shape[-1]
    us, iu = torch.sort(ku, dim=-1)
    vs, iv = torch.sort(kv, dim=-1)
    if a is None:
        A = (torch.arange(1, n + 1, device=ku.device, dtype=torch.float32) / n).expand_as(us)
        Bc = (torch.arange(1, m + 1, device=ku.device, dtype=torch.float32) / m).expand_as(vs)
    else:
        wa = (a / a.sum(-1, keepdim=True)).unsqueeze(1).expand(-1, L, -1)
        wb = (b / b.sum(-1, keepdim=True)).unsqueeze(1).expand(-1, L, -1)
        A = torch.cumsum(torch.gather(wa, -1, iu), -1)
        Bc = torch.cumsum(torch.gather(wb, -1, iv), -1)
        A = torch.cat([A[..., :-1], torch.ones_like(A[..., :1])], -1)
        Bc = torch.cat([Bc[..., :-1], torch.ones_like(Bc[..., :1])], -1)
    t = torch.sort(torch.cat([A, Bc], -1), dim=-1).values
    delta = torch.diff(t, dim=-1, prepend=torch.zeros_like(t[..., :1]))
    i = torch.searchsorted(A.contiguous(), t, right=False).clamp(max=n - 1)
    j = torch.searchsorted(Bc.contiguous(), t, right=False).clamp(max=m - 1)
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


def time_ops(ops, xs, xt, th, a, b):
    res = {}
    for name, fn in ops:
        def loss():
            with torch.no_grad():
                return fn(xs, xt, th, a, b)

        def train():
            x = xs.detach().requires_grad_(True)
            fn(x, xt, th, a, b).sum().backward()
            return x.grad
        res[name] = {"loss": events_ms(loss), "train_step": events_ms(train)}
        torch.cuda.empty_cache()
    return res


OPS = (("fused", fused), ("composed", composed), ("eager", eager))
res = {"device": torch.cuda.get_device_name(0), "B": B, "L": L, "D": D, "p": P}
for label, n, m, weighted in (("uniform_2048_1536", 2048, 1536, False), ("weighted_2048_2048", 2048, 2048, True)):
    args = inputs(n, m, weighted)
    r = time_ops(OPS, *args)
    with torch.no_grad():
        f, e = fused(*args), eager(*args)
    r["fused_vs_eager_max_rel_diff"] = ((f - e).abs() / e.abs()).max().item()
    r["ratios"] = {k: {"eager_over_fused": r["eager"][k]["median_ms"] / r["fused"][k]["median_ms"],
                       "composed_over_fused": r["composed"][k]["median_ms"] / r["fused"][k]["median_ms"]}
                   for k in ("loss", "train_step")}
    res[label] = {"n": n, "m": m, "weighted": weighted, **r}
    del args
    torch.cuda.empty_cache()
xs, xt, th, _, _ = inputs(2048, 2048, False)
res["esw_floor_2048"] = time_ops((("esw_slice_sums", lambda xs, xt, th, a, b: shw.esw_slice_sums(xs, xt, th, P)),), xs, xt,
                                 th, None, None)["esw_slice_sums"]
for label in ("uniform_2048_1536", "weighted_2048_2048"):
    res[label]["ratios"]["fused_over_esw_floor"] = {
        k: res[label]["fused"][k]["median_ms"] / res["esw_floor_2048"][k]["median_ms"] for k in ("loss", "train_step")}
res["fused_faster_than_eager"] = all(res[c]["ratios"][k]["eager_over_fused"] > 1.0
                                     for c in ("uniform_2048_1536", "weighted_2048_2048") for k in ("loss", "train_step"))
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "w") as fh:
    json.dump(res, fh, indent=1)
print(json.dumps({c: res[c]["ratios"] for c in ("uniform_2048_1536", "weighted_2048_2048")}))
print(json.dumps({"esw_floor_2048": {k: res["esw_floor_2048"][k]["median_ms"] for k in ("loss", "train_step")},
                  "fused_ms": {c: {k: res[c]["fused"][k]["median_ms"] for k in ("loss", "train_step")}
                               for c in ("uniform_2048_1536", "weighted_2048_2048")},
                  "fused_faster_than_eager": res["fused_faster_than_eager"]}))
