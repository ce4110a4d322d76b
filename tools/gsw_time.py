"""Timing of the generalised sliced-W primitives and of the notebook call shapes built on them (one process, warm-ups,
HIP events around every timed repetition; the median is reported and every repetition kept).

    time   shape 1, B = 64, n = 2048, L = 512, D = 3, p = 2 -- loss (no gradient) and training step (forward + backward
           to the source cloud) of
             fused      gsw_circular_slice_sums                      (keys formed inside the kernel)
             composed   torch forms the (B, L, n) keys, sorted_row_sums sorts them
             eager      the same in plain torch with torch.sort
             esw_floor  esw_slice_sums at the same shape (a dot-product key: the floor of the fused call)
           shape 2, the notebooks' B = 1, n = 1200, L = 100 -- the calls as the flow loop makes them, forward +
           backward: GSWD_circular, max_GSWD_circular, distributional_sliced_wasserstein_distance (lam = 10,
           TransformNet-shaped f), max_gsw_nn_1 (MLP 3 -> 8 -> 8 -> 4); these draw from the CPU generator and step Adam,
           so they are timed with the host clock around runs that end in a device synchronise.
    step   one fused training step at shape 1 and nothing else: run it under `rocprofv3 --kernel-trace --stats`.
usage: python tools/gsw_time.py time [out.json]      (default profiles/r15_gsw_time.json)
       python tools/gsw_time.py step"""
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import shw_amd as shw  # noqa: E402

mode = sys.argv[1] if len(sys.argv) > 1 else "time"
out_path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "r15_gsw_time.json")
B, N, L, D, P, R = 64, 2048, 512, 3, 2, 1.0
WARMUP, REPS = 3, 10


def shape1():
    g = torch.Generator().manual_seed(15)
    xs = torch.randn(B, N, D, generator=g).cuda()
    xt = (torch.randn(B, N, D, generator=g) * 0.7 + 0.2).cuda()
    torch.manual_seed(15)
    th = shw.rand_projections(D, L).cuda()
    return xs, xt, th


def keys(x, th):
    return (x.unsqueeze(1) - (th * R).unsqueeze(0).unsqueeze(-2)).pow(2).sum(-1).sqrt()


def fused(xs, xt, th):
    return shw.gsw_circular_slice_sums(xs, xt, th, R, P)


def composed(xs, xt, th):
    return shw.sorted_row_sums(keys(xs, th), keys(xt, th), P)


def eager(xs, xt, th):
    return (torch.sort(keys(xs, th), dim=-1)[0] - torch.sort(keys(xt, th), dim=-1)[0]).abs().pow(P).sum(-1)


def esw_floor(xs, xt, th):
    return shw.esw_slice_sums(xs, xt, th, P)


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


def time_shape1():
    xs, xt, th = shape1()
    res = {}
    for name, fn in (("fused", fused), ("composed", composed), ("eager", eager), ("esw_floor", esw_floor)):
        def loss():
            with torch.no_grad():
                return fn(xs, xt, th)

        def train():
            x = xs.detach().requires_grad_(True)
            fn(x, xt, th).sum().backward()
            return x.grad
        res[name] = {"loss": events_ms(loss), "train_step": events_ms(train)}
        torch.cuda.empty_cache()
    a, b = fused(xs, xt, th), composed(xs, xt, th)
    res["fused_vs_composed_max_rel_diff"] = ((a - b).abs() / b.abs()).max().item()
    res["key_matrix_bytes_per_cloud"] = B * L * N * 4
    return res


def unit_rows_of(linear):
    """f for DSWD: a linear map whose output rows are scaled to unit length (the role of the notebooks' TransformNet)"""
    return lambda x: torch.nn.functional.normalize(linear(x), dim=1, eps=0.0)


def host_ms(step, steps=20, warmup=3):
    for _ in range(warmup):
        step()
    torch.cuda.synchronize()
    times = []
    for _ in range(3):
        t0 = time.perf_counter()
        for _ in range(steps):
            step()
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) / steps * 1e3)
    return {"median_ms": sorted(times)[1], "runs_ms": times, "steps_per_run": steps}


def time_shape2():
    g = torch.Generator().manual_seed(16)
    target = torch.rand(1200, 3, generator=g).cuda()
    first = torch.rand(1200, 3, generator=g).cuda().requires_grad_(True)
    torch.manual_seed(16)
    linear = torch.nn.Linear(3, 3).cuda()
    f = unit_rows_of(linear)
    f_op = torch.optim.Adam(linear.parameters(), lr=0.005, betas=(0.999, 0.999))
    net = torch.nn.Sequential(torch.nn.Linear(3, 8), torch.nn.LeakyReLU(), torch.nn.Linear(8, 8), torch.nn.LeakyReLU(),
                              torch.nn.Linear(8, 4)).cuda()
    net_op = torch.optim.Adam(net.parameters(), lr=0.005)
    calls = {
        "GSWD_circular": lambda: shw.GSWD_circular(first, target, p=2, num_projection=100, r=1, device="cuda"),
        "max_GSWD_circular": lambda: shw.max_GSWD_circular(first, target, p=2, r=1, device="cuda", max_iter=10),
        "distributional_sliced_wasserstein_distance": lambda: shw.distributional_sliced_wasserstein_distance(
            first, target, 100, f, f_op, p=2, max_iter=10, lam=10, device="cuda"),
        "max_gsw_nn_1": lambda: shw.max_gsw_nn_1(first, target, net, net_op, max_iter=10, p=2),
    }
    res = {}
    for name, call in calls.items():
        def step():
            first.grad = None
            call().backward()
        res[name] = host_ms(step)
    return res


res = {"device": torch.cuda.get_device_name(0), "mode": mode}
if mode == "time":
    res["shape1"] = {"B": B, "n": N, "L": L, "D": D, "p": P, "r": R, **time_shape1()}
    res["shape2"] = {"B": 1, "n": 1200, "L": 100, "D": 3, **time_shape2()}
    s1 = res["shape1"]
    res["fused_over_composed"] = {k: s1["fused"][k]["median_ms"] / s1["composed"][k]["median_ms"]
                                  for k in ("loss", "train_step")}
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as fh:
        json.dump(res, fh, indent=1)
elif mode == "step":
    xs, xt, th = shape1()
    x = xs.detach().requires_grad_(True)
    fused(x, xt, th).sum().backward()
    torch.cuda.synchronize()
else:
    raise SystemExit(__doc__)
print(json.dumps(res))
