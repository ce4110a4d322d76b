"""Timing of the exact-W loss (csrc/shw_emd.hip) -- HIP events, one process, 2 warm-ups and 5 repetitions per figure, the
median reported and every repetition kept -- at (B = 64, n = 2048), (B = 32, n = 2048) and the notebooks' probe
(B = 1, n = 1200), on registration-like clouds (a rotated copy with 0.02 noise: the trainers' situation) and, for the
round counts, on independent sphere clouds as well:

    lp p = 2         emd_pair_costs, loss (no gradient) and training step (forward + backward to the source cloud)
    geodesic p = 2   loss
    scipy            scipy.optimize.linear_sum_assignment on the host, float64 costs, the first pairs of the batch only
                     (per-pair wall time; the stand-in for POT's CPU solver, which is not installed)
    sinkhorn         sinkhorn_pair_costs at eps 0.01 with 100 iterations (thresh 0: all of them), loss

usage: python tools/emd_time.py [out.json]      (default profiles/r20_emd_time.json)"""
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import shw_amd as shw  # noqa: E402

out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "r20_emd_time.json")
SHAPES = ((64, 2048), (32, 2048), (1, 1200))
WARMUP, REPS = 2, 5
SCIPY_PAIRS = 3


def unit(t):
    return torch.nn.functional.normalize(t, dim=-1)


def inputs(B, n, registered):
    g = torch.Generator().manual_seed(20 + n)
    x = unit(torch.randn(B, n, 3, generator=g))
    if not registered:
        return x.cuda(), unit(torch.randn(B, n, 3, generator=g)).cuda()
    rot = torch.linalg.qr(torch.randn(B, 3, 3, generator=g))[0]
    return x.cuda(), unit(x @ rot.transpose(1, 2) + 0.02 * torch.randn(B, n, 3, generator=g)).cuda()


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


def scipy_ms(x, y):
    from scipy.optimize import linear_sum_assignment
    times, costs = [], []
    for b in range(min(SCIPY_PAIRS, x.shape[0])):
        xb, yb = x[b].double().cpu().numpy(), y[b].double().cpu().numpy()
        t = time.perf_counter()
        C = ((xb[:, None, :] - yb[None, :, :]) ** 2).sum(-1)
        rows, cols = linear_sum_assignment(C)
        times.append((time.perf_counter() - t) * 1e3)
        costs.append(float(C[rows, cols].mean()))
    return {"per_pair_median_ms": statistics.median(times), "per_pair_runs_ms": times}, costs


def rounds_of(x, y, cost):
    with torch.no_grad():
        c, _, r = shw.emd_pair_costs(x, y, p=2, cost=cost, return_assignment=True)
    r = r.cpu().numpy()
    return c, {"mean": float(r.mean()), "max": int(r.max()), "per_n_mean": float(r.mean() / x.shape[1])}


res = {"device": torch.cuda.get_device_name(0), "warmup": WARMUP, "reps": REPS, "limit": shw.max_points_emd()}
for B, n in SHAPES:
    x, y = inputs(B, n, True)

    def loss(cost="lp"):
        with torch.no_grad():
            return shw.emd_pair_costs(x, y, p=2, cost=cost)

    def train():
        xs = x.detach().requires_grad_(True)
        shw.emd_pair_costs(xs, y, p=2).sum().backward()
        return xs.grad

    def sinkhorn():
        with torch.no_grad():
            return shw.sinkhorn_pair_costs(x, y, 0.01, 100, thresh=0.0)

    r = {"B": B, "n": n}
    r["lp_p2_loss"] = events_ms(loss)
    r["lp_p2_train_step"] = events_ms(train)
    r["geodesic_p2_loss"] = events_ms(lambda: loss("geodesic"))
    r["sinkhorn_eps0.01_100it_loss"] = events_ms(sinkhorn)
    cost, r["lp_p2_rounds"] = rounds_of(x, y, "lp")
    _, r["geodesic_p2_rounds"] = rounds_of(x, y, "geodesic")
    r["scipy_linear_sum_assignment"], ref = scipy_ms(x, y)
    r["max_abs_diff_to_scipy"] = float(np.abs(cost[:len(ref)].cpu().numpy().astype(np.float64) - np.array(ref)).max())
    r["scipy_batch_estimate_ms"] = r["scipy_linear_sum_assignment"]["per_pair_median_ms"] * B
    xi, yi = inputs(B, n, False)
    r["independent_clouds_lp_p2_loss"] = events_ms(lambda: shw.emd_pair_costs(xi, yi, p=2))
    _, r["independent_clouds_lp_p2_rounds"] = rounds_of(xi, yi, "lp")
    res[f"B{B}_n{n}"] = r
    print(json.dumps({f"B{B}_n{n}": {k: (v["median_ms"] if isinstance(v, dict) and "median_ms" in v else v)
                                     for k, v in r.items()}}), flush=True)
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "w") as fh:
    json.dump(res, fh, indent=1)
