"""Timing of the exact-W loss between clouds of different sizes (csrc/shw_emd_units.hip) -- HIP events, one process,
2 warm-ups and 5 repetitions per figure, the median reported and every repetition kept -- at B = 32 on registration-like
clouds (both clouds sample one shape, the target rotated, with 0.02 noise), for the runner's shapes (128, 256) and
(128, 512), for (1024, 2048), and for (768, 1024), U = 3072:

    lp p = 2         transport_pair_costs, loss (no gradient) and training step (forward + backward to the source cloud)
    geodesic p = 2   loss
    composed         the same three through emd_pair_costs(x.repeat_interleave(ks, 1), y.repeat_interleave(kt, 1)), which
                     is what a caller could do before this kernel, where U = lcm(n, m) <= 2048; each figure is timed in
                     turns with the kernel's (kernel, composed, kernel, composed, ...)
    scipy            scipy.optimize.linear_sum_assignment on the host, the expanded U x U float64 matrix, the first pairs
                     of the batch only (per-pair wall time; the stand-in for POT's CPU solver, which is not installed)

usage: python tools/emd_units_time.py [out.json]      (default profiles/r22_emd_units_time.json)"""
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

out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "r22_emd_units_time.json")
B = 32
SHAPES = ((128, 256), (128, 512), (1024, 2048), (768, 1024))
WARMUP, REPS = 2, 5
SCIPY_PAIRS = 3


def unit(t):
    return torch.nn.functional.normalize(t, dim=-1)


def inputs(n, m):
    g = torch.Generator().manual_seed(22 + n + m)
    base = unit(torch.randn(B, max(n, m), 3, generator=g))
    rot = torch.linalg.qr(torch.randn(B, 3, 3, generator=g))[0]
    y = unit(base[:, :m] @ rot.transpose(1, 2) + 0.02 * torch.randn(B, m, 3, generator=g))
    return base[:, :n].contiguous().cuda(), y.cuda()


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


def events_ms_ab(fa, fb):
    """two functions timed in turns (a, b, a, b, ...): what shares the machine or moves the clock meets both alike"""
    for _ in range(WARMUP):
        fa()
        fb()
    torch.cuda.synchronize()
    times = ([], [])
    for _ in range(REPS):
        for fn, ts in zip((fa, fb), times):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            ts.append(a.elapsed_time(b))
    return tuple({"median_ms": statistics.median(ts), "min_ms": min(ts), "runs_ms": ts} for ts in times)


def scipy_ms(x, y, ks, kt):
    from scipy.optimize import linear_sum_assignment
    times, costs = [], []
    for b in range(min(SCIPY_PAIRS, x.shape[0])):
        xb, yb = x[b].double().cpu().numpy(), y[b].double().cpu().numpy()
        t = time.perf_counter()
        C = np.repeat(np.repeat(((xb[:, None, :] - yb[None, :, :]) ** 2).sum(-1), ks, axis=0), kt, axis=1)
        rows, cols = linear_sum_assignment(C)
        times.append((time.perf_counter() - t) * 1e3)
        costs.append(float(C[rows, cols].mean()))
    return {"per_pair_median_ms": statistics.median(times), "per_pair_runs_ms": times}, costs


def rounds_of(x, y, cost):
    with torch.no_grad():
        c, _, r = shw.transport_pair_costs(x, y, p=2, cost=cost, return_plan=True)
    r = r.cpu().numpy()
    return c, {"mean": float(r.mean()), "max": int(r.max())}


res = {"device": torch.cuda.get_device_name(0), "warmup": WARMUP, "reps": REPS, "B": B}
for n, m in SHAPES:
    U, ks, kt = shw.transport_units(n, m)
    x, y = inputs(n, m)

    def loss(cost="lp"):
        with torch.no_grad():
            return shw.transport_pair_costs(x, y, p=2, cost=cost)

    def train():
        xs = x.detach().requires_grad_(True)
        shw.transport_pair_costs(xs, y, p=2).sum().backward()
        return xs.grad

    def composed_loss(cost="lp"):
        with torch.no_grad():
            return shw.emd_pair_costs(x.repeat_interleave(ks, 1), y.repeat_interleave(kt, 1), p=2, cost=cost)

    def composed_train():
        xs = x.detach().requires_grad_(True)
        shw.emd_pair_costs(xs.repeat_interleave(ks, 1), y.repeat_interleave(kt, 1), p=2).sum().backward()
        return xs.grad

    r = {"n": n, "m": m, "units": U, "ks": ks, "kt": kt}
    if U <= shw.max_points_emd():
        r["lp_p2_loss"], r["composed_lp_p2_loss"] = events_ms_ab(loss, composed_loss)
        r["lp_p2_train_step"], r["composed_lp_p2_train_step"] = events_ms_ab(train, composed_train)
        r["geodesic_p2_loss"], r["composed_geodesic_p2_loss"] = events_ms_ab(lambda: loss("geodesic"),
                                                                             lambda: composed_loss("geodesic"))
    else:
        r["lp_p2_loss"] = events_ms(loss)
        r["lp_p2_train_step"] = events_ms(train)
        r["geodesic_p2_loss"] = events_ms(lambda: loss("geodesic"))
    cost, r["lp_p2_rounds"] = rounds_of(x, y, "lp")
    _, r["geodesic_p2_rounds"] = rounds_of(x, y, "geodesic")
    if U <= shw.max_points_emd():
        r["max_abs_diff_to_composed"] = float((cost - composed_loss()).abs().max())
        r["train_grad_max_abs_diff_to_composed"] = float((train() - composed_train()).abs().max())
    r["scipy_linear_sum_assignment"], ref = scipy_ms(x, y, ks, kt)
    r["max_abs_diff_to_scipy"] = float(np.abs(cost[:len(ref)].cpu().numpy().astype(np.float64) - np.array(ref)).max())
    r["scipy_batch_estimate_ms"] = r["scipy_linear_sum_assignment"]["per_pair_median_ms"] * B
    res[f"B{B}_n{n}_m{m}"] = r
    print(json.dumps({f"B{B}_n{n}_m{m}": {k: (v["median_ms"] if isinstance(v, dict) and "median_ms" in v else v)
                                          for k, v in r.items()}}), flush=True)
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "w") as fh:
    json.dump(res, fh, indent=1)
