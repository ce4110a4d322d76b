"""Time of the frame gradients of the spherical sliced-W loss (csrc/shw_ssw_dirs.hip), in one process.

Config 3 (B = 64, n = m = 2048, L = 512, p = 2, per-pair frames):
  * the frame-gradient kernel alone and the point-gradient kernel alone on the same coefficient rows (both stream the same
    537 MB; the acceptance figure is their ratio);
  * the training step with gradients to the clouds only, to the frames only, and to both;
  * the composed path a caller had before: circle coordinates in eager torch, `shw.binary_search_circle` on the rows,
    autograd back to the frames.
The same at d = 8 and d = 64 (D-generic path) beside `shw_ssw_backward_points_dim`, and the host-clock latency of
`max_sliced_wasserstein_sphere` at the notebooks' shape (one pair, 1200 points, one frame, 10 ascent steps).
Event protocol of tools/sphere_dim_time.py: HIP events around windows of about 0.3 s after a warm-up, median of REPEATS.

usage: python tools/ssw_dirs_time.py [out.json]      (default profiles/r21_ssw_dirs_time.json)"""
import json
import math
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import shw_amd as shw  # noqa: E402
from shw_amd import _lib, ssw  # noqa: E402

B, N, L, P = 64, 2048, 512, 2
WARMUP, REPEATS = 3, 7


def inputs(d, B=B, N=N, L=L):
    """A displaced pair per batch entry (registration-like), per-pair frames."""
    g = torch.Generator().manual_seed(0)
    x = torch.nn.functional.normalize(torch.randn(B, N, d, generator=g), dim=-1)
    y = torch.randn(B, N, d, generator=g)
    y[..., 0] += 1.5
    y = torch.nn.functional.normalize(y, dim=-1)
    U = torch.linalg.qr(torch.randn(B, L, d, 2, generator=g))[0]
    return x.cuda(), y.cuda(), U.cuda()


def window_ms(fn, runs):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(runs):
        fn()
    stop.record()
    torch.cuda.synchronize()
    return start.elapsed_time(stop) / runs


def measure(fn):
    for _ in range(WARMUP):
        fn()
    torch.cuda.synchronize()
    one = window_ms(fn, 1)
    runs = max(2, min(200, int(300.0 / max(one, 1e-3))))
    times = [window_ms(fn, runs) for _ in range(REPEATS)]
    return {"median_ms": statistics.median(times), "min_ms": min(times), "max_ms": max(times), "runs_per_window": runs}


def kernels_alone(d):
    lib = _lib.load()
    x, y, U = inputs(d)
    stream = torch.cuda.current_stream().cuda_stream
    coef = torch.randn(2, B * L * N, dtype=torch.float32, device="cuda")
    gx, gy, gU = torch.empty_like(x), torch.empty_like(y), torch.empty_like(U)
    ptrs = (x.data_ptr(), y.data_ptr(), U.data_ptr(), coef[0].data_ptr(), coef[1].data_ptr())
    if d == 3:
        def dirs():
            _lib.check(lib.shw_ssw_backward_dirs(*ptrs, B, N, N, L, L * 6, 1.0 / L, None, None, gU.data_ptr(), stream),
                       "shw_ssw_backward_dirs")

        def points():
            _lib.check(lib.shw_ssw_backward_points(*ptrs, B, N, N, L, L * 6, 1.0 / L, None, None, gx.data_ptr(),
                                                   gy.data_ptr(), stream), "shw_ssw_backward_points")
    else:
        def dirs():
            _lib.check(lib.shw_ssw_backward_dirs_dim(*ptrs, B, N, N, d, L, L * d * 2, 1.0 / L, None, None, gU.data_ptr(),
                                                     stream), "shw_ssw_backward_dirs_dim")

        def points():
            _lib.check(lib.shw_ssw_backward_points_dim(*ptrs, B, N, N, d, L, L * d * 2, 1.0 / L, None, None,
                                                       gx.data_ptr(), gy.data_ptr(), stream), "shw_ssw_backward_points_dim")
    out = {"coefficient_bytes": 4 * B * L * 2 * N, "frame_kernel": measure(dirs), "point_kernel": measure(points)}
    out["frame_over_point_kernel"] = out["frame_kernel"]["median_ms"] / out["point_kernel"]["median_ms"]
    out["frame_kernel_TB_per_s"] = out["coefficient_bytes"] / out["frame_kernel"]["median_ms"] / 1e9
    return out


def training_steps(d):
    x, y, U = inputs(d)

    def step(clouds, frames):
        xg = x.clone().requires_grad_(clouds)
        Ug = U.clone().requires_grad_(frames)

        def run():
            xg.grad = None
            Ug.grad = None
            shw.sliced_cost(xg, y, Ug, p=P).backward()
        return measure(run)
    out = {"clouds_only": step(True, False), "frames_only": step(False, True), "both": step(True, True)}
    ssw.SSWWorkspace.clear()
    torch.cuda.empty_cache()
    return out


def composed_step():
    """What a caller composed before: coordinates in eager torch, the circle-level op, autograd to the frames."""
    x, y, U = inputs(3)
    Ug = U.clone().requires_grad_(True)

    def coords(X):
        planar = torch.einsum("bldk,bnd->blnk", Ug, X)
        return (torch.atan2(-planar[..., 1], -planar[..., 0]) + math.pi) / (2 * math.pi)

    def run():
        Ug.grad = None
        cs, ct = coords(x).reshape(B * L, N), coords(y).reshape(B * L, N)
        (shw.binary_search_circle(cs, ct, p=P).view(B, L).mean(1).sum()).backward()
    out = measure(run)
    torch.cuda.empty_cache()
    return out


def max_sliced_latency():
    g = torch.Generator().manual_seed(1)
    x = torch.nn.functional.normalize(torch.randn(1200, 3, generator=g), dim=-1).cuda()
    y = torch.randn(1200, 3, generator=g)
    y[:, 0] += 1.5
    y = torch.nn.functional.normalize(y, dim=-1).cuda()
    xg = x.clone().requires_grad_(True)

    def call():
        xg.grad = None
        shw.max_sliced_wasserstein_sphere(xg, y, num_projections=1, p=P, max_iter=10).backward()
    for _ in range(3):
        call()
    torch.cuda.synchronize()
    times = []
    for _ in range(5):
        t0 = time.perf_counter()
        for _ in range(10):
            call()
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) / 10 * 1e3)
    return {"host_clock_ms_per_call_median": statistics.median(times), "min_ms": min(times), "max_ms": max(times),
            "what": "forward (10 Adam ascent steps + final loss) and backward to the source cloud, one pair, 1200 points"}


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "r21_ssw_dirs_time.json")
    assert torch.cuda.is_available(), "needs a HIP device"
    result = {"device": torch.cuda.get_device_name(0), "B": B, "N": N, "L": L, "p": P, "warmup": WARMUP, "repeats": REPEATS}
    for d in (3, 8, 64):
        entry = {"kernels_alone": kernels_alone(d), "training_step": training_steps(d)}
        result[f"d{d}"] = entry
        print(f"d{d}", json.dumps(entry), flush=True)
    result["composed_eager_step_frames_only"] = composed_step()
    result["composed_over_fused_frames_only"] = (result["composed_eager_step_frames_only"]["median_ms"]
                                                 / result["d3"]["training_step"]["frames_only"]["median_ms"])
    print("composed", json.dumps(result["composed_eager_step_frames_only"]), result["composed_over_fused_frames_only"], flush=True)
    result["max_sliced_wasserstein_sphere_notebook_shape"] = max_sliced_latency()
    print("max_sliced", json.dumps(result["max_sliced_wasserstein_sphere_notebook_shape"]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as fh:
        json.dump(result, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
