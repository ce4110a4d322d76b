"""Timing of the notebooks' ASWD baseline and of the D-generic Euclidean sliced-W kernels.

    step     the notebook's ASWD outer step (Flow_cube.ipynb, the ASWD branch of the flow loop): N = 1200, L = 100,
             phi = Mapping(3) (D' = 6), max_iter = 10, loss.backward() and the Adam step on the evolving cloud, eager;
             host clock around steps that end in a device synchronise.
    kernels  the forward (with coefficient rows) and both backward kernels at D = 3 (the R^3 entries and the D-generic
             entry), 6 and 21, at (B, n, L) = (1, 1200, 100) and (64, 2048, 512), REPS launches each: run it under
             `rocprofv3 --kernel-trace --stats` and read the kernel table (esw_kernel* / esw_dim_kernel*, ...).
             The stats table sums by kernel name, so profile one configuration per run: kernels B n L D r3|dim.
usage: python tools/aswd_time.py step [out.json]
       python tools/aswd_time.py kernels [B n L D r3|dim]"""
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import shw_amd as shw  # noqa: E402

mode = sys.argv[1] if len(sys.argv) > 1 else "step"
out_path = sys.argv[2] if mode == "step" and len(sys.argv) > 2 else None
CONFIGS = [(B, n, L, D, entry) for B, n, L in ((1, 1200, 100), (64, 2048, 512))
           for D, entry in ((3, "r3"), (3, "dim"), (6, "dim"), (21, "dim"))]
if mode == "kernels" and len(sys.argv) > 2:
    CONFIGS = [tuple(int(v) for v in sys.argv[2:6]) + (sys.argv[6],)]
REPS = 20


class Mapping(torch.nn.Module):
    def __init__(self, size):
        super().__init__()
        self.net = torch.nn.Sequential(torch.nn.Linear(size, size))

    def forward(self, inputs):
        return torch.cat((inputs, self.net(inputs)), dim=-1)


def time_step(steps=40, warmup=5):
    g = torch.Generator().manual_seed(0)
    target = (torch.rand(1200, 3, generator=g) * 2 - 1).cuda()
    evolving = (torch.rand(1200, 3, generator=g) * 2 - 1).cuda().requires_grad_(True)
    lam = 0.05 / target.abs().mean()
    optimizer = torch.optim.Adam([evolving], lr=0.01, betas=(0.9, 0.999))
    torch.manual_seed(0)
    phi = Mapping(3).cuda()
    phi_op = torch.optim.Adam(phi.parameters(), lr=0.005, betas=(0.999, 0.999))

    def step():
        optimizer.zero_grad()
        loss = shw.augmented_sliced_wassersten_distance(evolving, target, 100, phi, phi_op, p=2, max_iter=10, lam=lam,
                                                        device="cuda", net_type="fc")
        loss.backward(retain_graph=True)
        optimizer.step()
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
    return {"aswd_outer_step_ms": sorted(times)[1], "aswd_outer_step_ms_runs": times, "steps_per_run": steps}


def run_kernels():
    lib = shw._lib.load()
    stream = torch.cuda.current_stream().cuda_stream
    done = []
    for B, n, L, D, entry in CONFIGS:
        g = torch.Generator().manual_seed(D)
        xs = torch.randn(B, n, D, generator=g).cuda()
        xt = (torch.randn(B, n, D, generator=g) * 0.7 + 0.2).cuda()
        th = torch.stack([shw.rand_projections(D, L) for _ in range(B)]).cuda()
        w = torch.ones(B, L, device="cuda")
        sums = torch.empty(B * L, device="cuda")
        cs, ct = torch.empty(B * L * n, device="cuda"), torch.empty(B * L * n, device="cuda")
        gxs, gxt = torch.empty_like(xs), torch.empty_like(xt)
        gth = torch.empty_like(th)
        P = [t.data_ptr() for t in (xs, xt, th, w, sums, cs, ct, gxs, gxt, gth)]
        for _ in range(REPS):
            if entry == "r3":
                rc = (lib.shw_esw_forward(P[0], P[1], P[2], B, n, L, L * D, 2.0, P[4], P[5], P[6], stream)
                      or lib.shw_esw_backward_points(P[2], P[5], P[6], P[3], B, n, L, L * D, P[7], P[8], stream)
                      or lib.shw_esw_backward_dirs(P[0], P[1], P[5], P[6], P[3], B, n, L, P[9], stream))
            else:
                rc = (lib.shw_esw_forward_dim(P[0], P[1], P[2], B, n, D, L, L * D, 2.0, P[4], P[5], P[6], stream)
                      or lib.shw_esw_backward_points_dim(P[2], P[5], P[6], P[3], B, n, D, L, L * D, P[7], P[8],
                                                         stream)
                      or lib.shw_esw_backward_dirs_dim(P[0], P[1], P[5], P[6], P[3], B, n, D, L, P[9], stream))
            assert rc == 0, rc
        torch.cuda.synchronize()
        done.append({"B": B, "n": n, "L": L, "D": D, "entry": entry, "launches": REPS})
        del cs, ct
        torch.cuda.empty_cache()
    return {"kernel_configs": done}


res = {"device": torch.cuda.get_device_name(0)}
if mode == "step":
    res.update(time_step())
if mode == "kernels":
    res.update(run_kernels())
print(json.dumps(res))
if out_path:
    with open(out_path, "w") as fh:
        json.dump(res, fh, indent=1)
