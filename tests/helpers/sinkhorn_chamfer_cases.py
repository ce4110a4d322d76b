"""Seeded inputs and float64 / float32 reference runs shared by tests/test_sinkhorn_chamfer_gpu.py (which compares the
HIP kernels with them) and tests/test_sinkhorn_mirror_cpu.py (which checks, without a GPU, the conditions the GPU tests
rely on: enough ties, a stop that float32 noise cannot move by a sweep, ...).

How every Sinkhorn bound is set: oracle/sinkhorn_mirror.py is run twice on the same float32 inputs, in float64 (the
reference value) and in float32.  The difference of the two runs, g, is the reference's own rounding noise for that
quantity.  A kernel result must lie within bound(g) = max(K g, FLOOR scale) of the float64 run, K = 16: the kernel
recomputes c_ij with FMAs, uses the hardware exp2 / log2 (1 ulp) and accumulates a row sequentially over up to 1025
candidates where torch sums pairwise -- random-walk growth sqrt(1025) ~ 32 against ~ log2(1025) = 10; 16 covers the
ratio.  FLOOR = 8 * 2^-24 (relative) covers the cases where the two mirror runs agree exactly (g = 0)."""
import functools

import numpy as np
import torch

from oracle import sinkhorn_mirror

K = 16
FLOOR = 8 * 2.0 ** -24


def bound(g, scale=1.0, k=K):
    return max(k * g, FLOOR * scale)


def ratio(gap, g, scale=1.0):
    """kernel gap in units of the mirror's own gap (of the floor where that is larger than g): for the messages"""
    return gap / max(g, FLOOR * scale / K)


def unit_cloud(gen, *shape):
    return torch.nn.functional.normalize(torch.randn(*shape, 3, generator=gen), dim=-1)


def lattice_cloud(gen, *shape):
    """coordinates k / 8, k uniform in -8..8: every difference, square and sum of squares is exact in float32"""
    return torch.randint(-8, 9, (*shape, 3), generator=gen).to(torch.float32) / 8


def relmax(a, b):
    a = np.asarray(a, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    return float(np.max(np.abs(a - b) / np.maximum(np.abs(b), 1e-30)))


def of_largest(a, b):
    """max |a - b| in units of the largest |b|"""
    a = np.asarray(a, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300))


# ------------------------------------------------------------------------------------------------ Sinkhorn, forward
FORWARD_SHAPES = [(1, 1), (9, 7), (520, 255), (257, 513), (513, 1025)]
FORWARD_CASES = [(n, m, 0.05, 30) for n, m in FORWARD_SHAPES] + [(257, 513, 0.005, 100)]
P_MIN = 1e-30          # entries of the plan below this are left out of the log P comparison (float32 underflow)


def forward_inputs(n, m, B=3):
    g = torch.Generator().manual_seed(70 + n + m)
    return unit_cloud(g, B, n), unit_cloud(g, B, m) * 0.9 + 0.05


def col_target(m):
    """what a column of P sums to right after a v-pass: the marginal the iteration uses, float32(1/m) + 1e-8"""
    return float(np.float32(1.0) / np.float32(m)) + 1e-8


def plan_gaps(P, cost, ref):
    """gaps of a float32 result (P (B,n,m), cost (B,)) to the float64 run `ref` (see forward_case), as floats"""
    P = np.asarray(P, dtype=np.float64)
    mask = ref["mask"]
    with np.errstate(divide="ignore"):
        logp = np.log(P[mask])
    m = P.shape[-1]
    return {"cost": relmax(cost, ref["cost"]),
            "logP": float(np.abs(logp - ref["logP"]).max()) if mask.any() else 0.0,
            "col": float(np.abs(P.sum(-2) - col_target(m)).max() / col_target(m)),
            "row": relmax(P.sum(-1), ref["row"])}


@functools.lru_cache(maxsize=None)
def forward_case(n, m, eps, iters):
    """inputs, the float64 run, and the float32 run's gaps to it (computed once per session, never modified)"""
    x, y = forward_inputs(n, m)
    cost, P, C, its, _, (u, v) = sinkhorn_mirror.sinkhorn_costs(x.double(), y.double(), eps, iters, history=True)
    P = P.numpy()
    mask = P >= P_MIN
    # log P_ij = (-C_ij + u_i + v_j) / eps: float32 rounds each of the three terms, so the floor of the log P bound is
    # relative to their size and not to the (possibly cancelled) sum
    terms = (C.abs() + u.abs().unsqueeze(-1) + v.abs().unsqueeze(-2)).max().item() / eps
    ref = {"cost": cost.numpy(), "C": C.numpy(), "mask": mask, "logP": np.log(P[mask]), "row": P.sum(-1), "its": its,
           "logP_scale": terms}
    c32, P32, _, its32 = sinkhorn_mirror.sinkhorn_costs(x, y, eps, iters)
    g = plan_gaps(P32.numpy(), c32.numpy(), ref)
    g["its32"] = its32
    return x, y, ref, g


# ------------------------------------------------------------------------------------ Sinkhorn, value and gradients
def mirror_grads(x, y, eps, iters, w, norm_p=2, cost_pow=1, thresh=1e-9, dtype=torch.float64):
    """(cost * w).sum() of the mirror (cost^(1/N) as the N-class returns it) and its gradients by autograd"""
    xd, yd = x.detach().clone().to(dtype).requires_grad_(True), y.detach().clone().to(dtype).requires_grad_(True)
    out = sinkhorn_mirror.sinkhorn_costs(xd, yd, eps, iters, norm_p=norm_p, cost_pow=cost_pow, thresh=thresh, history=True)
    cost = out[0] if cost_pow == 1 else out[0].pow(1.0 / cost_pow)
    (cost * torch.as_tensor(w, dtype=dtype)).sum().backward()
    return {"cost": cost.detach().numpy(), "gx": xd.grad.numpy(), "gy": yd.grad.numpy(), "its": out[3], "stats": out[4]}


def grad_gaps(cost, gx, gy, ref):
    return {"cost": relmax(cost, ref["cost"]), "gx": of_largest(gx, ref["gx"]), "gy": of_largest(gy, ref["gy"])}


def grad_reference(x, y, eps, iters, w, **kw):
    """the float64 run and the float32 run's gaps to it"""
    ref = mirror_grads(x, y, eps, iters, w, dtype=torch.float64, **kw)
    f32 = mirror_grads(x, y, eps, iters, w, dtype=torch.float32, **kw)
    g = grad_gaps(f32["cost"], f32["gx"], f32["gy"], ref)
    g["its32"] = f32["its"]
    g["stats32"] = f32["stats"]
    return ref, g


VARIANTS = {"L1": (1, 1), "L3": (3, 1), "L2_N2": (2, 2), "L2_N3": (2, 3), "L1_N2": (1, 2)}     # tag -> (norm_p, cost_pow)
VARIANT_SHAPE = (257, 513)
VARIANT_W = (1.0, -0.7)


def variant_inputs():
    n, m = VARIANT_SHAPE
    g = torch.Generator().manual_seed(5 * n + m)
    return unit_cloud(g, 2, n), unit_cloud(g, 2, m) * 0.9 + 0.05


@functools.lru_cache(maxsize=None)
def variant_case(tag):
    x, y = variant_inputs()
    norm_p, cost_pow = VARIANTS[tag]
    return (x, y) + grad_reference(x, y, 0.05, 25, VARIANT_W, norm_p=norm_p, cost_pow=cost_pow)


def l1_lattice_inputs():
    g = torch.Generator().manual_seed(64 * 96)
    return lattice_cloud(g, 2, 64), lattice_cloud(g, 2, 96)


@functools.lru_cache(maxsize=None)
def l1_lattice_case():
    x, y = l1_lattice_inputs()
    return (x, y) + grad_reference(x, y, 0.05, 25, VARIANT_W, norm_p=1)


# --------------------------------------------------------------------------------------------- Sinkhorn, early stop
STOP_T = 9
STOP_W = (1.0, -0.7, 0.4)
STOP_CASES = [(3, 40, 300, False), (3, 40, 300, True), (70, 8, 8, False)]       # B, n, m, own_copy


def stop_inputs(B, n, m, own_copy=False):
    g = torch.Generator().manual_seed(7 * n + m)
    x, y = unit_cloud(g, B, n), unit_cloud(g, B, m) * 0.9 + 0.05
    if own_copy:
        y[0, :n] = x[0]          # pair 0 carries a copy of its own source cloud: its statistic decays differently
    if B > 64:
        # the first 64 pairs are small clouds that converge within three sweeps: what holds the batch mean above the
        # threshold until sweep T are the pairs from 64 on, those a single trip of a 64-wide loop over pairs never sees
        x[:64] *= 0.3
        y[:64] *= 0.3
    return x, y


@functools.lru_cache(maxsize=None)
def stop_case(B, n, m, own_copy=False, eps=0.5, max_iter=40):
    """a threshold half way (geometrically) between the float64 statistic after sweeps T - 1 and T, and the
    reference run with it"""
    x, y = stop_inputs(B, n, m, own_copy)
    free = sinkhorn_mirror.sinkhorn_costs(x.double(), y.double(), eps, max_iter, thresh=0.0, history=True)[4]
    thresh = float(np.sqrt(free[STOP_T - 2] * free[STOP_T - 1]))
    w = [STOP_W[b % 3] for b in range(B)]
    ref, g = grad_reference(x, y, eps, max_iter, w, thresh=thresh)
    return x, y, w, thresh, free, ref, g


# -------------------------------------------------------------------------------------------------------- Chamfer
CHAMFER_SHAPES = [(257, 1027), (1029, 2049), (5, 3), (1, 1)]
CHAMFER_W = (1.0, -0.5)
CLUSTERED_SHAPE = (1029, 1027)
TILE, GROUP = 1024, 4


def chamfer_inputs(kind, n, m, B=2):
    g = torch.Generator().manual_seed(11 * n + m)
    if kind == "lattice":
        return lattice_cloud(g, B, n), lattice_cloud(g, B, m)
    if kind == "random":
        return torch.randn(B, n, 3, generator=g), torch.randn(B, m, 3, generator=g) * 0.8 + 0.1
    # clustered: y[b, j0] sits inside the small x cluster, every other y point is far away -- j0 is the nearest
    # neighbour of all n x points, so its gradient row collects n + 1 terms
    x = torch.randn(B, n, 3, generator=g) * 0.05
    y = torch.nn.functional.normalize(torch.randn(B, m, 3, generator=g), dim=-1) * 10
    for b in range(B):
        y[b, 200 + 700 * b] = torch.tensor([0.02, -0.01, 0.03])
    return x, y


def sqdist(x, y, dtype=np.float64):
    x = np.asarray(x, dtype=dtype)
    y = np.asarray(y, dtype=dtype)
    d = np.zeros((x.shape[0], x.shape[1], y.shape[1]), dtype=dtype)
    for k in range(3):
        d += (x[:, :, None, k] - y[:, None, :, k]) ** 2
    return d


@functools.lru_cache(maxsize=None)
def chamfer_case(kind, n, m):
    x, y = chamfer_inputs(kind, n, m)
    d = sqdist(x.numpy(), y.numpy())
    ref = {"d": d, "nn_xy": d.argmin(2), "nn_yx": d.argmin(1), "min_xy": d.min(2), "min_yx": d.min(1)}
    ref["pair"] = ref["min_xy"].mean(1) + ref["min_yx"].mean(1)
    return x, y, ref


def tie_counts(d):
    """d (B, queries, candidates): (queries, tied queries, tied with the first two minimisers in different groups of four,
    tied with them in different 1024-candidate tiles)"""
    best = d.min(-1, keepdims=True)
    hit = d == best
    tied = hit.sum(-1) >= 2
    first = hit.argmax(-1)
    rest = hit.copy()
    np.put_along_axis(rest, first[..., None], False, axis=-1)
    second = rest.argmax(-1)
    groups = tied & (first // GROUP != second // GROUP)
    tiles = tied & (first // TILE != second // TILE)
    return tied.size, int(tied.sum()), int(groups.sum()), int(tiles.sum())


def chamfer_grads(x, y, nn_xy, nn_yx, w, dtype):
    """autograd of the definition sum_b w_b [mean_i |x_i - y_nn(i)|^2 + mean_j |x_nn(j) - y_j|^2] with the float64 argmin
    made explicit (first minimum): torch.cdist(...).min() leaves the choice among tied candidates to rounding"""
    xd, yd = x.detach().clone().to(dtype).requires_grad_(True), y.detach().clone().to(dtype).requires_grad_(True)
    ixy = torch.as_tensor(nn_xy)[..., None].expand(-1, -1, 3)
    iyx = torch.as_tensor(nn_yx)[..., None].expand(-1, -1, 3)
    pair = ((xd - yd.gather(1, ixy)) ** 2).sum(-1).mean(1) + ((xd.gather(1, iyx) - yd) ** 2).sum(-1).mean(1)
    (pair * torch.as_tensor(w, dtype=dtype)).sum().backward()
    return xd.grad.numpy(), yd.grad.numpy()


@functools.lru_cache(maxsize=None)
def chamfer_grad_case(kind, n, m):
    x, y, ref = chamfer_case(kind, n, m)
    gx, gy = chamfer_grads(x, y, ref["nn_xy"], ref["nn_yx"], CHAMFER_W, torch.float64)
    fx, fy = chamfer_grads(x, y, ref["nn_xy"], ref["nn_yx"], CHAMFER_W, torch.float32)
    return x, y, ref, (gx, gy), (of_largest(fx, gx), of_largest(fy, gy))
