"""Inputs of the general float64 tests (tests/test_f64_general_cpu.py and tests/test_f64_general_gpu.py): seeded double
clouds of two sizes, weights and direction frames, built the same way on both sides so that the CPU file can assert what
the GPU file relies on (isolated minimisers, the rounding spread)."""
import torch

F64 = torch.float64
POWERS = (1, 1.5, 2, 3)
# (n, m): the smallest sizes at which each mechanism can break -- one atom, fewer atoms than lanes, one wave, one atom over
# / under a wave, several waves with the larger cloud second, a non-power-of-two above 1024; the limit is added by the tests
SHAPES = ((1, 1), (1, 5), (7, 5), (64, 48), (65, 63), (200, 256), (1200, 1000))
MANY = ((1, 1), (1, 5), (7, 5))                 # also run with B * L = 1250 > 1024 problems
GRAD_SHAPES = SHAPES[:6]                        # gradients against the definition: up to 200 x 256
WEIGHT_MODES = ("none", "shared", "per_pair")

# The rounding spread S over these cases: worst |minimum with CDFs from a forward cumsum - minimum with CDFs from
# 1 - reversed cumsum of the same weights|.  Two summation orders sample the rounding range of a third (the kernel's
# scan), they do not bound it, hence the margin of 10 in the GPU test.  tests/test_f64_general_cpu.py measures S, prints
# it and asserts it is no larger than this figure (measured: 1.25e-15, at 1200 x 1000).
ROUNDING_SPREAD = 1.5e-15


def unit_cloud(gen, *shape):
    return torch.nn.functional.normalize(torch.randn(*shape, 3, generator=gen, dtype=F64), dim=-1)


def frames(gen, *shape):
    return torch.linalg.qr(torch.randn(*shape, 3, 2, generator=gen, dtype=F64))[0]


def weights(gen, *shape):
    w = torch.rand(*shape, generator=gen, dtype=F64) + 0.25
    return w / w.sum(-1, keepdim=True)


def seed_of(n, m, p, mode, many=False):
    return 14100 + 7 * n + 3 * m + int(10 * p) + 1000 * WEIGHT_MODES.index(mode) + (50000 if many else 0)


def case(n, m, p, mode, many=False):
    """-> x (B, n, 3), y (B, m, 3), U, wu, wv.  B * L = 6, or 1250 with `many`; per-pair directions (B, L, 3, 2) for the
    shared weights and shared ones (L, 3, 2) otherwise; weights None, (n,) / (m,) or (B, n) / (B, m)."""
    g = torch.Generator().manual_seed(seed_of(n, m, p, mode, many))
    B, L = (5, 250) if many else (2, 3)
    x, y = unit_cloud(g, B, n), unit_cloud(g, B, m)
    U = frames(g, B, L) if mode == "shared" else frames(g, L)
    if mode == "none":
        return x, y, U, None, None
    if mode == "shared":
        return x, y, U, weights(g, n), weights(g, m)
    return x, y, U, weights(g, B, n), weights(g, B, m)


def modes_for(n, m):
    return WEIGHT_MODES if n != m else WEIGHT_MODES[1:]          # uniform equal sizes belong to the other kernels


# ---- gradcheck inputs: margins that keep a finite-difference step of 1e-6 on one smooth piece ----------------------
GRADCHECK_SEED, GRADCHECK_ROWS_SEED = 14501, 14502    # seeds for which the margins below hold (asserted on both sides)


def gradcheck_clouds(seed):
    """x (2, 12, 3), y (2, 9, 3), U (2, 3, 3, 2), wu (12,), wv (9,)."""
    g = torch.Generator().manual_seed(seed)
    return unit_cloud(g, 2, 12), unit_cloud(g, 2, 9), frames(g, 2, 3), weights(g, 12), weights(g, 9)


def gradcheck_rows(seed):
    """u (3, 10), v (3, 8), wu (10,), wv (8,)."""
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(3, 10, generator=g, dtype=F64), torch.rand(3, 8, generator=g, dtype=F64), weights(g, 10),
            weights(g, 8))


def gradcheck_rows_margins_ok(u, v, wu, wv, p):
    """Merged coordinates more than 1e-5 apart and away from the seam; p != 1: an isolated minimiser with both one-sided
    slopes above 1e-4; p == 1: the cumulated gap weights more than 1e-4 away from the median threshold 0.5."""
    from helpers import circle_general_exact as exact
    from oracle import ref_mirror
    merged = torch.sort(torch.cat([u, v, torch.zeros_like(u[:, :1]), torch.ones_like(u[:, :1])], -1), -1)[0]
    if not bool((torch.diff(merged, dim=-1) > 1e-5).all()):
        return False
    us, vs, cu, cv = exact.sorted_cdfs(u, v, wu, wv)
    if p != 1:
        _, theta = exact.minimise(us, vs, cu, cv, p)
        t = theta.reshape(-1, 1)
        left, _ = ref_mirror.cut_slopes(t - exact.SLOPE_PROBE, us, vs, cu, cv, p)
        _, right = ref_mirror.cut_slopes(t + exact.SLOPE_PROBE, us, vs, cu, cv, p)
        return bool(exact.isolated(theta, us, vs, cu, cv, p).all()) and bool((left < -1e-4).all()) and bool((right > 1e-4).all())
    R, n = u.shape
    gu, gv = torch.gather(wu.expand(R, -1), 1, torch.sort(u, -1)[1]), torch.gather(wv.expand(R, -1), 1, torch.sort(v, -1)[1])
    vals, order = torch.sort(torch.cat([us, vs], -1), dim=-1, stable=True)
    level = torch.cumsum(torch.gather(torch.cat([gu, -gv], -1), 1, order), -1)
    gaps = torch.diff(vals, dim=-1, append=torch.ones_like(vals[:, :1]))
    acc = torch.cumsum(torch.gather(gaps, 1, torch.sort(level, dim=-1, stable=True)[1]), -1)
    return bool(((acc - 0.5).abs() > 1e-4).all())


def gradcheck_margins_ok(x, y, U, wu, wv, p):
    from oracle import ref_mirror
    return all(gradcheck_rows_margins_ok(ref_mirror.circle_coords(x[b], U[b]), ref_mirror.circle_coords(y[b], U[b]), wu, wv, p)
               for b in range(x.shape[0]))
