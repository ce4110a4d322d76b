"""The circle coordinate of the float32 kernels on the device (`-m gpu`): csrc/ssw_common.hpp, circle_coord, the form
in turns with the select-free octant fold (tests/test_circle_coord_cpu.py restates it and checks it on the CPU).

a. test_crafted_points: shw.circle_coordinates at d = 3 with the frame [[1,0],[0,1],[0,0]], so that (a, b) = (x, y) of
   the point exactly (the projection is an FMA chain from +0: a zero sum is +0 whatever the signs of the inputs' zeros).
   4096 crafted points: every octant, both sides of the eight seams one ulp away and closer, the axes, the four signed
   zeros, |a|, |b| in {1e-38, 1e-30}.  Range [0, 1]; the axis and zero values exactly; the error against float64 atan2
   no larger than PARENT_MAX_ERR, the largest error of the three-reflection form this one replaced, measured on the
   device on the same 4096 points (the device's reciprocal is 1 ulp, so the CPU figure of the restatement is not the
   bound).  Points whose larger component is below the 1e-37 clamp have no resolved angle (both forms: the comment of
   circle_coord); for them the test asks the range and the right quadrant only, and they do not enter the error.

b. / c. test_seam_clouds: one pair, L = 4, n = m = 2048 (one wave, full class), 512 (two waves, full class) and 600 (a
   class with pads), p = 2 and 3.  Both clouds hold only points that project onto the seams and axes of every slice:
   (x, y) in {0, +-2^-j} (axes and diagonals of the plane z = 0, lifted to the unit sphere with z > 0) and the pole, with
   the frames R(phi) [[1,0],[0,1],[0,0]], phi = 0, 45, 225, 270 degrees.  The 45-degree frames hold fl(sqrt(1/2)), and a
   power of two times it is exact, so every projection is exact in float32 and in float64: each point sits ON a seam, an
   axis, or the origin of every slice.  Per-slice costs within 2e-5 relative of oracle/ref_mirror.per_slice_costs, the
   shifts equal to the oracle's, and the cloud against its own permutation costs exactly 0.0 at shift 0: the sort sees keys
   in [0, 1] and orders them.  The oracle's shift (oracle/exact_shift, all 2 n + 1 shifts in float64) is a SET here: atoms
   on the lattice of eighths make the slope of the cost in the cut an even multiple of 1 / (64 n) at p = 2 (eight
   boundaries, each an odd multiple), so it passes through zero and a run of neighbouring shifts (up to thirteen in these
   cases) shares the minimum to 1e-15; the test takes the shifts within 1e-9 relative of the minimum as the oracle's answer, asserts that every
   other shift costs at least 5e-4 relative more (25 x the tolerance of the costs), and asks the kernel for one of them.
"""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

# Largest |coordinate - float64 atan2| of the parent library (three dependent reflections, angle in radians) on the
# resolved points of crafted_points(), measured on an MI355X: 9.772985e-08, at (a, b) = (1399.4806, -208.69495); the form
# in turns measured 4.97e-08 in the same visit (profiles/r15_forward_summary.txt).
PARENT_MAX_ERR = 9.773e-08


@pytest.fixture(scope="module")
def shw():
    import shw_amd
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    shw_amd._lib.load()
    return shw_amd


FRAME = np.array([[1, 0], [0, 1], [0, 0]], dtype=np.float32)
P0, N0 = np.float32(0.0), np.float32(-0.0)


def truth(a, b):
    return (np.arctan2(-b.astype(np.float64), -a.astype(np.float64)) + np.pi) / (2 * np.pi)


@functools.lru_cache(maxsize=None)
def crafted_points():
    """(x, y) float32, 4096 each, and the number of leading points whose values are known exactly."""
    rng = np.random.default_rng(1504)
    xs, ys = [], []

    def add(x, y):
        xs.append(np.asarray(x, dtype=np.float32).ravel())
        ys.append(np.asarray(y, dtype=np.float32).ravel())

    mags = np.array([1.0, 0.37, 3.0, 2.0 ** -20, 1e-30, 1e-38, 1e30, 1.1754944e-38], dtype=np.float32)
    # the four signed zeros and the axes (either zero beside either sign of the other component): exact values
    add([P0, N0, N0, P0], [P0, P0, N0, N0])
    for z in (P0, N0):
        for s in (1, -1):
            add(s * mags, np.full(mags.size, z))
            add(np.full(mags.size, z), s * mags)
    exact = sum(v.size for v in xs)
    # |a|, |b| in {1e-38, 1e-30}, every sign
    for ma in (1e-38, 1e-30):
        for mb in (1e-38, 1e-30):
            add([ma, -ma, -ma, ma], [mb, mb, -mb, -mb])
    # the diagonals: |b| = |a| and one / two ulps to either side, every quadrant
    for m in np.array([1.0, 0.37, 3.0, 0.70710678, 2.0 ** -20, 1e-30, 1e30, 1.9999999], dtype=np.float32):
        near = [m]
        for _ in range(2):
            near = [np.nextafter(near[0], np.float32(0))] + near + [np.nextafter(near[-1], np.float32(np.inf))]
        near = np.array(near, dtype=np.float32)
        for sa in (1, -1):
            for sb in (1, -1):
                add(np.full(near.size, sa * m), sb * near)
                add(sa * near, np.full(near.size, sb * m))
    # the axes one step away: the other component the smallest denormal, a denormal, tiny normals, one ulp of the large one
    for m in np.array([1.0, 0.37, 3.0, 2.0 ** -20], dtype=np.float32):
        small = np.array([1e-45, 1e-40, 1.1754944e-38, 1e-30, float(m) * 2.0 ** -24, float(m) * 2.0 ** -23,
                          float(m) * 1e-4], dtype=np.float32)
        for sa in (1, -1):
            for sb in (1, -1):
                add(np.full(small.size, sa * m), sb * small)
                add(sa * small, np.full(small.size, sb * m))
    # every octant: angles within 1e-6 rad of the seams, then anywhere, at radii over twelve decades
    have = sum(v.size for v in xs)
    count = (4096 - have) // 2
    for spread, cnt in ((1e-6, count), (np.pi / 8, 4096 - have - count)):
        ang = rng.integers(0, 8, cnt) * (np.pi / 4) + rng.uniform(-spread, spread, cnt)
        rad = np.exp(rng.uniform(np.log(1e-6), np.log(1e6), cnt))
        add(rad * np.cos(ang), rad * np.sin(ang))
    x, y = np.concatenate(xs), np.concatenate(ys)
    assert x.size == 4096 and y.size == 4096
    return x, y, exact


def projected(v):
    """fma(v, 1, +0) and the zero terms that follow: -0 becomes +0, everything else is itself."""
    return (v + P0).astype(np.float32)


def coordinate_errors(shw):
    """(got, a, b, resolved, error on the resolved points): the device's coordinates of the crafted points."""
    x, y, _ = crafted_points()
    pts = torch.from_numpy(np.stack([x, y, np.zeros_like(x)], axis=1))
    got = shw.circle_coordinates(pts.cuda(), torch.from_numpy(FRAME[None]).cuda())
    assert tuple(got.shape) == (1, 4096) and got.dtype == torch.float32
    got = got[0].cpu().numpy()
    a, b = projected(x), projected(y)
    resolved = np.maximum(np.abs(a), np.abs(b)) >= np.float32(1e-37)
    err = np.abs(got.astype(np.float64) - truth(a, b))
    return got, a, b, resolved, err


def test_crafted_points(shw):
    x, y, exact = crafted_points()
    got, a, b, resolved, err = coordinate_errors(shw)
    octant = np.floor(truth(a, b) * 8).astype(np.int64) % 8
    assert np.unique(octant[resolved & (a != 0) & (b != 0)]).size == 8
    assert np.all((got >= 0.0) & (got <= 1.0))
    # exact values: zeros and axes.  (a, b) is never -0 here (the projection starts from +0), so b = 0 beside a > 0 is
    # coordinate 0, not 1, and a zero point is coordinate 0; the +-0 table of circle_coord itself is the CPU test's.
    want = truth(a[:exact], b[:exact])
    keep = resolved[:exact] | ((a[:exact] == 0) & (b[:exact] == 0)) | (a[:exact] == 0) | (b[:exact] == 0)
    assert keep.all()
    assert set(np.unique(want)) == {0.0, 0.25, 0.5, 0.75}
    assert np.array_equal(got[:exact].astype(np.float64), want), np.nonzero(got[:exact] != want)[0][:10]
    assert not np.signbit(got[:exact]).any()
    # unresolved points (both components below the clamp): the right quadrant, ends included
    quad = np.floor(truth(a[~resolved], b[~resolved]) * 4) / 4
    assert (~resolved).sum() >= 4
    assert np.all((got[~resolved] >= quad) & (got[~resolved] <= quad + 0.25))
    worst = float(err[resolved].max())
    at = int(np.argmax(np.where(resolved, err, 0)))
    print(f"largest error against float64 on {int(resolved.sum())} resolved points: {worst:.4e} at (a, b) = "
          f"({a[at]!r}, {b[at]!r}); rms {float(np.sqrt((err[resolved] ** 2).mean())):.3e}; bound {PARENT_MAX_ERR}")
    assert worst <= PARENT_MAX_ERR, worst


# ---- b, c -------------------------------------------------------------------------------------------------------------
C = np.float32(np.sqrt(0.5))
ANGLES = (0, 45, 225, 270)


def seam_frames():
    unit = {0: (1.0, 0.0), 45: (C, C), 90: (0.0, 1.0), 135: (-C, C), 180: (-1.0, 0.0), 225: (-C, -C), 270: (0.0, -1.0),
            315: (C, -C)}
    out = []
    for phi in ANGLES:
        cs, sn = unit[phi]
        f = np.array([[cs, -sn], [sn, cs], [0.0, 0.0]], dtype=np.float32) + P0      # (+ 0: no -0 entries)
        out.append(f)
    return np.stack(out)


def seam_point_set():
    """Points (x, y, z): x, y in {0, +-2^-j}, z > 0 completing the unit sphere, and the pole: 49 points."""
    pts = [(0.0, 0.0, 1.0)]
    for j in range(4):
        h = 2.0 ** -j
        for sx, sy in ((1, 0), (-1, 0), (0, 1), (0, -1)):
            pts.append((sx * h, sy * h, np.sqrt(max(1.0 - h * h, 0.0)) if j else 2.0 ** -12))
        if j:
            for sx in (1, -1):
                for sy in (1, -1):
                    pts.append((sx * h, sy * h, np.sqrt(1.0 - 2 * h * h)))
    return np.array(pts, dtype=np.float32)


def seam_cloud(rng, n, skew):
    """n points of the set, with multiplicities that differ from cloud to cloud (`skew` tilts them) so that the
    transport has work to do."""
    base = seam_point_set()
    w = rng.random(base.shape[0]) + skew * (base[:, 0] > 0) + 0.5 * skew * (base[:, 1] < 0)
    idx = rng.choice(base.shape[0], size=n, p=w / w.sum())
    return base[idx]


@functools.lru_cache(maxsize=None)
def seam_case(n, p):
    """Clouds, frames and the oracle's answers for one (n, p): computed once, never changed."""
    from oracle import exact_shift, ref_mirror
    rng = np.random.default_rng(1505 + n)
    x, y = seam_cloud(rng, n, 0.0), seam_cloud(rng, n, 1.5)
    U = seam_frames()
    # every projection is exact: the float32 FMA chain and float64 agree to the bit, and land on seams, axes or (0, 0)
    for pts in (x, y):
        for f in U:
            a64, b64 = pts.astype(np.float64) @ f[:, 0].astype(np.float64), pts.astype(np.float64) @ f[:, 1].astype(np.float64)
            assert np.array_equal(a64.astype(np.float32).astype(np.float64), a64)
            assert np.array_equal(b64.astype(np.float32).astype(np.float64), b64)
            assert not np.signbit(a64[a64 == 0]).any() and not np.signbit(b64[b64 == 0]).any()
            assert np.all((a64 == 0) | (b64 == 0) | (np.abs(a64) == np.abs(b64)))
    cu, cv = exact_shift.circle_coords(x, U), exact_shift.circle_coords(y, U)
    eighths = np.arange(8) / 8
    assert np.abs(cu[..., None] - eighths).min(axis=-1).max() < 1e-15           # multiples of 1/8, 1 itself not among them
    best, optimal = np.empty(len(U)), []
    for l in range(len(U)):
        ks, c = exact_shift.shift_costs(np.sort(cu[l]), np.sort(cv[l]), p)
        best[l] = c.min()
        tied = c <= best[l] * (1 + 1e-9)
        assert best[l] > 0 and c[~tied].min() - best[l] > 5e-4 * best[l], (n, p, l, np.sort(c)[:5])
        optimal.append(set(int(k) for k in ks[tied]))
    ref = ref_mirror.per_slice_costs(torch.from_numpy(x), torch.from_numpy(y), torch.from_numpy(U), p=p).numpy()
    assert np.abs(ref - best).max() <= 1e-5 * best.min(), (ref, best)             # the two oracles agree
    perm = rng.permutation(n)
    return x, y, U, ref.astype(np.float64), optimal, perm, cu


@pytest.mark.parametrize("p", [2, 3])
@pytest.mark.parametrize("n", [2048, 512, 600])
def test_seam_clouds(shw, n, p):
    x, y, U, ref, optimal, perm, cu = seam_case(n, p)
    xd, yd, Ud = (torch.from_numpy(v).cuda() for v in (x, y, U))
    coords = shw.circle_coordinates(xd, Ud).cpu().numpy()
    assert coords.shape == (4, n)
    assert np.abs(coords.astype(np.float64) - cu).max() <= 2.0 ** -24, np.abs(coords - cu).max()   # ON the seams, no wrap to 1
    _, cost, shift = shw.ssw_pair_losses(xd[None], yd[None], Ud, p=p, return_slices=True)
    cost, shift = cost[0].cpu().numpy().astype(np.float64), shift[0].cpu().numpy()
    err = np.abs(cost - ref) / ref
    print(f"n={n} p={p}: per-slice costs {cost}, largest relative error {err.max():.3e}; shifts {shift} (oracle {optimal})")
    assert err.max() <= 2e-5, (cost, ref)
    assert all(int(k) in ok for k, ok in zip(shift, optimal)), (shift, optimal)
    twin = torch.from_numpy(np.ascontiguousarray(x[perm])).cuda()
    _, cost0, shift0 = shw.ssw_pair_losses(xd[None], twin[None], Ud, p=p, return_slices=True)
    assert (cost0.cpu().numpy() == 0.0).all(), cost0
    assert (shift0.cpu().numpy() == 0).all(), shift0
