"""The loss kernels' distribution sort with the byte-offset bin map (csrc/bin_sort.hpp) on the GPU (`-m gpu`, MI355X).

The map must order every key exactly: a key counted into a wrong bin, or a bin map that is not monotone, leaves the
sorted arrays out of order and the slice cost wrong.  Two ways in:

  * projection mode (clouds on the sphere), one size per code path: 2048 (one wave per slice, full class) and 512 (two
    waves, 8 keys per lane, the smallest binned class) take the byte-offset map and the scalar-base point loads; 2001 (two
    waves, masked 32-keys-per-lane class with pads; odd n, so the clouds of successive pairs start 12 n bytes apart) and
    1200 (20 keys per lane, 768 bins) take the saturating map the classes with pads keep;
  * coordinate-row mode (shw.binary_search_circle): the caller supplies the numbers, so the rows are built to sit on the
    map's edges -- and, in a second test, to leave its domain [0, 1], which the kernel must still sort exactly.

Every launch has more than 1024 (pair, slice) problems: fewer take the small-grid kernels, which do not use this sort.
The expected values are the exhaustive float64 argmin over the shifts (oracle/exact_shift.py).
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

B, L = 3, 384                  # 1152 (pair, slice) problems: more than the small-grid limit of 1024
CHECKED = [(b, l) for b in range(B) for l in (0, 97, 191, 300, 383)]
ROWS, N = 1104, 2048
TOL = 2e-5                     # p = 2, as tests/test_shift_search_gpu.py
WINDOW = 12                    # shifts k0 - 12 .. k0 + 12 evaluated for every row (see windowed_min)


@pytest.fixture(scope="module")
def shw():
    import shw_amd
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    shw_amd._lib.load()
    return shw_amd


def unit_cloud(gen, n):
    return torch.nn.functional.normalize(torch.randn(n, 3, generator=gen), dim=-1)


@pytest.mark.parametrize("n", [2048, 2001, 1200, 512])
def test_projection_mode_matches_exact_shift(shw, n):
    from oracle import exact_shift
    g = torch.Generator().manual_seed(6100 + n)
    x = torch.stack([unit_cloud(g, n) for _ in range(B)])
    y = torch.stack([unit_cloud(g, n) for _ in range(B)])
    U = torch.linalg.qr(torch.randn(B, L, 3, 2, generator=g))[0]
    _, cost, shift = shw.ssw_pair_losses(x.cuda(), y.cuda(), U.cuda(), p=2, return_slices=True)
    cost, shift = cost.cpu().numpy(), shift.cpu().numpy()
    assert np.isfinite(cost).all()
    for b, l in CHECKED:
        cu = exact_shift.circle_coords(x[b].numpy(), U[b, l:l + 1].numpy())[0]
        cv = exact_shift.circle_coords(y[b].numpy(), U[b, l:l + 1].numpy())[0]
        ks, c = exact_shift.shift_costs(np.sort(cu), np.sort(cv), 2)
        j = int(np.argmin(c))
        print(f"n={n} (b,l)=({b},{l}) cost {cost[b, l]:.9e} exact {c[j]:.9e} rel {abs(cost[b, l] - c[j]) / c[j]:.2e} "
              f"shift {int(shift[b, l])} exact {int(ks[j])}")
        assert abs(cost[b, l] - c[j]) <= TOL * c[j], (b, l, cost[b, l], c[j])
        k = int(shift[b, l])
        assert -n <= k <= n, (b, l, k)
        # the same shift, or one whose exact cost ties with the minimum to fp32 accuracy
        assert k == ks[j] or c[k + n] <= c[j] * (1 + TOL), (b, l, k, int(ks[j]), c[k + n], c[j])


# ---------------------------------------------------------------------------------------------------------------------
# coordinate-row mode
# ---------------------------------------------------------------------------------------------------------------------
def edge_rows(seed, rows=ROWS, n=N, outside=0):
    """(rows, n) float32 coordinates in [0, 1] that sit on the edges of the bin maps: multiples of 1/1024 (the edges of
    floor(1024 key)) and of 1/4095 (the rounding points of the byte-offset map) with the floats just below and above
    them, 0.0, -0.0, 1.0 and the float below 1, a block of 30 equal values (under the 40-run limit of the distribution
    sort) and, in every eighth row, a block of 64 equal values (over it: that row sorts with the network).  With
    `outside` > 0 that many values of every row lie in [-0.5, 0) or (1, 1.5]."""
    rng = np.random.default_rng(seed)
    one, zero = np.float32(1), np.float32(0)
    out = rng.random((rows, n), dtype=np.float32)
    for r in range(rows):
        a = rng.choice(1025, 180, replace=False).astype(np.float32) / np.float32(1024)
        b = rng.choice(4096, 180, replace=False).astype(np.float32) / np.float32(4095)
        g = np.concatenate([a, b])
        g = np.concatenate([g, np.nextafter(g, np.float32(-1)), np.nextafter(g, np.float32(2))])
        g = g[(g >= 0) & (g <= 1)]
        special = np.array([0.0, -0.0, 1.0, np.nextafter(one, zero)], dtype=np.float32)
        block = [np.full(30, rng.random(dtype=np.float32), dtype=np.float32)]
        if r % 8 == 3:
            block.append(np.full(64, rng.random(dtype=np.float32), dtype=np.float32))
        if outside:
            lo = -rng.random(outside // 2, dtype=np.float32) * np.float32(0.5) - np.float32(1e-6)
            hi = one + np.float32(1e-6) + rng.random(outside - outside // 2, dtype=np.float32) * np.float32(0.4999)
            block += [lo.astype(np.float32), hi.astype(np.float32)]
        fixed = np.concatenate([g, special] + block)
        assert fixed.size < n
        out[r, :fixed.size] = fixed
        out[r] = out[r, rng.permutation(n)]
    return out


def windowed_min(u, v):
    """min over k in [k0 - WINDOW, k0 + WINDOW], k0 = round(sum u - sum v) (the kernels' first guess), of
    c(k) = mean_i |u_(i) - v_ext(i + k)|^2 for every row, in float64, with the argmin and its distance from k0.
    c is convex in k (ssw_common.hpp), so a minimum strictly inside the window is the minimum over all shifts -- which the
    caller checks, and confirms against exact_shift's exhaustive search on some rows."""
    us, vs = np.sort(u.astype(np.float64), axis=1), np.sort(v.astype(np.float64), axis=1)
    rows, n = us.shape
    i = np.arange(n)
    k0 = np.rint(us.sum(axis=1) - vs.sum(axis=1)).astype(np.int64)
    ds = np.arange(-WINDOW, WINDOW + 1)
    c = np.empty((ds.size, rows))
    for t, d in enumerate(ds):
        q = i[None, :] + (k0 + d)[:, None]
        v_ext = np.take_along_axis(vs, np.mod(q, n), axis=1) + np.floor_divide(q, n)
        c[t] = ((us - v_ext) ** 2).mean(axis=1)
    j = c.argmin(axis=0)
    return c[j, np.arange(rows)], k0 + ds[j], ds[j]


def check_rows(shw, u, v, exhaustive_rows):
    from oracle import exact_shift
    got = shw.binary_search_circle(torch.from_numpy(u).cuda(), torch.from_numpy(v).cuda(), p=2).cpu().numpy()
    want, k, d = windowed_min(u, v)
    assert (np.abs(d) < WINDOW).all(), "a minimum on the rim of the window is not known to be the global one"
    for r in exhaustive_rows:                                     # the oracle itself, every shift
        ks, c = exact_shift.shift_costs(np.sort(u[r].astype(np.float64)), np.sort(v[r].astype(np.float64)), 2)
        assert abs(c.min() - want[r]) <= 1e-12 * want[r] and ks[int(np.argmin(c))] == k[r], (r, c.min(), want[r])
    rel = np.abs(got - want) / want
    print(f"rows {u.shape[0]}: largest relative error {rel.max():.3e} (row {int(rel.argmax())}), median {np.median(rel):.3e}")
    assert np.isfinite(got).all()
    bad = np.nonzero(rel > TOL)[0]
    assert bad.size == 0, (bad[:10], got[bad[:10]], want[bad[:10]])


def test_rows_on_the_edges_of_the_map(shw):
    u, v = edge_rows(71), edge_rows(72)
    assert u.min() >= 0 and u.max() <= 1 and v.min() >= 0 and v.max() <= 1
    assert np.signbit(u[u == 0]).any()                            # -0.0 is there
    check_rows(shw, u, v, exhaustive_rows=(0, 3, 11, 500, ROWS - 1))    # 3, 11: rows with the 64-fold value


def outside_rows():
    """The rows of tests/golden/g13_rows_outside_unit.npz (seeds 81 / 82, six values per row outside [0, 1])."""
    u, v = edge_rows(81, outside=6), edge_rows(82, outside=6)
    # one out-of-range value in ONE cloud of the row only, at the very end / start of the row
    u[5], v[5] = np.clip(u[5], 0, 1), np.clip(v[5], 0, 1)
    v[5, -1] = np.float32(1.25)
    u[6], v[6] = np.clip(u[6], 0, 1), np.clip(v[6], 0, 1)
    u[6, 0] = np.float32(-0.25)
    return u, v


def test_rows_that_leave_the_unit_interval(shw, golden):
    """shw.h asks for coordinates in [0, 1]; values outside it have always been sorted exactly all the same (the former
    bin map saturated).  The byte-offset map does not, so such a row is sent to the network: same order, same cost.

    A row that spans more than one turn has no convex c(k) (v_ext is not monotone), so the shift search ends in a local
    minimum that exact_shift's global argmin need not share (on the CPU: rows 3 and 11 differ by 15 % and a factor 3.9).
    The expected values are therefore what the build before this map returned for these rows on an MI355X, recorded in
    the fixture with the seeds.  Sort and loads are exact and the solve is unchanged: the costs must be the same bits."""
    u, v = outside_rows()
    assert u.min() < -0.01 and u.max() > 1.01 and v.min() < -0.01 and v.max() > 1.01
    fix = golden("g13_rows_outside_unit.npz")
    assert int(fix["seed_u"]) == 81 and int(fix["seed_v"]) == 82 and int(fix["outside"]) == 6
    want = fix["cost"]
    got = shw.binary_search_circle(torch.from_numpy(u).cuda(), torch.from_numpy(v).cuda(), p=2).cpu().numpy()
    assert got.shape == want.shape and got.dtype == want.dtype
    diff = np.abs(got.astype(np.float64) - want) / want
    print(f"rows {got.size}: {int((got != want).sum())} differ from the recorded costs, largest relative difference {diff.max():.3e}")
    assert np.array_equal(got, want)
