"""The point loader of the full loss-kernel classes on the device (`-m gpu`): csrc/ssw_common.hpp, load_coords and the
rolling loader of the 2048-point one-wave class (load_coords_rolling: sub-chunks of 8 rows, the next one in flight while
one is computed, the target's first sub-chunk issued before the source's sort).  The tests pin what a loader must deliver
-- every row of a cloud once, from the right cloud of the right pair -- and pass on any correct loader.

Shapes: B = 2 pairs, L = 4 slices, n = m in {2048, 1024, 512}: the full classes of 32 (one wave per slice), 16 and 8 keys
per lane (two waves per slice).  A lane owns the points r * 64 + lane, "row" r = 0 .. n / 64 - 1.

1. Wrong sub-chunk.  A loader that takes a sub-chunk twice, drops one or takes one of the other cloud changes the
   multiset of coordinates of a slice.
   a. y = a fixed permutation of x: every per-slice cost is exactly 0.0 at shift 0.
   b. y = x except in ONE row r0 (64 points, replaced by a tight cap around +y), r0 at both sides of every sub-chunk
      boundary: 0, 7, 8, 15, 16, 23, 24, 31 (those below n / 64).  Per-slice costs within 2e-5 relative of
      oracle/ref_mirror.per_slice_costs, the bound of tests/test_circle_coord_gpu.py at p = 2 (the oracle's own float32
      error on these cases, against its float64 evaluation: 3e-7).
2. Prefetch across clouds or pairs.  Pair 0: the northern hemisphere (z > 0) against the southern one; pair 1: the eastern
   hemisphere (x > 0) against the western one, and its target -- the last cloud of the batch -- ends in one row of points
   of a third kind, a tight cap around +y.  Rows taken from the neighbouring cloud or pair move the costs by tens of per
   cent; every (pair, slice), the last of the grid included, within 2e-5 relative of the oracle.
3. The other entry through the same function, coordinate-row mode (`dirs == NULL`, n = 2048): the rows of
   shw.circle_coordinates (its own kernel, csrc/shw_ssw_dim.hip: it does not run through load_coords, and states the bits
   the R^3 loaders compute) go through shw.binary_search_circle at p = 2 and give the per-slice costs of the point mode
   within 2e-5 relative (the bound of tests/test_sphere_dim_gpu.py for this identity) and the oracle's within the same.
"""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

B, L = 2, 4
SIZES = (2048, 1024, 512)
BOUNDARY_ROWS = (0, 7, 8, 15, 16, 23, 24, 31)
TOL = 2e-5                       # tests/test_circle_coord_gpu.py, test_seam_clouds, p = 2


@pytest.fixture(scope="module")
def shw():
    import shw_amd
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    shw_amd._lib.load()
    return shw_amd


def unit(v):
    return (v / np.linalg.norm(v, axis=-1, keepdims=True)).astype(np.float32)


@functools.lru_cache(maxsize=None)
def base_case(n):
    """(x (B,n,3), U (B,L,3,2)) float32: seeded Gaussian clouds on the sphere and QR frames."""
    rng = np.random.default_rng(1800 + n)
    x = unit(rng.standard_normal((B, n, 3)))
    U = np.linalg.qr(rng.standard_normal((B, L, 3, 2)))[0].astype(np.float32)
    return x, U


def oracle_costs(x, y, U):
    """(B, L) float64 from oracle/ref_mirror.per_slice_costs, pair by pair."""
    from oracle import ref_mirror
    return np.stack([ref_mirror.per_slice_costs(torch.from_numpy(x[b]), torch.from_numpy(y[b]), torch.from_numpy(U[b]),
                                                p=2).numpy().astype(np.float64) for b in range(x.shape[0])])


def device_costs(shw, x, y, U):
    _, cost, shift = shw.ssw_pair_losses(torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda(), torch.from_numpy(U).cuda(),
                                         p=2, return_slices=True)
    return cost.cpu().numpy().astype(np.float64), shift.cpu().numpy()


@functools.lru_cache(maxsize=None)
def one_row_case(n, r0):
    x, U = base_case(n)
    y = x.copy()
    cap = np.array([0.0, 1.0, 0.0]) + 0.05 * np.random.default_rng(1600 + r0).standard_normal((B, 64, 3))
    y[:, r0 * 64:(r0 + 1) * 64] = unit(cap)
    return x, y, U, oracle_costs(x, y, U)


@functools.lru_cache(maxsize=None)
def hemisphere_case(n):
    rng = np.random.default_rng(1900 + n)
    g = unit(rng.standard_normal((4, n, 3)))
    x, y = np.empty((B, n, 3), dtype=np.float32), np.empty((B, n, 3), dtype=np.float32)
    x[0], y[0] = g[0], g[1]
    x[0][:, 2], y[0][:, 2] = np.abs(g[0][:, 2]), -np.abs(g[1][:, 2])          # north against south
    x[1], y[1] = g[2], g[3]
    x[1][:, 0], y[1][:, 0] = np.abs(g[2][:, 0]), -np.abs(g[3][:, 0])          # east against west
    cap = np.array([0.0, 1.0, 0.0]) + 0.05 * rng.standard_normal((64, 3))
    y[1][n - 64:] = unit(cap)                                                 # the batch's last row: a cap around +y
    _, U = base_case(n)
    return x, y, U, oracle_costs(x, y, U)


@pytest.mark.parametrize("n", SIZES)
def test_permuted_twin_costs_nothing(shw, n):
    x, U = base_case(n)
    rng = np.random.default_rng(1700 + n)
    y = np.stack([x[b][rng.permutation(n)] for b in range(B)])
    cost, shift = device_costs(shw, x, y, U)
    print(f"n={n}: costs {cost.ravel()}, shifts {shift.ravel()}")
    assert cost.shape == (B, L) and shift.shape == (B, L)
    assert (cost == 0.0).all(), cost
    assert (shift == 0).all(), shift


@pytest.mark.parametrize("n", SIZES)
def test_one_row_differs(shw, n):
    rows = [r for r in BOUNDARY_ROWS if r < n // 64]
    assert rows and rows[-1] == n // 64 - 1
    for r0 in rows:
        x, y, U, ref = one_row_case(n, r0)
        cost, _ = device_costs(shw, x, y, U)
        err = np.abs(cost - ref) / ref
        print(f"n={n} row {r0}: costs {cost.ravel()}, largest relative error {err.max():.3e} (bound {TOL})")
        assert ref.min() > 0
        assert err.max() <= TOL, (n, r0, cost, ref)


@pytest.mark.parametrize("n", SIZES)
def test_hemispheres_and_the_last_row_of_the_batch(shw, n):
    x, y, U, ref = hemisphere_case(n)
    cost, _ = device_costs(shw, x, y, U)
    err = np.abs(cost - ref) / ref
    print(f"n={n}: costs {cost.ravel()}, oracle {ref.ravel()}, largest relative error {err.max():.3e} (bound {TOL})")
    # what a loader that mixed the clouds up would give is far outside the bound: the source against itself costs 0, the
    # other pair's clouds and the target without its cap cost visibly different amounts
    swapped = oracle_costs(x, y[::-1].copy(), U)
    no_cap = y.copy()
    no_cap[1][n - 64:] = y[1][:64]
    assert (np.abs(swapped - ref) / ref).min() > 100 * TOL
    assert (np.abs(oracle_costs(x[1:], no_cap[1:], U[1:]) - ref[1:]) / ref[1:]).min() > 100 * TOL
    assert err.max() <= TOL, (cost, ref)


def test_coordinate_rows_take_the_unpipelined_branch(shw):
    n = 2048
    x, y, U, ref = hemisphere_case(n)
    xd, yd, Ud = (torch.from_numpy(v).cuda() for v in (x, y, U))
    cost, _ = device_costs(shw, x, y, U)
    cx, cy = shw.circle_coordinates(xd, Ud), shw.circle_coordinates(yd, Ud)
    assert tuple(cx.shape) == (B, L, n)
    rows = shw.binary_search_circle(cx.reshape(B * L, n), cy.reshape(B * L, n), p=2).cpu().numpy().astype(np.float64)
    rows = rows.reshape(B, L)
    print(f"rows {rows.ravel()}, points {cost.ravel()}: {int((rows == cost).sum())} of {rows.size} bit-equal; largest "
          f"relative difference {np.abs(rows / cost - 1).max():.3e}, from the oracle {np.abs(rows / ref - 1).max():.3e}")
    assert np.abs(rows / cost - 1).max() < TOL
    assert np.abs(rows / ref - 1).max() <= TOL
