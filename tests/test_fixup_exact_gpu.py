"""The fix-up phases of the loss kernels' distribution sort, bit for bit (`-m gpu`, MI355X).

The tolerance tests cannot see a pair of keys left in the wrong order: two keys of one bin differ by less than 1/1024
and move a slice cost by about 1e-10.  Here the target is the source with its points permuted.  The two multisets of
circle coordinates are then identical, so two exact sorts give the same array twice: the cost at shift 0 is exactly
0.0, and it is the only zero (c(k) = 0 for a k != 0 needs u_(i) = u_(i+k) + const for every i, i.e. all coordinates
equal).  One compare-exchange that returns a wrong or misplaced key makes the cost positive: two adjacent floats the
wrong way round in one of the arrays give 2 ulp^2 / n > 1e-18, far above the smallest float32.

No row or slice is left out: the CPU oracle (oracle/exact_shift.py) confirms on sampled problems that shift 0 is the
unique argmin, and nothing else can tie (see above).

  * projection mode, B L = 1152 problems (more than the 1024 below which the small-grid kernels take over):
    2048 (one wave per slice, full class), 512 and 1024 (two waves, full), 2001 and 1200 (classes with pads),
    4096 (cooperative sort);
  * coordinate-row mode (shw.binary_search_circle, n = 2048): rows that hold 0.0, -0.0, the smallest denormal, 1.0 and
    the float below it; a chain of g adjacent floats inside one bin, g = 1, 2, 3, 8, 9, 39, 40; and, in every eighth
    row, 41 equal values, one more than SHW_BINSORT_MAX_RUN, which sends the row to the network.  A chain of g >= 4
    has exactly 32 j - 3 smaller keys in the row, so it lies across the boundary between two lanes of the read-back
    (sorted positions 32 j - 3 .. 32 j - 4 + g).  With 32 j - 3 a chain of 2 or 3 would end in front of the boundary,
    so it starts at 32 j - (g - 1) and its last key is the first of the next lane.  A chain of one key (g = 1) cannot
    lie across a boundary: it is the last key of its lane, 32 j - 1, and has nothing to be exchanged with but its
    neighbours of other bins.  The other keys of a row are uniform, so the number of phases a row runs is its longest
    equal-bin run: 39 or 40 where the chain has its bin to itself (with a neighbour in the bin it is longer and the row
    takes the network), else 6 .. 18, odd and even (asserted).
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

B, L = 3, 384
ROWS, N = 1120, 2048
CHAINS = (1, 2, 3, 8, 9, 39, 40)


@pytest.fixture(scope="module")
def shw():
    import shw_amd
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    shw_amd._lib.load()
    return shw_amd


@pytest.mark.parametrize("n", [2048, 512, 1024, 2001, 1200, 4096])
def test_permuted_twin_projection_mode(shw, n):
    from oracle import exact_shift
    g = torch.Generator().manual_seed(7100 + n)
    x = torch.nn.functional.normalize(torch.randn(B, n, 3, generator=g), dim=-1)
    y = torch.stack([x[b][torch.randperm(n, generator=g)] for b in range(B)])
    U = torch.linalg.qr(torch.randn(B, L, 3, 2, generator=g))[0]
    _, cost, shift = shw.ssw_pair_losses(x.cuda(), y.cuda(), U.cuda(), p=2, return_slices=True)
    cost, shift = cost.cpu().numpy(), shift.cpu().numpy()
    print(f"n={n}: {int((cost != 0).sum())} of {cost.size} slice costs are not 0.0 (largest {np.abs(cost).max():.3e}), "
          f"{int((shift != 0).sum())} shifts are not 0")
    if n <= 1200:                                                 # the oracle is O(n^2) per slice
        for b, l in ((0, 0), (2, L - 1)):
            cu = np.sort(exact_shift.circle_coords(x[b].numpy(), U[b, l:l + 1].numpy())[0])
            ks, c = exact_shift.shift_costs(cu, cu, 2)
            assert ks[int(np.argmin(c))] == 0 and c.min() == 0 and (c == 0).sum() == 1
    assert cost.shape == (B, L) and shift.shape == (B, L)
    assert (cost == 0).all(), (np.argwhere(cost != 0)[:5], cost[cost != 0][:5])
    assert (shift == 0).all(), (np.argwhere(shift != 0)[:5], shift[shift != 0][:5])


def bin_of(key):
    """bin of the byte-offset map at 32 keys per lane (csrc/bin_sort.hpp, binsort_off<1024>)"""
    t = (np.asarray(key, dtype=np.float64) * 4095.0 + 8388608.0).astype(np.float32)      # one rounding, as the FMA
    return (t.view(np.uint32) & np.uint32(4092)) >> np.uint32(2)


def chain_rows(seed):
    """(ROWS, N) float32 rows as the module docstring describes, with the longest equal-bin run of every row"""
    rng = np.random.default_rng(seed)
    one, zero = np.float32(1), np.float32(0)
    special = np.array([0.0, -0.0, np.nextafter(zero, one), 1.0, np.nextafter(one, zero)], dtype=np.float32)
    out = np.empty((ROWS, N), dtype=np.float32)
    glen = np.empty(ROWS, dtype=np.int64)
    for r in range(ROWS):
        g = CHAINS[r % len(CHAINS)]
        rest = rng.random(N - g, dtype=np.float32)
        rest[:special.size] = special
        if r % 8 == 5:
            rest[8:8 + 41] = rng.random(dtype=np.float32)     # 41 equal values: this row takes the network
        rest = np.sort(rest)
        lim = min(3, max(g - 1, 1))                           # keys of the chain in front of the lane boundary
        for j in rng.permutation(np.arange(2, 62)):
            k = 32 * int(j) - lim
            lo, hi = np.float64(rest[k - 1]), np.float64(rest[k])
            c = np.float32((lo + hi) / 2)
            chain = c + np.arange(g, dtype=np.float32) * np.spacing(c)
            if hi - lo > 2e-5 and np.unique(bin_of(chain)).size == 1:
                break
        else:
            raise AssertionError("no place for the chain")
        row = np.concatenate([rest, chain])
        assert row.size == N and np.unique(chain).size == g and np.unique(bin_of(chain)).size == 1
        assert (np.diff(chain.view(np.int32)) == 1).all()                                 # adjacent floats
        assert int((row < chain[0]).sum()) == k and (k + lim) % 32 == 0 and (g == 1 or g > lim)
        glen[r] = max(g, int(np.bincount(bin_of(row), minlength=1024).max()))
        out[r] = row[rng.permutation(N)]
    return out, glen


def test_permuted_twin_coordinate_rows(shw):
    from oracle import exact_shift
    u, glen = chain_rows(73)
    assert {39, 40} <= set(glen.tolist()) and len({int(t) % 2 for t in glen if t < 39}) == 2
    rng = np.random.default_rng(74)
    v = np.stack([row[rng.permutation(N)] for row in u])
    assert u.min() >= 0 and u.max() <= 1 and np.signbit(u[u == 0]).any() and (u == np.float32(1e-45)).any()
    for r in (0, 5):                                           # the oracle: shift 0 is the only minimum
        s = np.sort(u[r].astype(np.float64))
        ks, c = exact_shift.shift_costs(s, s, 2)
        assert ks[int(np.argmin(c))] == 0 and c.min() == 0 and (c == 0).sum() == 1
    got = shw.binary_search_circle(torch.from_numpy(u).cuda(), torch.from_numpy(v).cuda(), p=2).cpu().numpy()
    bad = np.nonzero(got != 0)[0]
    print(f"rows {ROWS}: {bad.size} costs are not 0.0 (largest {np.abs(got).max():.3e}); longest runs of the first bad "
          f"rows {glen[bad[:10]]}")
    assert got.shape == (ROWS,)
    assert bad.size == 0, (bad[:10], got[bad[:10]], glen[bad[:10]])
