"""Every remainder of the fix-up's phase count in the headline loss kernel, bit for bit (`-m gpu`, MI355X).

The full one-wave class (n = m = 2048, p = 2) runs g phases of odd-even transposition behind its distribution sort, g the
longest run of keys that share a bin: the g mod 4 odd phases and the trips of four (csrc/bin_sort.hpp,
binsort_read_back_and_fix; tests/test_fixup_schedule_cpu.py restates the order).  Here g is set row by row.

Coordinate-row mode (shw_circle_ot, the kernel's sort behind the loader's row branch).  A row holds two keys in every bin
of the byte-offset map (tests/test_bin_map_cpu.py restates the map) except one bin with g keys a few ulps apart, g = 2 ..
13: every residue mod 4 three times.  To keep 2048 keys, g - 2 other bins hold one key; how many of them lie below the
heavy bin sets the sorted position of its first key: an even register of a lane, an odd register, or register 30 of a
lane, which puts the run across the boundary between two lanes (g = 2, the row with two keys in every bin, has nothing to
drop: even starts only).  No other bin holds more than two keys, so
the row runs exactly g phases.  The source row presents the heavy bin's keys in descending order -- at points lane + 64 r,
r = 0, 1, ..: one lane's successive keys, whose atomics are served in program order -- and the target row in another
order.  Source and target are the same multiset of distinct keys: two exact sorts give the same array twice, the cost is
exactly 0.0 and the shift 0, and any pair left the wrong way round makes the cost positive (two adjacent floats exchanged
give 2 ulp^2 / n, far above the smallest float32).  No tolerance is involved.  1152 rows (36 cases x 32 heavy bins), more
than the 1024 problems below which the small-grid kernels take over.

One projected case, B = 2, L = 8, N = 2048, seeded Gaussian clouds, against oracle/ref_mirror.per_slice_costs at 2e-5: as
the call stands (16 problems: the small-grid kernels) and with the two pairs repeated until the launch holds more than
1024 problems and runs the one-wave kernel.
"""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

N, NB = 2048, 1024
RUNS = tuple(range(2, 14))
PLACES = ("even", "odd", "across")
COPIES = 32


@pytest.fixture(scope="module")
def shw():
    import shw_amd
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    shw_amd._lib.load()
    return shw_amd


def bin_of(key):
    """bin of the byte-offset map at 32 keys per lane (csrc/bin_sort.hpp, binsort_off<1024>)"""
    t = (np.asarray(key, dtype=np.float64) * 4095.0 + 8388608.0).astype(np.float32)      # one rounding, as the FMA
    return (t.view(np.uint32) & np.uint32(4092)) >> np.uint32(2)


def heavy_row(g, place, copy, rng):
    """(source row, target row, sorted position of the heavy bin's first key)"""
    drops = g - 2                                             # bins that hold one key instead of two
    if place == "across":
        want = 30
    else:
        want = 2 * int(rng.integers(0, 8)) + (1 if place == "odd" else 0)
    below = (-want) % 2                                       # start = 2 h - below: its parity is that of `below`
    assert below <= drops, (g, place)                         # (g = 2 has no bin to drop: see cases())
    h = ((want + below) // 2) % 16 + 16 * (1 + copy)          # 2 h - below = want (mod 32); bins 16 .. 527
    bins = np.arange(NB)
    others = bins[bins != h]
    low = rng.choice(others[others < h], size=below, replace=False)
    high = rng.choice(others[others > h], size=drops - below, replace=False)
    single = np.zeros(NB, dtype=bool)
    single[low] = single[high] = True
    first = ((4.0 * others + 0.5) / 4095.0).astype(np.float32)
    second = ((4.0 * others[~single[others]] + 2.5) / 4095.0).astype(np.float32)
    c = np.float32((4.0 * h + 1.5) / 4095.0)
    chain = c + np.arange(g, dtype=np.float32) * np.spacing(c)
    rest = np.concatenate([first, second])
    keys = np.concatenate([rest, chain])
    assert keys.size == N and np.unique(keys).size == N and keys.min() > 0 and keys.max() < 1
    counts = np.bincount(bin_of(keys), minlength=NB)
    assert counts[h] == g and (bin_of(chain) == h).all() and np.delete(counts, h).max() <= 2 and counts.min() >= 1
    start = int((keys < chain[0]).sum())
    assert start % 32 == want, (g, place, start)

    def lay(order):
        lane = int(rng.integers(0, 64))
        at = lane + 64 * np.arange(g)                         # one lane's keys r = 0 .. g - 1: served in this order
        row = np.empty(N, dtype=np.float32)
        free = np.ones(N, dtype=bool)
        free[at] = False
        row[at] = chain[order]
        row[free] = rest[rng.permutation(rest.size)]
        return row

    other = rng.permutation(g)
    while g > 1 and (other == np.arange(g)[::-1]).all():
        other = rng.permutation(g)
    return lay(np.arange(g)[::-1]), lay(other), start


def cases():
    """g = 2 is the row with two keys in EVERY bin: each run starts at an even register and none lies across a lane
    boundary (2048 keys in 1024 bins leave no bin to drop), so its three cases are all even starts"""
    return [(g, "even" if g == 2 else place) for g in RUNS for place in PLACES]


@pytest.fixture(scope="module")
def rows():
    rng = np.random.default_rng(2301)
    u, v, meta = [], [], []
    for g, place in cases():
        for copy in range(COPIES):
            a, b, start = heavy_row(g, place, copy, rng)
            u.append(a); v.append(b); meta.append((g, place, start))
    return np.stack(u), np.stack(v), meta


def test_rows_cover_every_remainder_and_position(rows):
    u, v, meta = rows
    assert u.shape == (len(RUNS) * len(PLACES) * COPIES, N) and u.shape[0] > 1024
    assert (np.sort(u, axis=1) == np.sort(v, axis=1)).all() and (u != v).any(axis=1).all()
    for res in range(4):
        gs = {g for g, _, _ in meta if g % 4 == res}
        assert len(gs) == 3, (res, gs)
        for g in gs:
            starts = {s % 32 for gg, _, s in meta if gg == g}
            assert any(s % 2 == 0 and s < 30 for s in starts)
            assert g == 2 or any(s % 2 == 1 and s < 30 for s in starts)
            assert g == 2 or any(s == 30 for s in starts)                     # across a lane boundary: registers 30 ..


def test_heavy_bin_rows_cost_exactly_zero(shw, rows):
    u, v, meta = rows
    lib = shw._lib.load()
    du, dv = torch.from_numpy(u).cuda(), torch.from_numpy(v).cuda()
    cost = torch.full((u.shape[0],), -1.0, dtype=torch.float32, device="cuda")
    shift = torch.full((u.shape[0],), -99, dtype=torch.int32, device="cuda")
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    rc = lib.shw_circle_ot(du.data_ptr(), dv.data_ptr(), None, None, 0, 0, u.shape[0], N, N, 2.0,
                           shw._lib.CIRCLE_BISECTION, cost.data_ptr(), shift.data_ptr(), None, None, stream)
    assert rc == 0, rc
    torch.cuda.synchronize()
    cost, shift = cost.cpu().numpy(), shift.cpu().numpy()
    bad = np.nonzero((cost != 0) | (shift != 0))[0]
    print(f"rows {u.shape[0]}: {int((cost != 0).sum())} costs are not 0.0 (largest {np.abs(cost).max():.3e}), "
          f"{int((shift != 0).sum())} shifts are not 0; first bad (g, place, start): {[meta[i] for i in bad[:8]]}")
    assert bad.size == 0, ([meta[i] for i in bad[:8]], cost[bad[:8]], shift[bad[:8]])


def test_projected_case_against_the_mirror(shw):
    from oracle import ref_mirror
    B, L = 2, 8
    gen = torch.Generator().manual_seed(2302)
    x = torch.nn.functional.normalize(torch.randn(B, N, 3, generator=gen), dim=-1)
    y = torch.nn.functional.normalize(torch.randn(B, N, 3, generator=gen), dim=-1)
    U = torch.linalg.qr(torch.randn(B, L, 3, 2, generator=gen))[0]
    ref = torch.stack([ref_mirror.per_slice_costs(x[b], y[b], U[b], p=2) for b in range(B)]).numpy()
    _, cost, _ = shw.ssw_pair_losses(x.cuda(), y.cuda(), U.cuda(), p=2, return_slices=True)
    rel = np.abs(cost.cpu().numpy() - ref) / ref
    rep = 1024 // (B * L) + 1                                   # 65 copies: 1040 problems, the one-wave kernel
    _, many, _ = shw.ssw_pair_losses(x.repeat(rep, 1, 1).cuda(), y.repeat(rep, 1, 1).cuda(), U.repeat(rep, 1, 1, 1).cuda(),
                                     p=2, return_slices=True)
    many = many.cpu().numpy().reshape(rep, B, L)
    rel_many = np.abs(many - ref[None]) / ref[None]
    print(f"largest relative error: {rel.max():.3e} as called, {rel_many.max():.3e} over {rep * B * L} problems (bound 2e-5)")
    assert rel.max() <= 2e-5, rel.max()
    assert rel_many.max() <= 2e-5, rel_many.max()
    assert (many == many[0]).all()                              # the same problem gives the same bits in every copy
