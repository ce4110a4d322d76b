"""The headline loss kernel's sort with its counters UNDER the staging buffer, bit for bit (`-m gpu`, MI355X).

The full one-wave class (n = m = 2048, p = 2) counts its keys into 1280 bins (20 per lane of the scan; csrc/bin_sort.hpp,
wave_sort_binned with ALIAS_BPL): 5120 bytes of counters that start where the 4096 bytes of the other classes' 1024
counters start and run on over the first 1024 bytes of the staging buffer.  All 32 positions of a lane are taken before its
first key is written (binsort_place_full_two_step), and the next sort zeroes the counters only after this one's read-back.
What could go wrong is a key written over a counter that is still to be read, a counter zeroed over a key that is still to be
read, or a lane base of the scan that does not carry; each leaves keys out of order or lost.

Coordinate-row mode (shw_circle_ot, the kernel's sort behind the loader's row branch), more than 1024 rows in one launch
so that the one-wave kernel runs.  Source and target of a row are the same multiset of distinct keys in different orders:
two exact sorts give the same array twice, the cost is exactly 0.0 and the shift 0, and any pair left the wrong way round, or
a key lost, makes the cost positive (two adjacent floats exchanged give 2 ulp^2 / n, far above the smallest float32).  No
tolerance.  The rows, built with this file's restatement of the shipped map (tests/test_bin_map_wide_cpu.py checks the map):
  * every bin occupied (one key in each of the 1280, a second one in 768 of them), presented ascending, descending and in
    bit-reversed point order;
  * one heavy bin of g = 2 .. 13 keys a few ulps apart -- every other bin holds one or two -- at the first bin, the last
    bin (also the last counter under the buffer), the bin whose counter is the last one below byte 4096 and the one whose
    counter is the first at byte 4096, where the overlap begins;
  * the same with g = 40 and g = 41: the longest run the bins sort, and the shortest that goes to the bitonic network;
  * every key in [1/2, 1]: the first 640 bins are empty and the scan's lane bases carry across 32 whole lanes.
One asymmetric family (source uniform, a quarter of the target crowded into the 24 bins around byte 4096) against a float64
numpy evaluation of min_k c(k), and one projected case against oracle/ref_mirror.per_slice_costs, both at the project's
bound 2e-5.  On a library whose class has 1024 bins the rows are as exact and exercise less.
"""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

N, NB = 2048, 1280
SCALE = 4 * NB - 1
MASK = 8192 - 4                                  # next_pow2(4 NB) - 4
FIRST_UNDER_BUFFER = 4096 // 4                   # the bin whose counter is the first at byte 4096
PLACES = (0, NB - 1, FIRST_UNDER_BUFFER - 1, FIRST_UNDER_BUFFER)
RUNS = tuple(range(2, 14)) + (40, 41)
COPIES = 18


@pytest.fixture(scope="module")
def shw():
    import shw_amd
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    shw_amd._lib.load()
    return shw_amd


def bin_of(key):
    """bin of the byte-offset map with 1280 bins (csrc/bin_sort.hpp, binsort_off<1280>): one rounding, as the FMA"""
    t = (np.asarray(key, dtype=np.float64) * float(SCALE) + 8388608.0).astype(np.float32)
    return (t.view(np.uint32) & np.uint32(MASK)) >> np.uint32(2)


def bit_reversed(n):
    bits = n.bit_length() - 1
    i = np.arange(n)
    r = np.zeros(n, dtype=np.int64)
    for b in range(bits):
        r |= ((i >> b) & 1) << (bits - 1 - b)
    return r


def filled_bins(rng, heavy=None, g=0):
    """2048 distinct keys: `g` keys a few ulps apart in bin `heavy`, one key in every other bin and a second one in as many
    of them as it takes.  Returns (the keys without the heavy ones, the heavy ones ascending)."""
    bins = np.arange(NB)
    others = bins if heavy is None else bins[bins != heavy]
    twice = rng.choice(others, size=N - g - others.size, replace=False)
    first = ((4.0 * others + 0.5) / SCALE).astype(np.float32)
    second = ((4.0 * twice + 2.5) / SCALE).astype(np.float32)
    rest = np.concatenate([first, second])
    if heavy is None:
        chain = np.empty(0, dtype=np.float32)
    else:
        c = np.float32((4.0 * heavy + 1.5) / SCALE)
        chain = c + np.arange(g, dtype=np.float32) * np.spacing(c)
    keys = np.concatenate([rest, chain])
    assert keys.size == N and np.unique(keys).size == N and keys.min() > 0 and keys.max() < 1
    counts = np.bincount(bin_of(keys), minlength=NB)
    assert counts.size == NB and counts.min() >= 1
    if heavy is None:
        assert counts.max() == 2
    else:
        assert counts[heavy] == g and (bin_of(chain) == heavy).all() and np.delete(counts, heavy).max() <= 2
    return rest, chain


def heavy_row(g, heavy, rng):
    """The heavy bin's keys descending at one lane's successive points (lane + 64 r: served in program order), and past
    32 of them at a second lane's; the target in another order."""
    rest, chain = filled_bins(rng, heavy, g)

    def lay(order):
        a, b = rng.choice(64, size=2, replace=False)
        at = np.concatenate([a + 64 * np.arange(32), b + 64 * np.arange(32)])[:g]
        row = np.empty(N, dtype=np.float32)
        free = np.ones(N, dtype=bool)
        free[at] = False
        row[at] = chain[order]
        row[free] = rest[rng.permutation(rest.size)]
        return row

    other = rng.permutation(g)
    while (other == np.arange(g)[::-1]).all():
        other = rng.permutation(g)
    return lay(np.arange(g)[::-1]), lay(other)


@pytest.fixture(scope="module")
def rows():
    rng = np.random.default_rng(2801)
    u, v, meta = [], [], []
    rev = bit_reversed(N)
    for copy in range(4):
        rest, _ = filled_bins(rng)
        asc = np.sort(rest)
        for name, a, b in (("ascending", asc, asc[::-1]), ("descending", asc[::-1], asc[rev]), ("bit-reversed", asc[rev], asc)):
            u.append(a.copy()); v.append(b.copy()); meta.append(("every bin", name, copy))
    for copy in range(COPIES):
        for g in RUNS:
            for heavy in PLACES:
                a, b = heavy_row(g, heavy, rng)
                u.append(a); v.append(b); meta.append(("heavy", g, heavy))
    for copy in range(16):
        keys = np.unique((0.5 + 0.5 * rng.random(3 * N)).astype(np.float32))
        keys = rng.permutation(keys[keys < 1])[:N]
        assert keys.size == N and bin_of(keys).min() >= NB // 2
        u.append(keys); v.append(keys[rng.permutation(N)]); meta.append(("upper half", int(np.bincount(bin_of(keys)).max()), copy))
    return np.stack(u), np.stack(v), meta


def circle_ot(shw, u, v):
    lib = shw._lib.load()
    du, dv = torch.from_numpy(u).cuda(), torch.from_numpy(v).cuda()
    cost = torch.full((u.shape[0],), -1.0, dtype=torch.float32, device="cuda")
    shift = torch.full((u.shape[0],), -99, dtype=torch.int32, device="cuda")
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    rc = lib.shw_circle_ot(du.data_ptr(), dv.data_ptr(), None, None, 0, 0, u.shape[0], N, N, 2.0,
                           shw._lib.CIRCLE_BISECTION, cost.data_ptr(), shift.data_ptr(), None, None, stream)
    assert rc == 0, rc
    torch.cuda.synchronize()
    return cost.cpu().numpy(), shift.cpu().numpy()


def test_rows_are_what_they_claim(rows):
    u, v, meta = rows
    assert u.shape[0] > 1024 and u.shape == v.shape == (len(meta), N)
    assert (np.sort(u, axis=1) == np.sort(v, axis=1)).all() and (u != v).any(axis=1).all()
    assert 4 * (FIRST_UNDER_BUFFER - 1) == 4092 and 4 * FIRST_UNDER_BUFFER == 4096 and 4 * (NB - 1) + 4 <= 12288
    longest = np.array([np.bincount(bin_of(r), minlength=NB).max() for r in u])
    for i, m in enumerate(meta):
        if m[0] == "heavy":
            assert longest[i] == m[1] and np.bincount(bin_of(u[i]), minlength=NB)[m[2]] == m[1]
    assert {(m[1], m[2]) for m in meta if m[0] == "heavy"} == {(g, h) for g in RUNS for h in PLACES}
    assert {m[1] for m in meta if m[0] == "every bin"} == {"ascending", "descending", "bit-reversed"}
    asc = [i for i, m in enumerate(meta) if m[:2] == ("every bin", "ascending")]
    assert (np.diff(u[asc], axis=1) > 0).all() and (np.diff(v[asc], axis=1) < 0).all()


def test_same_multiset_rows_cost_exactly_zero(shw, rows):
    u, v, meta = rows
    cost, shift = circle_ot(shw, u, v)
    bad = np.nonzero((cost != 0) | (shift != 0))[0]
    print(f"rows {u.shape[0]}: {int((cost != 0).sum())} costs are not 0.0 (largest {np.abs(cost).max():.3e}), "
          f"{int((shift != 0).sum())} shifts are not 0; first bad: {[meta[i] for i in bad[:8]]}")
    assert bad.size == 0, ([meta[i] for i in bad[:8]], cost[bad[:8]], shift[bad[:8]])


def min_shift_cost(u, v):
    """min over k = -n .. n of c(k) = mean_i |u_(i) - (v_((i + k) mod n) + (i + k) div n)|^2, float64, 256 shifts at a time"""
    us, vs = np.sort(u.astype(np.float64)), np.sort(v.astype(np.float64))
    i = np.arange(N)
    best = np.inf
    for k0 in range(-N, N + 1, 256):
        q = i[None, :] + np.arange(k0, min(k0 + 256, N + 1))[:, None]
        c = ((us[None, :] - (vs[np.mod(q, N)] + np.floor_divide(q, N))) ** 2).mean(axis=1)
        best = min(best, float(c.min()))
    return best


def test_asymmetric_rows_against_float64(shw):
    """Source uniform; a quarter of the target crowded into the 24 bins around byte 4096 of the counters (runs of about 22
    .. 35 keys on both sides of the place where the overlap begins), the rest uniform.  Eight problems, each 130 times."""
    rng = np.random.default_rng(2802)
    lo, hi = (4.0 * (FIRST_UNDER_BUFFER - 12) - 0.5) / SCALE, (4.0 * (FIRST_UNDER_BUFFER + 12) - 0.5) / SCALE
    u = rng.random((8, N), dtype=np.float32)
    v = np.concatenate([rng.random((8, N - 512), dtype=np.float32),
                        (lo + (hi - lo) * rng.random((8, 512))).astype(np.float32)], axis=1)
    v = np.stack([r[rng.permutation(N)] for r in v])
    runs = [int(np.bincount(bin_of(r), minlength=NB).max()) for r in v]
    ref = np.array([min_shift_cost(a, b) for a, b in zip(u, v)])
    rep = 130
    cost, _ = circle_ot(shw, np.tile(u, (rep, 1)), np.tile(v, (rep, 1)))
    cost = cost.reshape(rep, 8)
    rel = np.abs(cost - ref[None]) / ref[None]
    print(f"longest runs of the targets {runs}; largest relative error {rel.max():.3e} over {rep * 8} rows (bound 2e-5)")
    assert min(runs) > 13 and ref.min() > 0
    assert rel.max() <= 2e-5, rel.max()
    assert (cost == cost[0]).all()                              # the same problem gives the same bits in every copy


def test_projected_case_against_the_mirror(shw):
    from oracle import ref_mirror
    B, L = 2, 8
    gen = torch.Generator().manual_seed(2803)
    x = torch.nn.functional.normalize(torch.randn(B, N, 3, generator=gen), dim=-1)
    y = torch.nn.functional.normalize(torch.randn(B, N, 3, generator=gen), dim=-1)
    U = torch.linalg.qr(torch.randn(B, L, 3, 2, generator=gen))[0]
    ref = torch.stack([ref_mirror.per_slice_costs(x[b], y[b], U[b], p=2) for b in range(B)]).numpy()
    rep = 1024 // (B * L) + 1                                   # 65 copies: 1040 problems, the one-wave kernel
    _, many, _ = shw.ssw_pair_losses(x.repeat(rep, 1, 1).cuda(), y.repeat(rep, 1, 1).cuda(), U.repeat(rep, 1, 1, 1).cuda(),
                                     p=2, return_slices=True)
    many = many.cpu().numpy().reshape(rep, B, L)
    rel = np.abs(many - ref[None]) / ref[None]
    print(f"largest relative error: {rel.max():.3e} over {rep * B * L} problems (bound 2e-5)")
    assert rel.max() <= 2e-5, rel.max()
    assert (many == many[0]).all()
