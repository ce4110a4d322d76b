"""The bin map of the distribution sort at the bin counts of the counters that lie under the staging buffer.  No GPU.

    off = bits(fma(key, 4 NB - 1, 2^23)) & (next_pow2(4 NB) - 4)        bin = off / 4          (csrc/bin_sort.hpp, binsort_off)

The headline loss kernel sorts 2048 keys with NB = 64 BPL bins, BPL a multiple of four bins per lane of the scan, where
the counters may take up to 12 288 bytes: NB = 1280 .. 2304 here, only one of them a power of two.  The sort is exact for
any map that is monotone non-decreasing in the key and stays inside the NB counters.  Restated on its own (the file for
the classes' regular bin counts is tests/test_bin_map_cpu.py): the FMA by integer arithmetic, the keys every float next
to a bin edge.
"""
import numpy as np
import pytest

BIN_COUNTS = [1280, 1536, 1792, 2048, 2304]      # 20, 24, 28, 32 and 36 bins per lane


def next_pow2(v):
    r = 1
    while r < v:
        r <<= 1
    return r


def fma_bits(key, nb):
    """fp32 fma(key, 4 nb - 1, 2^23) for fp32 keys in [0, 1 + 2^-23]: the sum lies in [2^23, 2^24), where an ulp is 1, so
    it is 2^23 + round_half_even(key (4 nb - 1)) -- product and rounding in integers."""
    key = np.asarray(key, dtype=np.float32)
    bits = key.view(np.uint32).astype(np.int64) & 0x7fffffff          # -0 -> +0
    e = bits >> 23
    mant = np.where(e == 0, bits & 0x7fffff, (bits & 0x7fffff) | 0x800000)
    s = np.where(e == 0, 149, 150 - e)                                # key = mant 2^-s
    assert (s >= 23).all()
    prod = mant * (4 * nb - 1)                                        # < 2^38
    s = np.minimum(s, 44)                                             # prod 2^-44 < 1/64: rounds to 0 all the same
    q = prod >> s
    rem = prod - (q << s)
    half = np.int64(1) << (s - 1)
    r = q + ((rem > half) | ((rem == half) & ((q & 1) == 1)))
    return (0x4b000000 + r).astype(np.uint32)


def offset(key, nb):
    return (fma_bits(key, nb) & np.uint32(next_pow2(4 * nb) - 4)).astype(np.int64)


def edge_keys(nb):
    """Every float next to a bin edge -- bin k begins where key (4 nb - 1) = 4 k - 1/2 -- three floats to either side of the
    nearest one, and the ends of the domain: 0, -0, denormals, 1 and the float above 1.  Ascending (-0 beside +0)."""
    k = np.arange(1, nb, dtype=np.float64)
    near = ((4.0 * k - 0.5) / (4 * nb - 1)).astype(np.float32)
    around = [near]
    lo = hi = near
    for _ in range(3):
        lo = np.nextafter(lo, np.float32(-1), dtype=np.float32)
        hi = np.nextafter(hi, np.float32(2), dtype=np.float32)
        around += [lo, hi]
    one = np.float32(1.0)
    ends = np.array([0.0, 1e-45, 1e-40, 1.1754942e-38, 1.1754944e-38, np.nextafter(one, np.float32(0)), 1.0,
                     np.nextafter(one, np.float32(2))], dtype=np.float32)
    keys = np.sort(np.concatenate(around + [ends]))
    return np.concatenate([np.array([-0.0], dtype=np.float32), keys])


@pytest.mark.parametrize("nb", BIN_COUNTS)
def test_offsets_are_counter_addresses_in_key_order(nb):
    keys = edge_keys(nb)
    assert np.signbit(keys[0]) and keys[1] == 0 and keys[-1] > 1
    off = offset(keys, nb)
    assert (off % 4 == 0).all()
    assert (np.diff(off) >= 0).all()
    assert off.min() == 0 and off.max() == 4 * nb - 4, (off.min(), off.max())
    assert (off[keys < np.float32(1e-30)] == 0).all()                 # 0, -0 and the denormals: the first counter
    assert (off[keys >= 1] == 4 * nb - 4).all()                       # 1 and the float above it: the last one
    assert np.unique(off).size == nb                                  # every counter has keys
    k = np.arange(1, nb, dtype=np.float64)
    below = ((4.0 * k - 0.75) / (4 * nb - 1)).astype(np.float32)      # a quarter of a rounding step to either side
    above = ((4.0 * k - 0.25) / (4 * nb - 1)).astype(np.float32)
    assert (offset(below, nb) == 4 * (k - 1)).all() and (offset(above, nb) == 4 * k).all()


@pytest.mark.parametrize("nb", BIN_COUNTS)
def test_uniform_keys_stay_inside_and_runs_shorten(nb):
    """Random keys: inside the counters, and the longest equal-bin run of 2048 uniform keys (the number of fix-up phases)
    is shorter than at 1024 bins on the same rows."""
    rng = np.random.default_rng(2800 + nb)
    rows = rng.random((200, 2048), dtype=np.float32)
    off = offset(rows, nb)
    assert (off % 4 == 0).all() and off.min() >= 0 and off.max() <= 4 * nb - 4
    runs = np.array([np.bincount(r // 4, minlength=nb).max() for r in off])
    base = np.array([np.bincount(r // 4, minlength=1024).max() for r in offset(rows, 1024)])
    assert runs.mean() < base.mean() - 0.5, (runs.mean(), base.mean())
