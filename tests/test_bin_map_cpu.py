"""The bin map of the distribution sort (csrc/bin_sort.hpp, binsort_off), restated in numpy.  No GPU.

    off = bits(fma(key, 4 NB - 1, 2^23)) & (next_pow2(4 NB) - 4)        bin = off / 4

The sort is exact for any map that is monotone non-decreasing in the key and stays inside the NB counters; this file
checks both over dense sets of fp32 keys in [0, 1] for every bin count the kernels use, and pins down where the keys
outside that domain land (the kernel's comment states it; the callers keep such keys away from the map).
"""
import numpy as np
import pytest

BIN_COUNTS = [256, 512, 768, 1024]      # 8, 16, 20 / 24 and 28 / 32 keys per lane


def next_pow2(v):
    r = 1
    while r < v:
        r <<= 1
    return r


def fma_bits_exact(key, nb):
    """Bit pattern of the fp32 fma(key, 4 nb - 1, 2^23) for fp32 keys in [0, 1 + 2^-23], by integer arithmetic: the sum lies
    in [2^23, 2^24) where an ulp is 1, so it is 2^23 + round_half_even(key (4 nb - 1))."""
    key = np.asarray(key, dtype=np.float32)
    bits = key.view(np.uint32).astype(np.int64) & 0x7fffffff          # -0 -> +0
    e = bits >> 23
    mant = np.where(e == 0, bits & 0x7fffff, (bits & 0x7fffff) | 0x800000)
    s = np.where(e == 0, 149, 150 - e)                                # key = mant 2^-s, s >= 23 for key <= 1 + 2^-23
    assert (s >= 23).all()
    prod = mant * (4 * nb - 1)                                        # < 2^36
    s = np.minimum(s, 40)                                             # prod 2^-40 < 1/16: rounds to 0 all the same
    q = prod >> s
    rem = prod - (q << s)
    half = np.int64(1) << (s - 1)
    r = q + ((rem > half) | ((rem == half) & ((q & 1) == 1)))
    return (0x4b000000 + r).astype(np.uint32)


def fma_bits_f64(key, nb):
    """The same for fp32 keys of any sign and size whose last mantissa bit is worth 2^-29 or more (|key| >= 2^-5, or a
    short dyadic fraction): product and sum are then exact in float64 and the cast rounds once, like the FMA."""
    with np.errstate(invalid="ignore", over="ignore"):
        t = np.asarray(key, dtype=np.float32).astype(np.float64) * np.float64(4 * nb - 1) + np.float64(2.0 ** 23)
        return t.astype(np.float32).view(np.uint32)


def offset(bits, nb):
    return bits & np.uint32(next_pow2(4 * nb) - 4)


def dense_keys(seed):
    rng = np.random.default_rng(seed)
    one = np.float32(1.0)
    parts = [
        rng.random(1_500_000, dtype=np.float32),
        np.linspace(0.0, 1.0, 300_001, dtype=np.float32),
        # around every bin edge of both the old map (k / NB) and the new one ((4 k + 2) / (4 NB - 1))
        np.concatenate([np.arange(0, 1025, dtype=np.float32) / np.float32(1024),
                        np.arange(0, 4096, dtype=np.float32) / np.float32(4095),
                        np.arange(0, 3072, dtype=np.float32) / np.float32(3071)]),
        np.array([0.0, -0.0, 1.0, np.nextafter(one, np.float32(0)), np.nextafter(one, np.float32(2)),
                  np.float32(1e-45), np.float32(1e-40), np.float32(1.1754944e-38), np.float32(2.0 ** -30)],
                 dtype=np.float32),
    ]
    k = np.concatenate(parts)
    below = np.nextafter(k, np.float32(-1), dtype=np.float32)
    above = np.nextafter(k, np.float32(2), dtype=np.float32)
    k = np.concatenate([k, below, above])
    k = k[(k >= 0) & (k <= np.nextafter(one, np.float32(2)))]
    return np.sort(k)                                                 # (-0 sorts with +0)


@pytest.mark.parametrize("nb", BIN_COUNTS)
def test_map_is_monotone_and_in_range(nb):
    keys = dense_keys(4100 + nb)
    assert keys.size > 3_000_000
    off = offset(fma_bits_exact(keys, nb), nb).astype(np.int64)
    assert (off % 4 == 0).all()
    b = off // 4
    assert b.min() == 0 and b.max() == nb - 1, (b.min(), b.max())
    assert (np.diff(b) >= 0).all()
    assert b[0] == 0                                                  # 0, -0 and the denormals
    assert (b[keys >= 1.0] == nb - 1).all()                           # 1 and the float above it
    # every counter can be reached: the map spreads [0, 1] over all NB bins
    assert np.unique(b).size == nb


@pytest.mark.parametrize("nb", BIN_COUNTS)
def test_float64_restatement_agrees(nb):
    """The restatement used for the out-of-range keys is the same function on the domain."""
    keys = dense_keys(77)[::7]
    keys = keys[(keys == 0) | (keys >= np.float32(2.0 ** -5))]
    assert keys.size > 300_000
    assert (fma_bits_exact(keys, nb) == fma_bits_f64(keys, nb)).all()


def test_keys_outside_the_domain_land_where_the_kernel_says():
    """bin_sort.hpp, comment of binsort_off: NaN -> the low bits of the NaN (0 for the canonical one), +inf -> 0, and no
    saturation: 1.5 -> (NB - 1) / 2, -0.25 -> NB / 2.  Always a multiple of four below next_pow2(4 NB)."""
    for nb in BIN_COUNTS:
        limit = next_pow2(4 * nb)
        odd = np.array([np.nan, np.inf, -np.inf, 1.5, -0.25, -0.5, 1.25, 2.0, -1.0, 1000.0, -1000.0], dtype=np.float32)
        off = offset(fma_bits_f64(odd, nb), nb).astype(np.int64)
        assert (off % 4 == 0).all() and (off >= 0).all() and (off < limit).all()
        assert off[0] == 0 and off[1] == 0                            # NaN (canonical), +inf
    nb = 1024
    got = offset(fma_bits_f64(np.array([1.5, -0.25], dtype=np.float32), nb), nb) // 4
    assert list(got) == [511, 512]                                    # not saturating: such keys must not reach the map


def test_equal_bin_runs_are_as_short_as_with_the_floor_map():
    """Longest run of keys sharing a bin on 2048 uniform keys (what sets the number of fix-up phases): the rounding map
    has bins 4 / (4 NB - 1) wide (3.5 / (4 NB - 1) at the two ends) against 1 / NB: the same run statistics."""
    rng = np.random.default_rng(5)
    nb = 1024
    new_runs, old_runs = [], []
    for _ in range(400):
        k = rng.random(2048, dtype=np.float32)
        new_runs.append(np.bincount(offset(fma_bits_exact(k, nb), nb) // 4, minlength=nb).max())
        old_runs.append(np.bincount(np.minimum((k * np.float32(nb)).astype(np.int64), nb - 1), minlength=nb).max())
    assert abs(np.mean(new_runs) - np.mean(old_runs)) < 0.25, (np.mean(new_runs), np.mean(old_runs))
    assert abs(np.percentile(new_runs, 99) - np.percentile(old_runs, 99)) <= 1
