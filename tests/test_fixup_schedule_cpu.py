"""The phase order of the full classes' fix-up (csrc/bin_sort.hpp, binsort_read_back_and_fix), restated in numpy.  No GPU.

After the read-back every lane holds 32 consecutive sorted positions, and every run of keys that share a bin is at most
g long.  The kernel then runs g phases of odd-even transposition, the g mod 4 odd ones FIRST and the trips of four
behind them:

    g mod 4 = 1:  odd            g mod 4 = 2:  even, odd            g mod 4 = 3:  odd, even, odd
    then g / 4 trips of  even, odd, even, odd

so the alternation is unbroken into the loop, which begins with an even phase, and the sequence starts with an even or
an odd phase depending on g.  An even phase compare-exchanges the register pairs (2i, 2i + 1) of a lane; an odd phase the
pairs (2i + 1, 2i + 2) and register 31 of every lane with register 0 of the next.

That g alternating phases sort a run of length <= g whichever parity comes first is checked here by the 0-1 principle:
for g = 1 .. 12 and every register offset 0 .. 31 of the run's first key (offsets 21 .. 31 put a run of 12 across a lane
boundary; both parities of the start occur), every one of the 2^g fillings of the run with zeros and ones, zeros to its
left and ones to its right, must come out sorted.  The schedule of g - 1 phases must leave at least one filling of a run
of length g unsorted (at every second offset or more: where the run's first pair is not a pair of the first phase): the
test cannot pass vacuously, and g phases are not one too many.
"""
import numpy as np
import pytest

EPT, LANES = 32, 3                      # the run starts in lane 1: a lane boundary on either side


def schedule(g):
    """the phases binsort_read_back_and_fix runs for a longest run g: 'e' (even) and 'o' (odd), in order"""
    head = {0: "", 1: "o", 2: "eo", 3: "oeo"}[g & 3]
    return head + "eoeo" * (g >> 2)


def even_phase(x):
    """x: (fillings, LANES, EPT); pairs (2i, 2i + 1) inside every lane"""
    lo = np.minimum(x[..., 0::2], x[..., 1::2])
    hi = np.maximum(x[..., 0::2], x[..., 1::2])
    x[..., 0::2], x[..., 1::2] = lo, hi


def odd_phase(x):
    """pairs (2i + 1, 2i + 2) inside every lane, then the last key of a lane against the first key of the next; the
    first lane's register 0 and the last lane's register 31 keep their keys"""
    a, b = x[..., 1:EPT - 1:2], x[..., 2:EPT:2]
    lo, hi = np.minimum(a, b), np.maximum(a, b)
    x[..., 1:EPT - 1:2], x[..., 2:EPT:2] = lo, hi
    last, first = x[:, :-1, EPT - 1].copy(), x[:, 1:, 0].copy()      # as they stand after the in-lane pairs
    x[:, :-1, EPT - 1] = np.minimum(last, first)
    x[:, 1:, 0] = np.maximum(last, first)


def run_phases(x, phases):
    for ph in phases:
        (even_phase if ph == "e" else odd_phase)(x)
    return x


def fillings(g, offset):
    """(2^g, LANES, EPT) arrays: zeros, the 2^g fillings of a run of g keys that starts at register `offset` of lane 1, ones"""
    start = EPT + offset
    x = np.zeros((1 << g, LANES * EPT), dtype=np.int8)
    x[:, start + g:] = 1
    x[:, start:start + g] = (np.arange(1 << g)[:, None] >> np.arange(g)[None, :]) & 1
    return x.reshape(1 << g, LANES, EPT)


def is_sorted(x):
    flat = x.reshape(x.shape[0], -1)
    return (np.diff(flat, axis=1) >= 0).all(axis=1)


def test_schedule_alternates_and_ends_in_the_loop():
    for g in range(0, 41):
        s = schedule(g)
        assert len(s) == g
        assert all(a != b for a, b in zip(s, s[1:]))                  # unbroken alternation
        assert g == 0 or s[-1] == "o"                                 # every path ends with an odd phase ...
        assert s[len(s) - 4 * (g >> 2):] == "eoeo" * (g >> 2)         # ... and the trips begin with an even one
    assert {schedule(g)[0] for g in range(1, 13)} == {"e", "o"}       # both parities come first for some g


@pytest.mark.parametrize("g", range(1, 13))
def test_g_phases_sort_every_run_of_length_g(g):
    crossing = 0
    for offset in range(EPT):
        x = fillings(g, offset)
        before = x.sum()
        run_phases(x, schedule(g))
        assert x.sum() == before                                      # a compare-exchange loses no key
        ok = is_sorted(x)
        assert ok.all(), (g, offset, np.nonzero(~ok)[0][:5])
        crossing += offset + g > EPT
    assert crossing == g - 1                                          # the runs that lie across the lane boundary


@pytest.mark.parametrize("g", range(2, 13))
def test_one_phase_fewer_is_not_enough(g):
    unsorted = [offset for offset in range(EPT)
                if not is_sorted(run_phases(fillings(g, offset), schedule(g - 1))).all()]
    print(f"g={g}: {g - 1} phases leave a filling unsorted at {len(unsorted)} of {EPT} offsets")
    assert unsorted, g
    # a run whose first pair is not a pair of the first phase loses that phase: at least every second offset
    assert len(unsorted) >= EPT // 2, (g, unsorted)
