"""The shift solve's target fetch at every alignment of its window (`-m gpu`).

The full 2048-point loss kernel fetches the sorted target four rows at a time (csrc/ssw_common.hpp, "grouped rows"): the
window of a shift k starts at row (k - 1) mod 32 of a column (k mod 32 for a one-shift evaluation), its position inside an
aligned group of four picks one of four unrolled bodies, and the groups behind a multiple of 8 come from the next column
(the carry).  This test pins what the solve returns, not the form of the fetch: it passes on the plain-row fetch too.

Rows as in tests/test_issue_rate_forms_gpu.py::test_shift_fetch_arithmetic (coordinate-row mode, shw_circle_ot): n distinct
multiples of 2^-20 inside an arc of 1/16 of the circle, target = (source + delta) mod 1 with delta a multiple of 2^-20, so
every value and every difference is exact in float32.  delta = 1 - (the K-th largest source value) makes exactly K target
values wrap and the optimal shift k* = K (arc in [0.7, 0.7625), delta < 1/2); delta = 1 - (the K-th smallest value) makes
n - K wrap and k* = -K (arc in [0.2, 0.2625), delta > 1/2).  K in 0 .. 8, 27 .. 37, 59 .. 69, n/2 - 2 .. n/2 + 2,
n - 3 .. n - 1, both signs: k* - 1 and k* take every residue mod 4 on both sides of the wrap of the row index (|k*| near
0, 32 and 64), of the multiple of 8 rows next to it, of half a turn, and at the end of the bracket |k| <= n.

n = 2048 only: the one kernel whose fetch is grouped (the two-wave kernels of 512 and 1024 points keep plain rows).
Oracle: oracle/exact_shift.shift_costs (float64, all 2 n + 1 shifts) on the sorted rows, once per power; its minimum must
be unique on every row and lie at the k* the row was built for -- asserted on the CPU first, so a tie cannot hide a wrong
shift.  GPU: the returned shift equals the argmin on every row, the cost is within 2e-6 relative of the float64 minimum
(the bound test_shift_fetch_arithmetic uses for such rows).  p = 2 (three-cost and one-shift evaluations), p = 3 and
p = 1.5 (the general-power kernel, which shares the search and keeps plain rows).
"""
import ctypes
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

N = 2048
GRID = 1 << 20
KS = tuple(range(0, 9)) + tuple(range(27, 38)) + tuple(range(59, 70)) + tuple(range(N // 2 - 2, N // 2 + 3)) + \
    tuple(range(N - 3, N))


@pytest.fixture(scope="module")
def shw():
    import shw_amd
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    shw_amd._lib.load()
    return shw_amd


def shifted_rows(n, seed):
    """(u, v, k*) of one row per wanted shift: u = n distinct multiples of 2^-20 in an arc of 1/16, v = (u + delta) mod 1"""
    rng = np.random.default_rng(seed)
    us, vs, ks = [], [], []
    for sign in (1, -1):
        for K in KS:
            start = int((0.7 if sign > 0 else 0.2) * GRID)
            ticks = np.sort(start + rng.choice(GRID // 16, size=n, replace=False))         # integers: coordinates * 2^20
            if sign > 0:
                d = GRID - ticks[n - K] if K > 0 else GRID // 5                             # exactly K values reach 1 and wrap
            else:
                d = GRID - ticks[K]                                                         # exactly n - K values wrap
            moved = (ticks + d) % GRID
            assert np.unique(moved).size == n and int((ticks + d >= GRID).sum()) == (K if sign > 0 else n - K)
            assert (2 * d < GRID) == (sign > 0)
            us.append(ticks[rng.permutation(n)])
            vs.append(moved[rng.permutation(n)])
            ks.append(sign * K)
    u = (np.stack(us).astype(np.float64) / GRID).astype(np.float32)
    v = (np.stack(vs).astype(np.float64) / GRID).astype(np.float32)
    assert (u.astype(np.float64) * GRID == np.stack(us)).all() and (v.astype(np.float64) * GRID == np.stack(vs)).all()   # exact
    return u, v, np.array(ks)


_ROWS = {}
_ORACLE = {}


def rows():
    if not _ROWS:
        _ROWS["rows"] = shifted_rows(N, 1900)
    return _ROWS["rows"]


def shift_oracle(p):
    """float64 minimum, argmin and number of shifts that attain the minimum, per row; computed once per p"""
    if p not in _ORACLE:
        from oracle import exact_shift
        u, v, _ = rows()

        def one(r):
            ks, c = exact_shift.shift_costs(np.sort(u[r].astype(np.float64)), np.sort(v[r].astype(np.float64)), p)
            i = int(np.argmin(c))
            return c[i], ks[i], int((c == c[i]).sum())

        with ThreadPoolExecutor(max_workers=min(8, os.cpu_count() or 1)) as pool:         # numpy releases the GIL
            out = list(pool.map(one, range(u.shape[0])))
        _ORACLE[p] = (np.array([o[0] for o in out]), np.array([o[1] for o in out]), np.array([o[2] for o in out]))
    return _ORACLE[p]


def circle_ot_with_shift(shw, u, v, p):
    """shw_circle_ot (the entry under shw.binary_search_circle) with its aux output: cost and optimal shift per row"""
    lib = shw._lib.load()
    nrows, n = u.shape
    cost = torch.empty(nrows, dtype=torch.float32, device="cuda")
    aux = torch.empty(nrows, dtype=torch.int32, device="cuda")
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    rc = lib.shw_circle_ot(u.data_ptr(), v.data_ptr(), None, None, 0, 0, nrows, n, n, float(p),
                           shw._lib.CIRCLE_BISECTION, cost.data_ptr(), aux.data_ptr(), None, None, stream)
    shw._lib.check(rc, "shw_circle_ot")
    torch.cuda.synchronize()
    return cost.cpu().numpy(), aux.cpu().numpy()


def test_rows_cover_every_alignment():
    """CPU part of the design: the wanted shifts are the issue's, and they reach every body and both sides of every carry"""
    _, _, want = rows()
    assert set(np.abs(want)) == set(KS) and len(want) == 2 * len(KS)
    for sel in (want[want > 0], want[want < 0]):
        assert {int(k - 1) % 4 for k in sel} == {0, 1, 2, 3} and {int(k) % 4 for k in sel} == {0, 1, 2, 3}
        # the first row of the window, (k - 1) mod 32 or k mod 32 (one-shift evaluation): both sides of the wrap 31 | 0
        # and of the multiple of 8 next to it that the wanted shifts straddle (7 | 8 for k* > 0, 23 | 24 for k* < 0)
        first = {int(k - 1) % 32 for k in sel} | {int(k) % 32 for k in sel}
        assert {30, 31, 0, 1} <= first and ({7, 8} <= first if sel[0] >= 0 else {23, 24} <= first)
        for near in (0, 32, 64, N // 2, N - 1):
            assert (np.abs(np.abs(sel) - near) <= 5).any()


@pytest.mark.parametrize("p", [2, 3, 1.5])
def test_shift_and_cost_at_every_alignment(shw, p):
    u, v, want = rows()
    best, arg, ties = shift_oracle(p)
    assert (ties == 1).all(), want[ties != 1]                                             # a unique minimum on every row
    assert (arg == want).all(), (arg[arg != want], want[arg != want])                     # ... at the shift it was built for
    reps = 1024 // len(want) + 1                                                          # more than 1024 rows per launch
    ut = torch.from_numpy(np.tile(u, (reps, 1))).cuda().contiguous()
    vt = torch.from_numpy(np.tile(v, (reps, 1))).cuda().contiguous()
    assert ut.shape[0] > 1024
    cost, shift = circle_ot_with_shift(shw, ut, vt, p)
    exp_cost, exp_shift = np.tile(best, reps), np.tile(arg, reps)
    err = np.abs(cost.astype(np.float64) - exp_cost) / exp_cost
    print(f"p={p}: {ut.shape[0]} rows, largest relative error of the cost {err.max():.3e} (k* {exp_shift[int(err.argmax())]}); "
          f"{int((shift != exp_shift).sum())} of {shift.size} shifts differ from the argmin")
    assert (shift == exp_shift).all(), (exp_shift[shift != exp_shift][:10], shift[shift != exp_shift][:10])
    assert err.max() <= 2e-6, (err.max(), exp_shift[int(err.argmax())])
