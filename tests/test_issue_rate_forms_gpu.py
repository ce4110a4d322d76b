"""The full classes of the loss kernels: fix-up loop, placement addresses, shift fetches, sign of the angle (`-m gpu`).

These tests pin results that the instruction forms of round 8 must not alter; they pass on the parent too.

1. test_chain_on_every_lane_boundary: permuted twins in coordinate-row mode (shw.binary_search_circle, more than 1024
   rows per launch, so the throughput kernels run).  The target row is the source row permuted, so two exact sorts give
   cost exactly 0.0 (tests/test_fixup_exact_gpu.py has the argument).  Every row has ONE bin that holds a chain of g
   adjacent floats, g in 4 .. 12, 39, 40 (g mod 4 = 0, 1, 2, 3: whole trips of the four-phase loop and every
   remainder), and every other bin holds two keys or one (g - 2 bins hold one, so that the row has n keys): the longest
   equal-bin run of the row -- the number of phases the kernel runs -- is exactly g, which numpy asserts with the bin
   map of the class.  The chain lies across the boundary between lanes j - 1 and j of the read-back, for every
   j = 1 .. 63 in turn (rows of 16 lanes meet at 15|16, 31|32, 47|48), with 1 .. g - 1 of its keys in front of the
   boundary; or it is the row's smallest keys (sorted position 0, lane 0), or its largest (ending at position n - 1,
   lane 63): the two lanes that have no neighbour on one side.  n = 2048 (one wave per slice), 1024 and 512 (two waves).

2. test_shift_fetch_arithmetic: rows of n distinct multiples of 2^-20 inside an arc of 1/16 of the circle, target =
   (source + delta) mod 1 with delta a multiple of 2^-20: every value and every difference is exact in float32.  With
   delta = 1 - (the K-th largest source value) exactly K target values wrap around, and the optimal shift is k* = K
   (delta < 1/2, arc in [0.7, 0.7625)) or k* = -K (delta > 1/2: delta = 1 - the K-th smallest value, arc in
   [0.2, 0.2625)); every term of that matching is delta or 1 - delta.  The K are chosen so that (k* - 1) mod 32, the row
   the window of the fetch starts in, takes the values 0, 1, 15, 30, 31, with |k*| near 0, 32, n / 2 and n - 1 (the turn and
   column-wrap paths), for both signs.  The CPU oracle (oracle/exact_shift.shift_costs, float64, all 2 n + 1 shifts)
   gives the expected cost and argmin of every distinct row inside the test; its minimum must be unique and at the k*
   the row was built for.  GPU: cost within 2e-6 relative of the float64 minimum (the inputs are exact, so the bound is
   tighter than the suite's 2e-5 per slice) and the shift shw_circle_ot returns equal to the argmin.  p = 2 (three-cost
   and one-cost evaluations) and p = 3 (the general-power kernel).

3. test_projections_on_the_axes: projection mode, B L = 1152 slices, clouds that hold (+-1, 0, 0), (0, +-1, 0),
   (0, 0, +-1) and the all-zero point, frames that include the axis-aligned ones of both signs: for those slices
   a = 0 or b = 0 exactly, with either sign of the other component.  Permuted twin: cost 0.0 and shift 0 on every
   slice; an independent target: per-slice cost against oracle/ref_mirror.per_slice_costs (rtol 5e-5, atol 1e-9, the
   tolerance of tests/test_ssw_gpu.py for ssw_pair_losses) on the axis-aligned slices and some others.
"""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

CHAINS = (4, 5, 6, 7, 8, 9, 10, 11, 12, 39, 40)


@pytest.fixture(scope="module")
def shw():
    import shw_amd
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    shw_amd._lib.load()
    return shw_amd


# ---- 1 ----------------------------------------------------------------------------------------------------------------
def bin_of(key, n):
    """bin of the byte-offset map of the full class of n keys (csrc/bin_sort.hpp, binsort_off<n / 2>)"""
    nb = n // 2
    t = (np.asarray(key, dtype=np.float64) * (4.0 * nb - 1.0) + 8388608.0).astype(np.float32)   # one rounding, as the FMA
    return (t.view(np.uint32) & np.uint32(4 * nb - 4)) >> np.uint32(2)


def chain_row(rng, n, g, place):
    """n float32 keys: a chain of g adjacent floats alone in its bin, sorted positions c0 .. c0 + g - 1; two keys or one
    in every other bin.  place = j in 1 .. 63: c0 < (n / 64) j < c0 + g;  'first': c0 = 0;  'last': c0 = n - g.
    Returns (row in sorted order, c0)."""
    nb, ept = n // 2, n // 64
    scale = 4.0 * nb - 1.0
    if place == "first":
        c0 = 0
    elif place == "last":
        c0 = n - g
    else:
        edge = ept * place
        lim = 1 + (place + g) % (g - 1)                        # keys of the chain in front of the boundary
        lim = min(max(lim, g - (n - edge)), min(g - 1, edge))   # ... the chain fits into the row
        c0 = edge - lim
        assert c0 >= 0 and c0 + g <= n and c0 < edge < c0 + g
    # the chain's bin b has c0 smaller keys: two per bin below it less the `low` bins that hold one; g - 2 single bins in all
    singles = g - 2
    low = [t for t in range(singles + 1) if (c0 + t) % 2 == 0 and t <= (c0 + t) // 2 and singles - t <= nb - 1 - (c0 + t) // 2]
    assert low, (n, g, place)
    low = low[int(rng.integers(len(low)))]
    b = (c0 + low) // 2
    count = np.full(nb, 2)
    count[rng.choice(b, size=low, replace=False)] = 1
    count[b + 1 + rng.choice(nb - 1 - b, size=singles - low, replace=False)] = 1
    count[b] = 0
    bins = np.repeat(np.arange(nb), count)
    lo = np.maximum(4.0 * bins - 0.3, 0.0)
    hi = np.minimum(4.0 * bins + 3.3, scale)
    rest = ((lo + (hi - lo) * rng.random(bins.size)) / scale).astype(np.float32)
    c = np.float32((4.0 * b + 1.5) / scale)
    chain = c + np.arange(g, dtype=np.float32) * np.spacing(c)
    assert (np.diff(chain.view(np.int32)) == 1).all()                                    # adjacent floats
    row = np.sort(np.concatenate([rest, chain]))
    assert row.size == n and row.min() >= 0 and row.max() <= 1
    assert (row[c0:c0 + g] == chain).all()
    return row, c0


def chain_rows(n, seed):
    rng = np.random.default_rng(seed)
    rows, built = [], []
    for rep in range(2):                                          # 2 x 11 x 65 = 1430 rows: more than 1024
        for g in CHAINS:
            for place in list(range(1, 64)) + ["first", "last"]:
                row, c0 = chain_row(rng, n, g, place)
                counts = np.bincount(bin_of(row, n), minlength=n // 2)
                assert counts.max() == g and (counts == g).sum() == 1, (n, g, place, counts.max())
                assert np.unique(bin_of(row[c0:c0 + g], n)).size == 1
                rows.append(row[rng.permutation(n)])
                built.append((g, place, c0))
    return np.stack(rows), built


@pytest.mark.parametrize("n", [2048, 1024, 512])
def test_chain_on_every_lane_boundary(shw, n):
    u, built = chain_rows(n, 8100 + n)
    ept = n // 64
    assert u.shape[0] > 1024
    assert {g for g, _, _ in built} == set(CHAINS)                                       # every trip shape is a row's run
    for j in range(1, 64):                                                                # every boundary, by every chain
        assert {g for g, place, c0 in built if place == j and c0 < ept * j < c0 + g} == set(CHAINS)
    assert {g for g, place, c0 in built if place == "first" and c0 == 0} == set(CHAINS)
    assert {g for g, place, c0 in built if place == "last" and c0 + g == n} == set(CHAINS)
    rng = np.random.default_rng(8200 + n)
    v = np.stack([row[rng.permutation(n)] for row in u])
    got = shw.binary_search_circle(torch.from_numpy(u).cuda(), torch.from_numpy(v).cuda(), p=2).cpu().numpy()
    bad = np.nonzero(got != 0)[0]
    print(f"n={n}, rows {u.shape[0]}: {bad.size} costs are not 0.0 (largest {np.abs(got).max():.3e}); "
          f"first bad rows (g, place, c0): {[built[i] for i in bad[:10]]}")
    assert got.shape == (u.shape[0],)
    assert bad.size == 0, ([built[i] for i in bad[:10]], got[bad[:10]])


# ---- 2 ----------------------------------------------------------------------------------------------------------------
N2 = 2048
GRID = 1 << 20
# (k* - 1) mod 32 of k* = K:  0, 1, 15, 30, 31 | 0 | 30;   of k* = -K:  30, 15, 1, 0, 31 | 31 | 0
# (fourteen rows: the oracle takes a quarter of a second per row)
K_POS = (1, 2, 16, 31, 32, 1025, 2047)
K_NEG = (1, 16, 30, 31, 32, 1024, 2047)

def shifted_rows(seed):
    """(u, v, k) of one row per wanted shift: u = N2 distinct multiples of 2^-20 in an arc of 1/16, v = (u + delta) mod 1"""
    rng = np.random.default_rng(seed)
    us, vs, ks = [], [], []
    for sign, wanted in ((1, K_POS), (-1, K_NEG)):
        for K in wanted:
            start = int((0.7 if sign > 0 else 0.2) * GRID)
            ticks = np.sort(start + rng.choice(GRID // 16, size=N2, replace=False))        # integers: coordinates * 2^20
            if sign > 0:
                d = GRID - ticks[N2 - K] if K > 0 else GRID // 5                            # exactly K values reach 1 and wrap
            else:
                d = GRID - ticks[K] if K < N2 else GRID - ticks[N2 - 1] - 1                 # exactly N2 - K values wrap
            moved = (ticks + d) % GRID
            assert np.unique(moved).size == N2 and int((ticks + d >= GRID).sum()) == (K if sign > 0 else N2 - K)
            assert (2 * d < GRID) == (sign > 0)
            us.append(ticks[rng.permutation(N2)])
            vs.append(moved[rng.permutation(N2)])
            ks.append(sign * K)
    u = (np.stack(us).astype(np.float64) / GRID).astype(np.float32)
    v = (np.stack(vs).astype(np.float64) / GRID).astype(np.float32)
    assert (u.astype(np.float64) * GRID == np.stack(us)).all() and (v.astype(np.float64) * GRID == np.stack(vs)).all()   # exact
    return u, v, np.array(ks)


_ORACLE = {}


def shift_oracle(p):
    """the rows with the float64 minimum and argmin of every row, computed once per p (the rows never change)"""
    if p not in _ORACLE:
        from oracle import exact_shift
        u, v, want = shifted_rows(8300)
        best, arg = np.empty(len(want)), np.empty(len(want), dtype=np.int64)
        for r in range(len(want)):
            ks, c = exact_shift.shift_costs(np.sort(u[r].astype(np.float64)), np.sort(v[r].astype(np.float64)), p)
            i = int(np.argmin(c))
            assert (c == c[i]).sum() == 1, (r, want[r])                                   # a unique minimum
            best[r], arg[r] = c[i], ks[i]
        _ORACLE[p] = (u, v, want, best, arg)
    return _ORACLE[p]


def circle_ot_with_shift(shw, u, v, p):
    """shw_circle_ot (the entry under shw.binary_search_circle) with its aux output: cost and optimal shift per row"""
    lib = shw._lib.load()
    rows, n = u.shape
    cost = torch.empty(rows, dtype=torch.float32, device="cuda")
    aux = torch.empty(rows, dtype=torch.int32, device="cuda")
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    rc = lib.shw_circle_ot(u.data_ptr(), v.data_ptr(), None, None, 0, 0, rows, n, n, float(p),
                           shw._lib.CIRCLE_BISECTION, cost.data_ptr(), aux.data_ptr(), None, None, stream)
    shw._lib.check(rc, "shw_circle_ot")
    torch.cuda.synchronize()
    return cost.cpu().numpy(), aux.cpu().numpy()


@pytest.mark.parametrize("p", [2, 3])
def test_shift_fetch_arithmetic(shw, p):
    u, v, want, best, arg = shift_oracle(p)
    assert (arg == want).all(), (arg, want)                                               # the rows do what they were built for
    res = {int((k - 1) % 32) for k in arg}
    assert {0, 1, 15, 30, 31} <= res
    assert {0, 1, 15, 30, 31} <= {int((k - 1) % 32) for k in arg if k > 0} and {0, 1, 15, 30, 31} <= {int((k - 1) % 32) for k in arg if k < 0}
    for near in (0, 32, N2 // 2, N2 - 1):
        assert (np.abs(arg[arg > 0] - near) <= 16).any() and (np.abs(-arg[arg < 0] - near) <= 16).any()
    reps = 1040 // len(want)                                                              # 74 x 14 rows: more than 1024 per launch
    ut = torch.from_numpy(np.tile(u, (reps, 1))).cuda().contiguous()
    vt = torch.from_numpy(np.tile(v, (reps, 1))).cuda().contiguous()
    assert ut.shape[0] > 1024
    cost, shift = circle_ot_with_shift(shw, ut, vt, p)
    api = shw.binary_search_circle(ut, vt, p=p).cpu().numpy()
    exp_cost, exp_shift = np.tile(best, reps), np.tile(arg, reps)
    err = np.abs(cost.astype(np.float64) - exp_cost) / exp_cost
    print(f"p={p}: largest relative error of the cost {err.max():.3e} (row {int(err.argmax())}, k* {exp_shift[int(err.argmax())]}); "
          f"{int((shift != exp_shift).sum())} of {shift.size} shifts differ from the argmin")
    assert (api == cost).all()
    assert (shift == exp_shift).all(), (np.nonzero(shift != exp_shift)[0][:10], shift[shift != exp_shift][:10])
    assert err.max() <= 2e-6, (err.max(), exp_shift[int(err.argmax())])


# ---- 3 ----------------------------------------------------------------------------------------------------------------
def axis_frames():
    """(3, 2) frames whose columns are signed unit vectors of two different axes: 6 x 4 = 24 of them"""
    out = []
    for i in range(3):
        for j in range(3):
            if i != j:
                for si in (1.0, -1.0):
                    for sj in (1.0, -1.0):
                        f = np.zeros((3, 2), dtype=np.float32)
                        f[i, 0], f[j, 1] = si, sj
                        out.append(f)
    return np.stack(out)


def axis_cloud(gen, n):
    x = torch.nn.functional.normalize(torch.randn(n, 3, generator=gen), dim=-1)
    special = torch.tensor([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1], [0, 0, 0]], dtype=torch.float32)
    where = torch.randperm(n, generator=gen)[:special.shape[0]]
    x[where] = special
    return x


def test_projections_on_the_axes(shw):
    from oracle import ref_mirror
    B, L, n = 3, 384, 2048
    g = torch.Generator().manual_seed(8400)
    x = torch.stack([axis_cloud(g, n) for _ in range(B)])
    twin = torch.stack([x[b][torch.randperm(n, generator=g)] for b in range(B)])
    y = torch.stack([axis_cloud(g, n) for _ in range(B)])
    U = torch.linalg.qr(torch.randn(B, L, 3, 2, generator=g))[0]
    frames = torch.from_numpy(axis_frames())
    at = torch.arange(frames.shape[0]) * 16 + 5                                           # spread over the launch
    U[:, at] = frames
    a = torch.einsum("bnd,bld->bln", x, U[..., 0])
    b_ = torch.einsum("bnd,bld->bln", x, U[..., 1])
    for sel in (a, b_):                                                                   # exact zeros beside both signs
        other = b_ if sel is a else a
        assert ((sel == 0) & (other > 0)).any() and ((sel == 0) & (other < 0)).any() and ((sel == 0) & (other == 0)).any()
    _, cost, shift = shw.ssw_pair_losses(x.cuda(), twin.cuda(), U.cuda(), p=2, return_slices=True)
    cost, shift = cost.cpu().numpy(), shift.cpu().numpy()
    print(f"twins: {int((cost != 0).sum())} of {cost.size} slice costs are not 0.0, {int((shift != 0).sum())} shifts are not 0")
    assert cost.shape == (B, L)
    assert (cost == 0).all(), (np.argwhere(cost != 0)[:5], cost[cost != 0][:5])
    assert (shift == 0).all(), (np.argwhere(shift != 0)[:5], shift[shift != 0][:5])
    _, cost, _ = shw.ssw_pair_losses(x.cuda(), y.cuda(), U.cuda(), p=2, return_slices=True)
    cost = cost.cpu().numpy()
    check = torch.cat([at, torch.tensor([0, 1, L - 1])])
    ref = ref_mirror.per_slice_costs(x[0], y[0], U[0, check], p=2).numpy()
    err = np.abs(cost[0, check.numpy()] - ref) / ref
    print(f"per-slice costs of {check.numel()} slices against the reference: largest relative error {err.max():.3e}")
    assert np.allclose(cost[0, check.numpy()], ref, rtol=5e-5, atol=1e-9)
