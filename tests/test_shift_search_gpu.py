"""Shift search of the loss kernels on slices where it has to travel (`-m gpu`, MI355X).

On independent uniform clouds the first guess k0 = round(sum u - sum v) is almost always the optimal shift, so the
search takes one or two evaluations.  Here the source is uniform on the sphere and the target lies on a spherical cap:
its circle coordinates bunch on part of the circle and k* - k0 is several steps, so the search gallops and bisects,
and takes unit steps in both directions.  The per-slice costs and shifts are compared with the exhaustive float64
argmin over every shift (oracle/exact_shift.py).  N = 2048 runs the one-wave loss kernel (enough slices to stay off
the small-grid kernels), N = 2000 the two-wave one; a target of 64-fold duplicate points has equal-bin runs longer than
any the distribution sort fixes up, so that slice sorts with the network instead.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

B, L = 3, 384                  # 1152 (pair, slice) problems: more than the small-grid limit of 1024
CHECKED = [(b, l) for b in range(B) for l in (0, 97, 191, 300, 383)]


@pytest.fixture(scope="module")
def shw():
    import shw_amd
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    shw_amd._lib.load()
    return shw_amd


def unit_cloud(gen, n):
    return torch.nn.functional.normalize(torch.randn(n, 3, generator=gen), dim=-1)


def cap_cloud(gen, n, zmin, distinct=None):
    """n points with z > zmin; with `distinct`, that many different points, each repeated n / distinct times."""
    k = distinct or n
    pts = []
    while sum(len(p) for p in pts) < k:
        x = unit_cloud(gen, 4 * k)
        pts.append(x[x[:, 2] > zmin])
    x = torch.cat(pts)[:k]
    return x.repeat_interleave(n // k, dim=0) if distinct else x


@pytest.mark.parametrize("n,p,zmin,distinct", [
    (2048, 2, 0.0, None),
    (2048, 2, 0.8, None),
    (2048, 3, 0.5, None),
    (2000, 2, 0.5, None),
    (2048, 2, 0.5, 32),
])
def test_shift_search_travels_to_exact_argmin(shw, n, p, zmin, distinct):
    from oracle import exact_shift
    g = torch.Generator().manual_seed(9100 + n + int(10 * zmin) + (distinct or 0) + 7 * p)
    x = torch.stack([unit_cloud(g, n) for _ in range(B)])
    y = torch.stack([cap_cloud(g, n, zmin, distinct) for _ in range(B)])
    U = torch.linalg.qr(torch.randn(B, L, 3, 2, generator=g))[0]
    _, cost, shift = shw.ssw_pair_losses(x.cuda(), y.cuda(), U.cuda(), p=p, return_slices=True)
    cost, shift = cost.cpu().numpy(), shift.cpu().numpy()
    tol = 2e-5 if p == 2 else 4e-5
    travel = []
    for b, l in CHECKED:
        cu = exact_shift.circle_coords(x[b].numpy(), U[b, l:l + 1].numpy())[0]
        cv = exact_shift.circle_coords(y[b].numpy(), U[b, l:l + 1].numpy())[0]
        ks, c = exact_shift.shift_costs(np.sort(cu), np.sort(cv), p)
        j = int(np.argmin(c))
        travel.append(abs(int(ks[j]) - int(np.rint(cu.sum() - cv.sum()))))
        assert abs(cost[b, l] - c[j]) <= tol * c[j], (b, l, cost[b, l], c[j])
        # the same shift, or one whose exact cost ties with the minimum to fp32 accuracy
        k = int(shift[b, l])
        assert -n <= k <= n, (b, l, k)
        assert k == ks[j] or c[k + n] <= c[j] * (1 + tol), (b, l, k, int(ks[j]), c[k + n], c[j])
    # the data does what the test is for: the search has to leave its first guess, by several steps
    assert max(travel) >= 4 and sum(t >= 2 for t in travel) >= len(travel) // 2, travel
