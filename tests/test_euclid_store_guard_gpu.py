"""GPU test (`-m gpu`, MI355X) of the one coefficient store site of the Euclidean sliced-W forward kernels
(csrc/euclid_common.hpp, euclid_forward): a row that holds a NaN key stores nothing past its n coefficients.

A positive NaN key orders after the +inf padding keys, so in a size class that pads (n = 70: 2 keys per lane, 58 pads) a
sorted position below n then holds a pad, whose index lies between n and 127.  A store at that index lands in the next
row's coefficients or, for the last row, behind the buffer.  The C entries are called with buffers this test owns: each
coefficient buffer is one tensor of rows * n + 128 floats filled with a sentinel, so an overflow stays inside it.

  the 128 floats behind the last row are untouched;
  every row of pair 0 (sums and both coefficient rows) equals a run without the NaN bit for bit;
  the sums of the last pair, which holds the NaN, are NaN.

n = 128 fills its class (no pads, no pad index to store at) and holds for any build; n = 70 is the case the guard is
for: without it shw_esw_forward and shw_esw_forward_dim write the sentinel's first float."""

import pytest
import torch

pytestmark = pytest.mark.gpu

PAIRS, SLICES, TAIL = 2, 3, 128
SENTINEL = -12345.0
ROWS = PAIRS * SLICES


@pytest.fixture(scope="module")
def lib():
    import shw_amd
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return shw_amd._lib.load()


def positive_nan():
    return torch.tensor(0x7FC00000, dtype=torch.int32).view(torch.float32).item()


def inputs(entry, n):
    """(source, target, directions) on the device; `source` is (PAIRS, n, D) clouds or (ROWS, n) keys."""
    g = torch.Generator().manual_seed(29)
    if entry == "gsw_rows":
        return torch.randn(ROWS, n, generator=g).cuda(), torch.randn(ROWS, n, generator=g).cuda(), None
    D = 5 if entry == "esw_dim" else 3
    th = torch.nn.functional.normalize(torch.randn(SLICES, D, generator=g), dim=-1)
    return torch.randn(PAIRS, n, D, generator=g).cuda(), torch.randn(PAIRS, n, D, generator=g).cuda(), th.cuda()


def run(lib, entry, n, p, src, dst, th):
    """-> sums (ROWS,), the two coefficient buffers (ROWS * n + TAIL,) as the entry left them."""
    sums = torch.full((ROWS,), SENTINEL, device="cuda")
    ca = torch.full((ROWS * n + TAIL,), SENTINEL, device="cuda")
    cb = torch.full((ROWS * n + TAIL,), SENTINEL, device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    a, b, s = src.data_ptr(), dst.data_ptr(), sums.data_ptr()
    if entry == "esw":
        rc = lib.shw_esw_forward(a, b, th.data_ptr(), PAIRS, n, SLICES, 0, p, s, ca.data_ptr(), cb.data_ptr(), st)
    elif entry == "esw_dim":
        rc = lib.shw_esw_forward_dim(a, b, th.data_ptr(), PAIRS, n, src.shape[-1], SLICES, 0, p, s, ca.data_ptr(),
                                     cb.data_ptr(), st)
    elif entry == "gsw_circular":
        rc = lib.shw_gsw_circular_forward(a, b, th.data_ptr(), PAIRS, n, src.shape[-1], SLICES, 0, 1.0, p, s,
                                          ca.data_ptr(), cb.data_ptr(), st)
    else:
        rc = lib.shw_gsw_rows_forward(a, b, ROWS, n, p, s, ca.data_ptr(), cb.data_ptr(), st)
    assert rc == 0, rc
    torch.cuda.synchronize()
    return sums, ca, cb


def same_bits(x, y):
    return torch.equal(x.view(torch.int32), y.view(torch.int32))


@pytest.mark.parametrize("n", [70, 128])
@pytest.mark.parametrize("p", [2.0, 1.5])
@pytest.mark.parametrize("entry", ["esw", "esw_dim", "gsw_circular", "gsw_rows"])
def test_a_nan_key_stores_nothing_past_its_row(lib, entry, p, n):
    src, dst, th = inputs(entry, n)
    clean = run(lib, entry, n, p, src, dst, th)
    bad = src.clone()
    if entry == "gsw_rows":
        bad[SLICES * (PAIRS - 1):, 7] = positive_nan()       # the keys of one source point on every slice of the last pair
    else:
        bad[PAIRS - 1, 7, 1] = positive_nan()                # one coordinate of one source point of the last pair
    sums, ca, cb = run(lib, entry, n, p, bad, dst, th)

    first = SLICES * n                                       # pair 0: rows 0 .. SLICES - 1
    for name, got, want in (("coef_a", ca, clean[1]), ("coef_b", cb, clean[2])):
        tail = got[ROWS * n:]
        touched = (tail.view(torch.int32) != torch.full_like(tail, SENTINEL).view(torch.int32)).nonzero().flatten().tolist()
        assert not touched, f"{name}: floats {touched} behind the last row were written: {tail[touched].tolist()}"
        assert same_bits(got[:first], want[:first]), f"{name}: pair 0 differs from the run without the NaN"
    assert same_bits(sums[:SLICES], clean[0][:SLICES]), "the sums of pair 0 differ from the run without the NaN"
    assert torch.isnan(sums[SLICES * (PAIRS - 1):]).all(), sums.tolist()
    assert torch.isfinite(clean[0]).all(), clean[0].tolist()
