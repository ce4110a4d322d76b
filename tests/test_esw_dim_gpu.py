"""GPU tests (`-m gpu`, MI355X) of the Euclidean sliced-W kernels for point dimension D in 1..64 and of the notebooks'
ASWD baseline (`augmented_sliced_wassersten_distance`) built on them.

  the D-generic kernels against the float64 restatement (oracle/euclid_sw.py): slice sums, gradients w.r.t. both
  clouds and the directions, shared and per-pair directions;
  the new C entry at D = 3 against the R^3 kernels it generalises;
  bit-identical gradients from run to run;
  ASWD against fixture G11 (tests/golden/g11_notebook_aswd.npz, tools/make_golden_aswd.py: the notebook cell exec'd
  on the CPU) -- value, gradient, phi after the ascent, five steps of the notebook's flow loop;
  the CPU-generator direction stream of the D-generic call shape.
Tolerances are stated at each assertion.
"""

import numpy as np
import pytest
import torch

from helpers.compare import grad_close

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def shw():
    import shw_amd
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    shw_amd._lib.load()
    return shw_amd


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda")


def rel(a, b):
    a = np.asarray(a, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    return float(np.max(np.abs(a - b) / np.maximum(np.abs(b), 1e-30)))


def clouds(gen, B, n, D):
    return torch.randn(B, n, D, generator=gen), torch.randn(B, n, D, generator=gen) * 0.7 + 0.2


def directions(shw, B, L, D, per_pair):
    if per_pair:
        return torch.stack([shw.rand_projections(D, L) for _ in range(B)])
    return shw.rand_projections(D, L)


class Mapping(torch.nn.Module):
    """the notebooks' phi (Flow_cube.ipynb, the `def rand_projections` cell): x -> cat(x, Linear(x))"""

    def __init__(self, size, W=None, b=None):
        super().__init__()
        self.size = size
        self.net = torch.nn.Sequential(torch.nn.Linear(size, size))
        if W is not None:
            with torch.no_grad():
                self.net[0].weight.copy_(torch.as_tensor(W))
                self.net[0].bias.copy_(torch.as_tensor(b))

    def forward(self, inputs):
        return torch.cat((inputs, self.net(inputs)), dim=-1)


# ------------------------------------------------------------------------------------------- against the restatement
@pytest.mark.parametrize("D", [1, 2, 4, 6, 10, 21, 64])
@pytest.mark.parametrize("n", [1, 64, 1200, 4096])
@pytest.mark.parametrize("p", [1, 2, 3])
@pytest.mark.parametrize("B,per_pair", [(1, False), (3, True), (3, False)])
def test_slice_sums_and_gradients_against_the_float64_restatement(shw, D, n, p, B, per_pair):
    """Slice sums 2e-5 relative, as the D = 3 test (plus 1e-6 of the largest sum absolute: a key is a D-term fp32 dot
    product, so its rounding error is absolute, and a lone sorted difference near zero has no relative accuracy);
    gradients w.r.t. both clouds within 5e-4 of the largest entry (the D = 3 test's bound, with grad_close's near-tie
    allowance); gradients w.r.t. the directions 1e-3, a sum over n points of fp32 products."""
    from oracle import euclid_sw
    g = torch.Generator().manual_seed(7000 + 97 * D + n + 13 * p + B)
    L = 8
    a, b = clouds(g, B, n, D)
    torch.manual_seed(7100 + D + n + p)
    th = directions(shw, B, L, D, per_pair)
    xa, xb, tg = a.cuda().requires_grad_(True), b.cuda().requires_grad_(True), th.cuda().requires_grad_(True)
    sums = shw.esw_slice_sums(xa, xb, tg, p)
    ad, bd, td = (t.double().requires_grad_(True) for t in (a, b, th))
    ref = torch.stack([euclid_sw.slice_sums(ad[k], bd[k], td[k] if per_pair else td, p) for k in range(B)])
    got = sums.detach().cpu().numpy()
    want = ref.detach().numpy()
    assert np.allclose(got, want, rtol=2e-5, atol=1e-6 * np.abs(want).max() + 1e-12), rel(got, want)
    w = torch.rand(B, L, generator=g) + 0.5
    (sums * w.cuda()).sum().backward()
    (ref * w.double()).sum().backward()
    assert xa.grad.shape == (B, n, D) and tg.grad.shape == th.shape
    if p > 1 or n > 1:
        grad_close(xa.grad.cpu().numpy(), ad.grad.numpy(), strict=5e-4)
        grad_close(xb.grad.cpu().numpy(), bd.grad.numpy(), strict=5e-4)
        grad_close(tg.grad.cpu().numpy(), td.grad.numpy(), strict=1e-3)


def test_limits_raise_value_errors_that_name_them(shw):
    x = torch.zeros(1, 8, 65, device="cuda")
    with pytest.raises(ValueError, match="1 to 64"):
        shw.esw_slice_sums(x, x, torch.zeros(4, 65, device="cuda"))
    x = torch.zeros(1, 8, 0, device="cuda")
    with pytest.raises(ValueError, match="1 to 64"):
        shw.esw_slice_sums(x, x, torch.zeros(4, 0, device="cuda"))
    x = torch.zeros(1, 4097, 6, device="cuda")
    with pytest.raises(ValueError, match="4096"):
        shw.esw_slice_sums(x, x, torch.zeros(4, 6, device="cuda"))
    with pytest.raises(ValueError):                          # unequal clouds, as the notebook cell requires
        shw.esw_slice_sums(torch.zeros(1, 8, 6, device="cuda"), torch.zeros(1, 9, 6, device="cuda"),
                           torch.zeros(4, 6, device="cuda"))
    with pytest.raises(TypeError):                           # directions of another dimension
        shw.esw_slice_sums(torch.zeros(1, 8, 6, device="cuda"), torch.zeros(1, 8, 6, device="cuda"),
                           torch.zeros(4, 5, device="cuda"))


# ------------------------------------------------------------------------------------------- new entry at D = 3
@pytest.mark.parametrize("n,p,per_pair", [(1200, 2, False), (4096, 1, True), (64, 3, False), (700, 2, True)])
def test_new_entry_at_d3_matches_the_r3_kernels(shw, n, p, per_pair):
    """The D-generic kernels at D = 3 form the same keys (x0*t0, then fma in coordinate order), the same sort and the
    same fixed-order reductions as the R^3 kernels: slice sums within fp32 rounding (1e-6 relative) and gradients
    within 1e-5 of the largest entry, every entry."""
    lib = shw._lib.load()
    g = torch.Generator().manual_seed(8000 + n + p)
    B, L, D = 2, 24, 3
    a, b = clouds(g, B, n, D)
    torch.manual_seed(8100 + n)
    th = directions(shw, B, L, D, per_pair).cuda().contiguous()
    xs, xt = a.cuda().contiguous(), b.cuda().contiguous()
    w = (torch.rand(B, L, generator=g) + 0.5).cuda().contiguous()
    stride = L * D if per_pair else 0
    stream = torch.cuda.current_stream().cuda_stream
    out = {}
    for tag in ("r3", "dim"):
        sums = torch.empty(B * L, device="cuda")
        cs, ct = torch.empty(B * L * n, device="cuda"), torch.empty(B * L * n, device="cuda")
        gxs, gxt = torch.empty(B, n, D, device="cuda"), torch.empty(B, n, D, device="cuda")
        gth = torch.empty(B, L, D, device="cuda")
        if tag == "r3":
            rcs = [lib.shw_esw_forward(xs.data_ptr(), xt.data_ptr(), th.data_ptr(), B, n, L, stride, float(p),
                                       sums.data_ptr(), cs.data_ptr(), ct.data_ptr(), stream),
                   lib.shw_esw_backward_points(th.data_ptr(), cs.data_ptr(), ct.data_ptr(), w.data_ptr(), B, n, L,
                                               stride, gxs.data_ptr(), gxt.data_ptr(), stream),
                   lib.shw_esw_backward_dirs(xs.data_ptr(), xt.data_ptr(), cs.data_ptr(), ct.data_ptr(), w.data_ptr(),
                                             B, n, L, gth.data_ptr(), stream)]
        else:
            rcs = [lib.shw_esw_forward_dim(xs.data_ptr(), xt.data_ptr(), th.data_ptr(), B, n, D, L, stride, float(p),
                                           sums.data_ptr(), cs.data_ptr(), ct.data_ptr(), stream),
                   lib.shw_esw_backward_points_dim(th.data_ptr(), cs.data_ptr(), ct.data_ptr(), w.data_ptr(), B, n, D,
                                                   L, stride, gxs.data_ptr(), gxt.data_ptr(), stream),
                   lib.shw_esw_backward_dirs_dim(xs.data_ptr(), xt.data_ptr(), cs.data_ptr(), ct.data_ptr(),
                                                 w.data_ptr(), B, n, D, L, gth.data_ptr(), stream)]
        assert rcs == [0, 0, 0], (tag, rcs)
        torch.cuda.synchronize()
        out[tag] = [t.cpu().numpy() for t in (sums, gxs, gxt, gth)]
    assert np.allclose(out["dim"][0], out["r3"][0], rtol=1e-6, atol=0)
    for got, want in zip(out["dim"][1:], out["r3"][1:]):
        grad_close(got, want, strict=1e-5, exact=True)


# ------------------------------------------------------------------------------------------- determinism
@pytest.mark.parametrize("D", [6, 21])
def test_gradients_are_bit_identical_from_run_to_run(shw, D):
    g = torch.Generator().manual_seed(9000 + D)
    B, n, L = 3, 1200, 100
    a, b = clouds(g, B, n, D)
    torch.manual_seed(9100 + D)
    th = directions(shw, B, L, D, True)
    w = (torch.rand(B, L, generator=g) + 0.5).cuda()
    runs = []
    for _ in range(2):
        xa, xb, tg = a.cuda().requires_grad_(True), b.cuda().requires_grad_(True), th.cuda().requires_grad_(True)
        sums = shw.esw_slice_sums(xa, xb, tg, 2)
        (sums * w).sum().backward()
        runs.append([t.detach().cpu() for t in (sums, xa.grad, xb.grad, tg.grad)])
    for first, second in zip(*runs):
        assert torch.equal(first, second)


# ------------------------------------------------------------------------------------------- ASWD against G11
def _run_case(shw, g, name):
    phi = Mapping(3, g["phi_weight0"], g["phi_bias0"]).cuda()
    phi_op = torch.optim.Adam(phi.parameters(), lr=0.005, betas=(0.999, 0.999))
    first = dev(g["source"]).requires_grad_(True)
    target = dev(g["target"])
    lam = 0.05 / target.abs().mean()                    # the notebook's lam, from the device target
    torch.manual_seed(int(g[f"{name}_seed"]))
    val = shw.augmented_sliced_wassersten_distance(first, target, int(g[f"{name}_L"]), phi, phi_op,
                                                   p=float(g[f"{name}_p"]), max_iter=int(g[f"{name}_max_iter"]),
                                                   lam=lam, device="cuda", net_type="fc")
    W, b = phi.net[0].weight.detach().cpu().numpy(), phi.net[0].bias.detach().cpu().numpy()
    val.backward()
    return val, first.grad.cpu().numpy(), W, b, phi


def test_g11_aswd_final_evaluation_against_the_notebook_cell(shw, golden):
    """max_iter = 0: the final evaluation alone, on the directions the cell drew from the stored seed.  Value 1e-5
    relative; gradient w.r.t. the first cloud (through phi and the D' = 6 kernels) 2e-4 of the largest entry, as the G9
    test, with the count of entries outside that bound pinned."""
    g = golden("g11_notebook_aswd.npz")
    val, grad, W, b, phi = _run_case(shw, g, "it0_p2")
    assert rel(val.item(), g["it0_p2_value"]) < 1e-5
    grad_close(grad, g["it0_p2_grad_first"], strict=2e-4, max_outside=0)
    assert np.array_equal(W, g["phi_weight0"]) and np.array_equal(b, g["phi_bias0"])     # no ascent step
    assert phi.net[0].weight.grad is not None and torch.isfinite(phi.net[0].weight.grad).all()


@pytest.mark.parametrize("name", ["it10_p2", "it3_p1"])
def test_g11_aswd_with_the_phi_ascent_against_the_notebook_cell(shw, golden, name):
    """The notebook's call (max_iter = 10, lam = 0.05 / target.abs().mean()) and a p = 1 case.  Value 1e-4 relative,
    as the G9 max-sliced test.  phi after the call within 1e-4 absolute: every Adam step (betas (0.999, 0.999)) moves
    a parameter by lr * m_hat / sqrt(v_hat), a ratio of smoothed gradients that does not depend on their scale, so a
    relative gradient difference d between fp32-on-GPU and the cell moves a parameter by about lr * d per step; ten
    steps at lr = 0.005 with d <= 1e-3 stay below 5e-5."""
    g = golden("g11_notebook_aswd.npz")
    val, grad, W, b, _ = _run_case(shw, g, name)
    assert rel(val.item(), g[f"{name}_value"]) < 1e-4
    assert np.abs(W - g[f"{name}_phi_weight"]).max() < 1e-4
    assert np.abs(b - g[f"{name}_phi_bias"]).max() < 1e-4
    grad_close(grad, g[f"{name}_grad_first"], strict=2e-4, max_outside=0)


def test_g11_aswd_flow_trace_against_the_notebook_loop(shw, golden):
    """Five outer steps of the notebook's ASWD flow loop (Adam lr 0.01 on the evolving cloud, phi's own Adam inside
    every call): the loss per step 1e-4 relative, as the G10 flow test; the final cloud as there -- Adam moves every
    point by about lr per step whatever the gradient's size, so at most 8 coordinates (near-zero gradients whose sign
    can differ) may be more than 2 lr off and the median difference stays below 1e-4."""
    g = golden("g11_notebook_aswd.npz")
    lr = float(g["flow_lr"])
    target = dev(g["target"])
    lam = 0.05 / target.abs().mean()
    phi = Mapping(3, g["phi_weight0"], g["phi_bias0"]).cuda()
    phi_op = torch.optim.Adam(phi.parameters(), lr=0.005, betas=(0.999, 0.999))
    evolving = dev(g["source"]).requires_grad_(True)
    optimizer = torch.optim.Adam([evolving], lr=lr, betas=(0.9, 0.999))
    torch.manual_seed(int(g["flow_seed"]))
    trace = []
    for _ in range(len(g["flow_trace"])):
        optimizer.zero_grad()
        loss = shw.augmented_sliced_wassersten_distance(evolving, target, 100, phi, phi_op, p=2, max_iter=10, lam=lam,
                                                        device="cuda", net_type="fc")
        loss.backward(retain_graph=True)
        optimizer.step()
        trace.append(loss.item())
    assert rel(trace, g["flow_trace"]) < 1e-4
    moved = np.abs(evolving.detach().cpu().numpy() - g["flow_evolved"])
    assert (moved > 2 * lr).sum() <= 8 and np.median(moved) < 1e-4
    assert np.abs(phi.net[0].weight.detach().cpu().numpy() - g["flow_phi_weight"]).max() < 1e-3


def test_g11_directions_are_the_cells_draws_and_the_alias_is_the_same_function(shw, golden):
    """The eleven draws of the notebook's call, from the stored seed.  1e-6 relative, not bit equality: torch's CPU
    randn and sqrt are vectorised by the host's instruction set, and hosts differ in the last bits."""
    g = golden("g11_notebook_aswd.npz")
    torch.manual_seed(int(g["it10_p2_seed"]))
    drawn = np.stack([shw.rand_projections(6, 100).numpy() for _ in range(11)])
    assert np.allclose(drawn, g["it10_p2_thetas"], rtol=1e-6, atol=1e-7)
    assert shw.augmented_sliced_wasserstein_distance is shw.augmented_sliced_wassersten_distance


# ------------------------------------------------------------------------------------------- random-number parity
@pytest.mark.parametrize("D,L", [(6, 100), (2, 30), (21, 50)])
def test_call_shape_draws_the_cells_directions(shw, D, L):
    """Under torch.manual_seed, sliced_wasserstein_distance on (1200, D) clouds equals the restatement on
    rand_projections(D, L) drawn from the same seed: 1e-5 relative."""
    from oracle import euclid_sw
    g = torch.Generator().manual_seed(9500 + D)
    a, b = torch.randn(1200, D, generator=g), torch.randn(1200, D, generator=g) * 0.6 + 0.3
    torch.manual_seed(31 + D)
    val = shw.sliced_wasserstein_distance(a.cuda(), b.cuda(), num_projection=L, p=2, device="cuda")
    torch.manual_seed(31 + D)
    th = shw.rand_projections(D, L)
    ref = euclid_sw.sliced_wasserstein_distance(a.double(), b.double(), th.double(), 2)
    assert val.dim() == 0 and abs(val.item() - ref.item()) < 1e-5 * ref.item()


def test_max_sliced_w_ascends_on_a_six_dimensional_direction(shw):
    """max_sliced_wasserstein_distance at D = 6 (the direction gradient of the D-generic kernel): the same 25 Adam ascent
    steps run on the float64 restatement from the same starting direction land on the same value, 1e-3 relative."""
    from oracle import euclid_sw
    g = torch.Generator().manual_seed(9600)
    a, b = torch.randn(400, 6, generator=g), torch.randn(400, 6, generator=g) * 0.6 + 0.3
    torch.manual_seed(5)
    d1 = shw.max_sliced_wasserstein_distance(a.cuda(), b.cuda(), p=2, max_iter=25, device="cuda").item()
    torch.manual_seed(5)
    proj = shw.rand_projections(6, 1).double().requires_grad_(True)
    opt = torch.optim.Adam([proj], lr=0.005, betas=(0.999, 0.999))
    for _ in range(25):
        d = torch.pow(euclid_sw.slice_sums(a.double(), b.double(), proj, 2).mean(), 0.5)
        opt.zero_grad()
        (-d).backward()
        opt.step()
        proj.data = proj.data / torch.sqrt(torch.sum(proj.data ** 2, dim=1))
    ref = torch.pow(euclid_sw.slice_sums(a.double(), b.double(), proj.detach(), 2).mean(), 0.5).item()
    assert abs(d1 - ref) < 1e-3 * ref
