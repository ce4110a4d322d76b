"""Torch restatement of the generalised sliced-Wasserstein family (GSWD, max-GSWD, gsw_nn, DSWD), differentiable through
autograd.  It runs in whatever dtype its inputs have: float64 is the reference of the GPU tests, and the same code in
float32 on the CPU measures how far float32 arithmetic alone moves a result (the basis of any tolerance that is not one
of the Euclidean kernels' own).  Written from the definitions: a key per (slice, point), both key rows sorted, the sum
of |sorted difference|^p, then (mean over slices)^(1/p)."""
from itertools import combinations

import torch


def sorted_row_sums(u, v, p):
    """(..., n), (..., n) -> (...)"""
    du = torch.sort(u, dim=-1).values - torch.sort(v, dim=-1).values
    return du.abs().pow(p).sum(-1)


def outer(sums, p):
    return sums.mean().pow(1.0 / p)


# ------------------------------------------------------------------------------------------------ defining functions
def circular_keys(X, thetas, r):
    """(n, D), (L, D) -> (L, n): | x_i - r theta_l |_2"""
    diff = X.unsqueeze(0) - (thetas * r).unsqueeze(1)
    return diff.pow(2).sum(-1).sqrt()


def circular_slice_sums(Xs, Xt, thetas, r, p):
    """(B,n,D), (B,n,D), (L,D) or (B,L,D) -> (B,L)"""
    out = []
    for b in range(Xs.shape[0]):
        th = thetas[b] if thetas.dim() == 3 else thetas
        out.append(sorted_row_sums(circular_keys(Xs[b], th, r), circular_keys(Xt[b], th, r), p))
    return torch.stack(out)


def monomial_exponents(degree, dim):
    """all exponent vectors of total degree `degree` in `dim` variables: stars and bars, bars in lexicographic order"""
    rows = []
    for bars in combinations(range(degree + dim - 1), dim - 1):
        prev, row = -1, []
        for b in bars + (degree + dim - 1,):
            row.append(b - prev - 1)
            prev = b
        rows.append(row)
    return torch.tensor(rows, dtype=torch.float64)


def polynomial_keys(X, coefficient, degree):
    """(n, D), (F, L) -> (L, n): sum_f coefficient[f, l] prod_d x_d ^ e_fd"""
    e = monomial_exponents(degree, X.shape[-1]).to(X.dtype)
    feats = (X.unsqueeze(1) ** e.unsqueeze(0)).prod(-1)
    return (feats @ coefficient).transpose(0, 1)


def linear_keys(X, thetas):
    """(n, D), (L, D) -> (L, n)"""
    return thetas @ X.transpose(0, 1)


def unit_columns(c):
    return c / c.pow(2).sum(0).sqrt()


# ------------------------------------------------------------------------------------------------ the family
def gswd_circular(a, b, theta, r, p):
    return outer(sorted_row_sums(circular_keys(a, theta, r), circular_keys(b, theta, r), p), p)


def gswd_polynomial(a, b, raw_coefficient, degree, p):
    c = unit_columns(raw_coefficient)
    return outer(sorted_row_sums(polynomial_keys(a, c, degree), polynomial_keys(b, c, degree), p), p)


def _adam(params):
    return torch.optim.Adam(params, lr=0.005, betas=(0.999, 0.999))


def max_gswd_circular(a, b, theta0, r, p, max_iter):
    """theta0 (1, D), already of unit length.  Returns (value, final theta)."""
    theta = theta0.clone().requires_grad_(True)
    opt = _adam([theta])
    ad, bd = a.detach(), b.detach()
    for _ in range(max_iter):
        opt.zero_grad()
        (-gswd_circular(ad, bd, theta, r, p)).backward()
        opt.step()
        with torch.no_grad():
            theta.copy_(theta / theta.pow(2).sum(1).sqrt())
    theta = theta.detach()
    return gswd_circular(a, b, theta, r, p), theta


def max_gswd_polynomial(a, b, raw_coefficient, degree, p, max_iter):
    """raw_coefficient (F, 1), the draw before normalisation.  Returns (value, final coefficient)."""
    c = unit_columns(raw_coefficient).clone().requires_grad_(True)
    opt = _adam([c])
    ad, bd = a.detach(), b.detach()
    for _ in range(max_iter):
        opt.zero_grad()
        (-outer(sorted_row_sums(polynomial_keys(ad, c, degree), polynomial_keys(bd, c, degree), p), p)).backward()
        opt.step()
        with torch.no_grad():
            c.copy_(unit_columns(c))
    c = c.detach()
    return outer(sorted_row_sums(polynomial_keys(a, c, degree), polynomial_keys(b, c, degree), p), p), c


def gsw_nn(a, b, net, p):
    return outer(sorted_row_sums(net(a).transpose(0, 1), net(b).transpose(0, 1), p), p)


def max_gsw_nn(a, b, net, net_op, max_iter, p):
    ad, bd = a.detach(), b.detach()
    for _ in range(max_iter):
        net_op.zero_grad()
        (-gsw_nn(ad, bd, net, p)).backward()
        net_op.step()
    return gsw_nn(a, b, net, p)


def cosine_spread(x, eps=1e-8):
    """mean_ij | cos(x_i, x_j) |"""
    w = x.norm(dim=1, keepdim=True)
    return ((x @ x.t()) / (w * w.t()).clamp(min=eps)).abs().mean()


def dswd(a, b, draws, f, f_op, p, max_iter, lam):
    """draws: (max_iter + 1, L, D), the unit directions of the ascent steps and of the final evaluation, in order."""
    ad, bd = a.detach(), b.detach()
    for it in range(max_iter):
        dirs = f(draws[it])
        loss = lam * cosine_spread(dirs) - outer(sorted_row_sums(linear_keys(ad, dirs), linear_keys(bd, dirs), p), p)
        f_op.zero_grad()
        loss.backward()
        f_op.step()
    dirs = f(draws[max_iter])
    return outer(sorted_row_sums(linear_keys(a, dirs), linear_keys(b, dirs), p), p)


# ------------------------------------------------------------------------------------------------ the caller's modules
class UnitLinear(torch.nn.Module):
    """x -> Linear(x) / |Linear(x)| (the role of the notebooks' TransformNet)"""

    def __init__(self, size, weight=None, bias=None, dtype=torch.float32):
        super().__init__()
        self.net = torch.nn.Sequential(torch.nn.Linear(size, size, dtype=dtype))
        if weight is not None:
            with torch.no_grad():
                self.net[0].weight.copy_(torch.as_tensor(weight))
                self.net[0].bias.copy_(torch.as_tensor(bias))

    def forward(self, x):
        out = self.net(x)
        return out / out.pow(2).sum(1, keepdim=True).sqrt()


class SmallMLP(torch.nn.Module):
    """`depth` Linear + LeakyReLU layers of `width`, then a Linear to `dout` (the role of the notebooks' MLP);
    parameters in the order weight, bias per layer"""

    def __init__(self, din, dout, width, depth, params=None, dtype=torch.float32):
        super().__init__()
        layers, w = [], din
        for _ in range(depth):
            layers += [torch.nn.Linear(w, width, dtype=dtype), torch.nn.LeakyReLU()]
            w = width
        layers.append(torch.nn.Linear(w, dout, dtype=dtype))
        self.features = torch.nn.Sequential(*layers)
        if params is not None:
            with torch.no_grad():
                for mine, given in zip(self.parameters(), params):
                    mine.copy_(torch.as_tensor(given))

    def forward(self, x):
        return self.features(x)
