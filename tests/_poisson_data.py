"""
_poisson_data.py — the count data the tests of the Poisson (log link) likelihood, sampler_d="poisson_log", run on, and the
likelihood's formulas restated term by term.  The reference distribution itself is oracle.svi_oracle.likelihood's.

The decoder's output a is the log-rate (sigmoid_d=False).  With a_c = min(a, 30):

    log p(x | a) = x a_c - exp(a_c) - lgamma(x + 1)        = torch.distributions.Poisson(exp(a_c)).log_prob(x)
"""
import torch

CLAMP = 30.0


def log_prob_formula(a, x):
    """The formula the kernels implement, term by term (the kernels leave lgamma(x + 1) to pv_poisson_lognorm)."""
    ac = a.clamp(max=CLAMP)
    return x * ac - torch.exp(ac) - torch.lgamma(x + 1)


def dnll_da_formula(a, x):
    """d(-log p)/da: what autograd gives through the clamp."""
    return (torch.exp(a.clamp(max=CLAMP)) - x) * (a <= CLAMP).to(a.dtype)


def lognorm(x):
    """C = sum lgamma(x + 1) over every image and pixel, float64."""
    return torch.lgamma(x.double() + 1).sum().item()


def rates(centres, dims):
    """rate_b(u) = 1 + 2 exp(-|u - c_b|^2 / 0.18), u on linspace(-1, 1, d) per axis."""
    axes = [torch.linspace(-1.0, 1.0, d) for d in dims]
    mesh = torch.meshgrid(*axes, indexing="ij")
    d2 = 0.0
    for i, m in enumerate(mesh):
        d2 = d2 + (m.unsqueeze(0) - centres[:, i].reshape(-1, *([1] * len(dims)))) ** 2
    return 1.0 + 2.0 * torch.exp(-d2 / 0.18)


def counts(g, batch, dims):
    """`batch` count images on `dims` from generator g: the centres c_b = rand - 0.5 per axis first, then torch.poisson(rate).
    The caller draws its eps from the same generator afterwards."""
    c = torch.rand(batch, len(dims), generator=g) - 0.5
    return torch.poisson(rates(c, tuple(dims)), generator=g)
