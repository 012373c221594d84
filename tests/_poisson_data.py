"""
_poisson_data.py — the count data the tests of the Poisson (log link) likelihood, sampler_d="poisson_log", run on, and the
likelihood's formulas restated term by term.  The reference distribution itself is oracle.svi_oracle.likelihood's.

The decoder's output a is the log-rate (sigmoid_d=False).  With a_c = min(a, 30):

    log p(x | a) = x a_c - exp(a_c) - lgamma(x + 1)        = torch.distributions.Poisson(exp(a_c)).log_prob(x)
"""
import torch

import pyroved_amd as pv
from oracle import svi_oracle as orc

CLAMP = 30.0
KW = dict(sampler_d="poisson_log", sigmoid_d=False)          # the models' keywords


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


def config(dims, inv, **kw):
    return orc.Config(data_dim=tuple(dims), latent_dim=2, invariances=inv, sampler="poisson_log", sigmoid_d=False, **kw)


# ------------------------------------------------------------------------------- the fp32-class step cases
# (tests/test_gpu_poisson.py runs them; tests/test_poisson_cpu.py confirms, with the reference alone, the condition its parameter
#  check rests on): the smallest shapes at which each code path differs
STEP_CASES = {
    "8x8_rts_b6": dict(dims=(8, 8), inv=["r", "t", "s"], b=6),
    "8x8_none_b6": dict(dims=(8, 8), inv=None, b=6),                       # the layered path and pv_lik_elem
    "1d16_t_b5": dict(dims=(16,), inv=["t"], b=5),
    "16x16_r_b4": dict(dims=(16, 16), inv=["r"], b=4),
    "12x20_rts_b6": dict(dims=(12, 20), inv=["r", "t", "s"], b=6),         # non-square
    "8x8_rt_cdim3_b6": dict(dims=(8, 8), inv=["r", "t"], b=6, c_dim=3),
    "28x28_rt_b16": dict(dims=(28, 28), inv=["r", "t"], b=16),             # more than one tile per workgroup plus the tail
    "jivae_8x8_rt_k3_b6": dict(dims=(8, 8), inv=["r", "t"], b=6, K=3),     # enumerated classes
    "jivae_8x8_none_k3_b6_sampled": dict(dims=(8, 8), inv=None, b=6, K=3, sampled=True),   # the drawn class (vanilla decoder)
}


def step_case(name, device):
    """(model, cfg, x, y, [eps of step 0, eps of step 1], B); y: None, the conditioning one-hot, or (sampled class) the two
    steps' drawn classes."""
    c = STEP_CASES[name]
    dims, inv, b, K, c_dim = c["dims"], c["inv"], c["b"], c.get("K", 0), c.get("c_dim", 0)
    if K:
        model = pv.models.jiVAE(dims, 2, K, inv, seed=1, device=device, **KW)
    else:
        model = pv.models.iVAE(dims, 2, inv, c_dim=c_dim, seed=1, device=device, **KW)
    cfg = config(dims, inv, c_dim=c_dim, discrete_dim=K)
    g = torch.Generator().manual_seed(0)
    x = counts(g, b, dims)
    eps = [torch.randn(b, cfg.z_dim, generator=g) for _ in range(2)]
    y = None
    if c_dim:
        y = torch.zeros(b, c_dim)
        y[torch.arange(b), torch.arange(b) % c_dim] = 1.0
        x = x.flatten(1)
    if c.get("sampled"):
        y = []
        for _ in range(2):
            oh = torch.zeros(b, K)
            oh[torch.arange(b), torch.randint(0, K, (b,), generator=g)] = 1.0
            y.append(oh)
    return model, cfg, x, y, eps, b
