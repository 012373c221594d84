"""
_categorical_cases.py — the reference, the data and the case table of the categorical likelihood's tests:
iVAE(..., channels=C, sampler_d="categorical", sigmoid_d=False), enum pv_lik's PV_LIK_CATEGORICAL.

The C values of a position are one observation on the simplex and the decoder's C outputs its logits a:
    log p(x | z) = sum over positions of sum_c x_c (a_c - logsumexp_c a)          (no multinomial coefficient).

The reference.  oracle/ knows the per-value likelihoods only and orc.elbo reaches them through the module global
orc.likelihood, called with the flattened channel-last row.  The fixture `categorical_oracle` below replaces that global for
the duration of a test: for cfg.sampler == "categorical" it returns an object whose log_prob(x) holds the per-value terms
x_c log softmax(a)_c (softmax over the trailing C of every position), and it delegates to the original otherwise.  With
it SVIOracle (and its particles / Renyi / mean-field switches), _pixel_weight_cases.WeightedOracle and
_image_weight_cases.ImageWeightedOracle are the references as they stand, in float64.

Helper modules are not assertion-rewritten: every bare assert carries its tag, value and bar.
"""
import numpy as np
import pytest
import torch

import pyroved_amd as pv
from oracle import svi_oracle as orc
import _multichannel_cases as mc


# ------------------------------------------------------------------------------- the reference likelihood
class ChannelCategorical:
    """log_prob(x): the per-value terms x_c (a_c - logsumexp_c a) in x's shape; the softmax runs over the trailing C values of
    every position of the channel-last row (..., positions * C)."""

    def __init__(self, logits, channels):
        self.shape, self.channels = logits.shape, channels
        self.logp = torch.log_softmax(logits.reshape(*logits.shape[:-1], -1, channels), -1).reshape(logits.shape)

    def log_prob(self, x):
        return x * self.logp


@pytest.fixture
def categorical_oracle(monkeypatch):
    original = orc.likelihood

    def likelihood(cfg, loc):
        if cfg.sampler == "categorical":
            return ChannelCategorical(loc, cfg.channels)
        return original(cfg, loc)
    monkeypatch.setattr(orc, "likelihood", likelihood)
    return likelihood


def probs_of(logits):
    """softmax over the trailing (channel) axis of the reference's logits (n, *dims, C)"""
    return torch.softmax(logits, -1)


# ------------------------------------------------------------------------------- cases
# entries as _multichannel_cases.CASES (model_kwargs / case_config apply), plus  soft: Dirichlet(1, .., 1) rows instead of one-hot
# labels;  routes: "fused" (model.engine(fused_channels=True): pv_sdec_fused_mc_cat_kernel) and / or "layered" (fused=0:
# pv_out_lik_mc_cat_kernel<C>, the vanilla decoder: pv_lik_elem_cat_kernel<C>).  Hidden sizes [128, 128], tanh unless stated.
KIND = dict(sampler="categorical", sigmoid_d=False)
CASES = {
    # 24 units, one per workgroup (fused); 384 rows (layered)
    "k01_8x8_rts_c3_b6": dict(dims=(8, 8), inv=["r", "t", "s"], C=3, b=6, routes=("fused", "layered"), **KIND),
    # one coordinate, the smallest C
    "k02_1d32_t_c2_b5": dict(dims=(32,), inv=["t"], C=2, b=5, routes=("fused", "layered"), **KIND),
    # 2 560 units, 10 per workgroup: a sample boundary inside a workgroup; the widest softmax
    "k03_16x16_r_c8_b160": dict(dims=(16, 16), inv=["r"], C=8, b=160, routes=("fused",), **KIND),
    # [z | y]; soft labels
    "k04_8x8_rt_c4_cdim3_b6_soft": dict(dims=(8, 8), inv=["r", "t"], C=4, b=6, c_dim=3, soft=True, routes=("fused", "layered"), **KIND),
    # 63 positions: no multiple of 16, layered whatever is asked
    "k05_7x9_rt_c3_b3_72_40_softplus": dict(dims=(7, 9), inv=["r", "t"], C=3, b=3, hidden_d=[72, 40], activation="softplus",
                                            routes=("layered",), **KIND),
    # the vanilla decoder: the grouped element-wise kernel
    "k06_8x8_none_c2_b6": dict(dims=(8, 8), inv=None, C=2, b=6, routes=("layered",), **KIND),
    # 784 units on 256 workgroups: images split over workgroups
    "k07_28x28_rt_c3_b16": dict(dims=(28, 28), inv=["r", "t"], C=3, b=16, routes=("fused",), **KIND),
}
CASE1, CASE_VANILLA = "k01_8x8_rts_c3_b6", "k06_8x8_none_c2_b6"
STEP_CELLS = [(name, route) for name in sorted(CASES) for route in CASES[name]["routes"]]
ENGINE_KW = {"fused": dict(fused_channels=True), "layered": dict(fused=0)}
# the stability cell: CASE1 with decoder.out.weight multiplied by this — the seed-1 model's largest |logit| on CASE1's data is
# 0.285, so it reaches ~100 (tests/test_categorical_cpu.py confirms the size); exp of such a logit overflows fp32
STABILITY_SCALE = 350.0


def labels(g, b, dims, C):
    """One-hot label maps (b, *dims, C): the argmax over C of a rand field drawn from g.  The fields of images 1 .. C-1 are image
    0's rolled by 1 .. C-1 along the class axis, so that every (position, class) input is 1 in at least one image of the batch
    (b >= C): with independent fields and six images a third of the classes never occurs at a position, (2/3)^6 = 9 % of the
    encoder's first-layer gradient columns are exactly zero, and check_params_after_adam's 1 % cap on such entries is breached
    by the data, not by the kernel."""
    assert b >= C, "labels: batch %d below the %d classes" % (b, C)
    field = torch.rand(b, *dims, C, generator=g)
    for i in range(1, C):
        field[i] = torch.roll(field[0], i, dims=-1)
    return pv.utils.onehot_channels(field.argmax(-1), C)


def soft_labels(g, b, dims, C):
    """Rows on the simplex, Dirichlet(1, .., 1): normalised exponentials -log(rand) drawn from g."""
    e = -torch.log(torch.rand(b, *dims, C, generator=g).clamp_min(1e-12))
    return e / e.sum(-1, keepdim=True)


def case_data(c, particles=1):
    """(x, y, [eps of step 0, eps of step 1]) from torch.Generator().manual_seed(0): the data first, then the eps draws (each
    (particles * b, z_dim), rows [p][b]); y one-hot rows b % c_dim as in _multichannel_cases.case_data."""
    g = torch.Generator().manual_seed(0)
    x = (soft_labels if c.get("soft") else labels)(g, c["b"], tuple(c["dims"]), c["C"])
    z_dim = mc.case_config(c).z_dim
    eps = [torch.randn(particles * c["b"], z_dim, generator=g) for _ in range(2)]
    y = None
    if c.get("c_dim"):
        y = torch.zeros(c["b"], c["c_dim"])
        y[torch.arange(c["b"]), torch.arange(c["b"]) % c["c_dim"]] = 1.0
    return x, y, eps


def make_model(c, device):
    return pv.models.iVAE(c["dims"], 2, c["inv"], seed=1, device=device, **mc.model_kwargs(c))


# ------------------------------------------------------------------------------- what the GPU tests share
class WithLoc:
    """The engine with loc_out=self.loc added to every loss_and_grads call: _judge.steps_vs_reference then leaves loc to the
    `checks` (its own check_loc compares with the decoder's raw output, which is the logits here, not the probabilities)."""

    def __init__(self, eng, loc):
        self._eng, self.loc = eng, loc

    def __getattr__(self, name):
        return getattr(self._eng, name)

    def loss_and_grads(self, *args, **kw):
        return self._eng.loss_and_grads(*args, loc_out=self.loc, **kw)


def check_probs(loc, logits, tag, rtol=1e-4, atol=2e-6):
    """loc (rows, positions * C) against softmax of the reference's logits at check_loc's bars; rows sum to 1 within 1e-6."""
    C = logits.shape[-1]
    want = probs_of(logits.detach()).reshape(loc.shape[0], -1).numpy()
    got = loc.detach().cpu().numpy()
    sums = got.reshape(got.shape[0], -1, C).sum(-1)
    print("%s: probabilities max abs error %.2e, max |row sum - 1| %.2e" % (tag, np.abs(got - want).max(), np.abs(sums - 1).max()))
    assert np.isfinite(got).all(), "%s: loc has non-finite entries" % tag
    np.testing.assert_allclose(got, want, rtol=rtol, atol=atol, err_msg="%s loc (class probabilities)" % tag)
    np.testing.assert_allclose(sums, 1.0, rtol=0, atol=1e-6, err_msg="%s rows of loc sum to 1" % tag)
