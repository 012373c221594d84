"""
_multichannel_cases.py — the data and the case table the tests of multi-channel models, iVAE(..., channels=C), run on.  The
reference itself is oracle.svi_oracle with Config(channels=C): x is (B, *data_dim, C), channel-last.
"""
import numpy as np
import torch

from oracle import svi_oracle as orc


# ------------------------------------------------------------------------------- data
def _bumps(g, batch, dims, C):
    """exp(-d^2 / 0.18) around a centre per (image, channel), rand - 0.5 per axis, on linspace(-1, 1) axes: (batch, C, *dims);
    and the amplitudes 0.5 + 0.4 c / (C - 1), shaped to broadcast."""
    cen = torch.rand(batch, C, len(dims), generator=g) - 0.5
    mesh = torch.meshgrid(*[torch.linspace(-1.0, 1.0, d) for d in dims], indexing="ij")
    d2 = 0.0
    for i, m in enumerate(mesh):
        d2 = d2 + (m.reshape(1, 1, *dims) - cen[:, :, i].reshape(batch, C, *([1] * len(dims)))) ** 2
    amp = 0.5 + 0.4 * torch.arange(C, dtype=torch.float32) / max(C - 1, 1)
    return torch.exp(-d2 / 0.18), amp.reshape(1, C, *([1] * len(dims)))


def _channel_last(t):
    return t.permute(0, *range(2, t.dim()), 1).contiguous()


def images(g, batch, dims, C):
    """(batch, *dims, C) in (0, 1): x = 0.05 + amp_c exp(-d^2 / 0.18).  The channels differ in centre and amplitude, so an
    implementation that swaps or merges channels cannot pass.  The caller draws its eps from g afterwards."""
    e, amp = _bumps(g, batch, tuple(dims), C)
    return _channel_last(0.05 + amp * e)


def counts(g, batch, dims, C):
    """(batch, *dims, C) Poisson counts of rate 1 + 2 amp_c exp(-d^2 / 0.18)."""
    e, amp = _bumps(g, batch, tuple(dims), C)
    return _channel_last(torch.poisson(1.0 + 2.0 * amp * e, generator=g))


# ------------------------------------------------------------------------------- the GPU tests' cases
# (tests/test_gpu_multichannel.py runs them; tests/test_multichannel_cpu.py confirms, with the reference alone, the condition
#  its parameter check rests on).  Hidden sizes [128, 128] unless stated; no lrelu / relu decoder: their exact zeros of the
#  activation's derivative put ~7 % of a gradient tensor's entries under the near-zero threshold, above the 1 % cap.
CASES = {
    "c01_8x8_rts_c2_b6": dict(dims=(8, 8), inv=["r", "t", "s"], C=2, b=6),                                  # 384 rows: whole workgroups
    "c02_7x9_rt_c3_b3_gauss_nosig_72_40_softplus": dict(dims=(7, 9), inv=["r", "t"], C=3, b=3, sampler="gaussian",
                                                        sigmoid_d=False, hidden_d=[72, 40], activation="softplus"),
    "c03_1d16_t_c4_b5_gelu": dict(dims=(16,), inv=["t"], C=4, b=5, activation="gelu"),
    "c04_8x8_r_c3_b6_poisson": dict(dims=(8, 8), inv=["r"], C=3, b=6, sampler="poisson_log", sigmoid_d=False),
    "c05_4x4_r_c8_b2_512_512": dict(dims=(4, 4), inv=["r"], C=8, b=2, hidden_d=[512, 512]),
    "c06_8x8_rts_c2_cdim3_b6": dict(dims=(8, 8), inv=["r", "t", "s"], C=2, b=6, c_dim=3),
    "c07_6x6_r_c5_b4_softplus": dict(dims=(6, 6), inv=["r"], C=5, b=4, activation="softplus"),
    "c08_6x6_r_c7_b4_gauss": dict(dims=(6, 6), inv=["r"], C=7, b=4, sampler="gaussian"),
    "c09_6x6_r_c6_b4_cbern": dict(dims=(6, 6), inv=["r"], C=6, b=4, sampler="continuous_bernoulli"),
    "c10_28x28_rt_c3_b16": dict(dims=(28, 28), inv=["r", "t"], C=3, b=16),                                  # 12 544 rows, 196 workgroups
    "c11_8x8_none_c2_b6": dict(dims=(8, 8), inv=None, C=2, b=6),                                            # vanilla decoder
}


def model_kwargs(c):
    """models.iVAE keyword arguments of a case."""
    kw = dict(channels=c["C"], c_dim=c.get("c_dim", 0), activation=c.get("activation", "tanh"),
              sampler_d=c.get("sampler", "bernoulli"), sigmoid_d=c.get("sigmoid_d", True))
    if "hidden_d" in c:
        kw["hidden_dim_d"] = list(c["hidden_d"])
    return kw


def case_config(c):
    return orc.Config(data_dim=tuple(c["dims"]), latent_dim=2, invariances=c["inv"], channels=c["C"], c_dim=c.get("c_dim", 0),
                      activation=c.get("activation", "tanh"), sampler=c.get("sampler", "bernoulli"),
                      sigmoid_d=c.get("sigmoid_d", True))


def case_data(c, particles=1):
    """(x, y, [eps of step 0, eps of step 1]) from torch.Generator().manual_seed(0): the data first, then the eps draws
    (each (particles * b, z_dim), rows [p][b])."""
    g = torch.Generator().manual_seed(0)
    make = counts if c.get("sampler") == "poisson_log" else images
    x = make(g, c["b"], c["dims"], c["C"])
    z_dim = case_config(c).z_dim
    eps = [torch.randn(particles * c["b"], z_dim, generator=g) for _ in range(2)]
    y = None
    if c.get("c_dim"):
        y = torch.zeros(c["b"], c["c_dim"])
        y[torch.arange(c["b"]), torch.arange(c["b"]) % c["c_dim"]] = 1.0
    return x, y, eps


def loss_atol(c):
    """test_model_variants_vs_oracle: 1e-6 per value of the batch for the continuous Bernoulli, none otherwise."""
    return 1e-6 * c["b"] * int(np.prod(c["dims"])) if c.get("sampler") == "continuous_bernoulli" else 0.0


def round_to_float32(o):
    """Both sides of a step test continue from the SAME float32 parameters."""
    with torch.no_grad():
        for v in o.p.values():
            v.copy_(v.float().to(v.dtype))
