"""
_particles_cases.py — the step cases of the multi-particle ELBO's tests: tests/test_gpu_particles.py runs them,
tests/test_particles_cpu.py confirms with the reference alone the condition their parameter check rests on, and the Renyi
tests (tests/_renyi_cases.py) reuse shapes and seeds.
"""
import torch

from conftest import make_x

import pyroved_amd as pv
from oracle import svi_oracle as orc
from _judge import LR

# name: (data_dim, invariances, model kwargs, B, P) — what each covers is in the comment
STEP_CASES = {
    "8x8_rts_b6_p3": ((8, 8), ["r", "t", "s"], {}, 6, 3),                        # 18 samples: crosses a 16-row block
    "8x8_none_b6_p3": ((8, 8), None, {}, 6, 3),                                  # vanilla decoder (layered whatever `fused`)
    "1d16_t_b5_p7": ((16,), ["t"], {}, 5, 7),                                    # 35 samples, odd everything
    "8x8_rt_cdim3_b6_p2": ((8, 8), ["r", "t"], dict(c_dim=3), 6, 2),             # conditioning
    "16x16_r_gauss_b4_p2": ((16, 16), ["r"], dict(sampler_d="gaussian", sigmoid_d=False), 4, 2),   # Gaussian sampler
}
STEP_SEEDS = dict(model=1, x=0, eps=17)


def oracle_of(kl, params, cfg, P, dtype=torch.float32):
    return orc.SVIOracle(params, cfg, lr=LR, dtype=dtype, kl=kl, particles=P)


def step_case(name, device):
    data_dim, inv, kw, b, P = STEP_CASES[name]
    model = pv.models.iVAE(data_dim, 2, inv, seed=STEP_SEEDS["model"], device=device, **kw)
    cfg = orc.Config(data_dim=data_dim, latent_dim=2, invariances=inv, c_dim=kw.get("c_dim", 0),
                     sampler=kw.get("sampler_d", "bernoulli"), sigmoid_d=kw.get("sigmoid_d", True))
    x = make_x("rand", b, data_dim, seed=STEP_SEEDS["x"])
    y = None
    if cfg.c_dim:
        y = torch.zeros(b, cfg.c_dim)
        y[torch.arange(b), torch.arange(b) % cfg.c_dim] = 1.0
        x = x.flatten(1)
    g = torch.Generator().manual_seed(STEP_SEEDS["eps"])
    eps = [torch.randn(P * b, cfg.z_dim, generator=g) for _ in range(2)]
    return model, cfg, x, y, eps, b, P
