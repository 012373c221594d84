"""
_renyi_cases.py — the cases of the importance-weighted (Renyi / IWAE) bound's tests, the two float64 references every step
is judged by (the bound with free weights, and the step with the engine's weights held) and the bar on the weights.
tests/test_gpu_renyi.py states how the bars compose; tests/test_renyi_cpu.py confirms the cases' conditions.
"""
import numpy as np
import torch

from conftest import load_golden, make_x, meta_of

import pyroved_amd as pv
from oracle import svi_oracle as orc
from _judge import LR, state
from _particles_cases import STEP_CASES, STEP_SEEDS, step_case

BETA = 1.7
ALPHAS = (0.0, 0.5)
CASES = dict(STEP_CASES)
CASES["28x28_r_b128_p2"] = None          # the ivae_28x28_r_b128 fixture's data with P = 2 (throughput precision only)


def case_inputs(name, device):
    """(cfg, parameters on the CPU, x, y, [eps of step 0, eps of step 1], B, P, beta) — what tests/test_renyi_cpu.py checks the
    condition on and every GPU test runs; `model` rides along as the ninth item."""
    if name in STEP_CASES:
        model, cfg, x, y, eps, b, P = step_case(name, device)
    else:
        meta = meta_of(load_golden("ivae_28x28_r_b128"))
        assert meta["batch"] == 128
        b, P = meta["batch"], 2
        model = pv.models.iVAE(meta["data_dim"], 2, meta["invariances"], seed=STEP_SEEDS["model"], device=device)
        cfg = orc.Config(data_dim=tuple(meta["data_dim"]), latent_dim=2, invariances=meta["invariances"])
        x, y = make_x(meta["xkind"], b, meta["data_dim"]), None
        g = torch.Generator().manual_seed(STEP_SEEDS["eps"])
        eps = [torch.randn(P * b, cfg.z_dim, generator=g) for _ in range(2)]
    return cfg, state(model), x, y, eps, b, P, BETA, model


def weight_check(tag, w_gpu, ref, alpha, ll_bar):
    """max |log w - log w_ref| over entries with w_ref > 1e-6 against 2 |1 - alpha| ll_bar max_s |ll_s|; printed first."""
    w_ref, logw_ref = ref["weights"].detach().double(), ref["log_weights"].detach().double()
    keep = w_ref > 1e-6
    got = torch.log(w_gpu.double().cpu())[keep]
    err = (got - logw_ref[keep]).abs().max().item()
    bar = 2.0 * abs(1.0 - alpha) * ll_bar * ref["ll_per_sample"].detach().abs().max().item()
    print("%s: max |log w - log w_ref| %.3e (bar %.3e) over %d of %d weights" % (tag, err, bar, int(keep.sum()), keep.numel()))
    assert err <= bar, "%s: log-weights %.3e from the reference (bar %.3e)" % (tag, err, bar)
    sums = w_gpu.double().cpu().view(-1, ref["z_loc"].shape[0]).sum(0)
    np.testing.assert_allclose(sums.numpy(), 1.0, rtol=0, atol=1e-6)


def free_and_held(params, cfg, P, alpha, x, eps, beta, y, w_gpu, held=None):
    """The float64 reference twice: the bound itself (free weights) from `params`, and the oracle `held` (made from `params`
    when not given: it carries Adam's state from step to step) that takes the Adam step on the gradient with the engine's
    weights held."""
    free = orc.SVIOracle(params, cfg, lr=LR, dtype=torch.float64, particles=P, renyi=alpha)
    of = free.loss_and_grads(x, eps, beta, y)
    g_free = {k: v.grad.detach().clone() for k, v in free.p.items()}
    if held is None:
        held = orc.SVIOracle(params, cfg, lr=LR, dtype=torch.float64, particles=P, renyi=alpha)
    held.weights = w_gpu.detach().cpu().double()
    held.step(x, eps, beta, y)
    return of, g_free, held
