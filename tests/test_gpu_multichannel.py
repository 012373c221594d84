"""
GPU tests (-m gpu) of multi-channel models: iVAE(..., channels=C), x of shape (B, *data_dim, C), the spatial decoder's output
layer Linear(H, C) on the C-output likelihood kernel (pv_out_lik_mc) of the layer-by-layer path.

The reference is the project's own float64 oracle (oracle.svi_oracle) with Config(channels=C).  Cases, data and eps come from
tests/_multichannel_cases.CASES / case_data (torch.Generator().manual_seed(0): data first, then the eps draws).  Every step
case runs two steps with Adam between, each from identical float32 parameters (tests/_judge.py: steps_vs_reference), at the
project's bars for the fp32-class paths: loss and ll 2e-5 (+ the atol test_model_variants_vs_oracle gives the sampler), the KL scalars 1e-4, every gradient tensor
1e-4 relative L2, parameters after Adam by check_params_after_adam's rule with the 5e-5 bar (its 1 % cap is confirmed with
the reference alone in tests/test_multichannel_cpu.py), z_loc / z_scale rtol 1e-4 atol 5e-6, loc_out and decode rtol 1e-4
atol 2e-6.
"""
import numpy as np
import pytest
import torch

import pyroved_amd as pv
from oracle import svi_oracle as orc
import _multichannel_cases as mc
from _judge import (RTOL_ELBO, RTOL_KL, LR, state, reload, check_scalars, check_z, check_grads, check_params_after_adam,
                    steps_vs_reference, cpu_threads_16)
from _renyi_cases import weight_check

pytestmark = pytest.mark.gpu

Z_ATOL_MC = 5e-6           # z_loc / z_scale's atol in these tests (encode's bar in tests/test_gpu_parity.py)
CASE1 = "c01_8x8_rts_c2_b6"


def make(name, **engine_kw):
    c = mc.CASES[name]
    model = pv.models.iVAE(c["dims"], 2, c["inv"], seed=1, device="cuda", **mc.model_kwargs(c))
    return c, model, model.engine(**engine_kw)


def run_steps(name, fused, make_oracle, engine_kw=None, particles=1):
    c, model, eng = make(name, fused=fused, **(engine_kw or {}))
    b, n_obs = c["b"], int(np.prod(c["dims"])) * c["C"]
    assert eng.uses_fused(b) is False and eng.supports_dp_step is False
    x, y, eps = mc.case_data(c, particles)
    o = make_oracle(state(model), mc.case_config(c))
    loc = torch.full((particles * b, n_obs), float("nan"), device="cuda")
    steps_vs_reference(eng, model, o, x, y, eps, 1.0, "%s fused=%d" % (name, fused), 0, Z_ATOL_MC, atol=mc.loss_atol(c),
                       loc_out=loc)                                # (0: the 5e-5 bar after Adam)
    return c, model, eng, o, x, y


# ------------------------------------------------------------------------------- 1. steps
STEP_PARAMS = [(n, 2) for n in sorted(mc.CASES)] + [(CASE1, 0)]


@pytest.mark.parametrize("name,fused", STEP_PARAMS)
def test_steps_vs_reference(gpu_device, name, fused):
    """Two steps per case with the default request fused = 2 (it falls back to the layered kernels), and fused = 0 on case 1;
    then encode and decode from the trained state."""
    c, model, eng, o, x, y = run_steps(name, fused, lambda p, cfg: orc.SVIOracle(p, cfg, lr=LR, dtype=torch.float64))
    shape = (c["b"],) + tuple(c["dims"]) + (c["C"],)
    enc_args = (x,) if y is None else (x, y)
    z_loc, z_scale = model.encode(*enc_args)
    zl, zs = o.encode(x, y)
    np.testing.assert_allclose(z_loc.numpy(), zl.numpy(), rtol=1e-4, atol=5e-6)
    np.testing.assert_allclose(z_scale.numpy(), zs.numpy(), rtol=1e-4, atol=5e-6)
    zc = z_loc[:, -2:] if c["inv"] else z_loc
    dec = model.decode(zc, y)
    assert tuple(dec.shape) == shape
    want = o.decode(zc, y, rate=True)
    print("%s: decode max abs error %.2e" % (name, (dec.double() - want).abs().max().item()))
    np.testing.assert_allclose(dec.numpy(), want.numpy(), rtol=1e-4, atol=2e-6)


def test_both_requests_run_the_same_launches(gpu_device):
    """fused = 0 and the default fused = 2 on case 1: the same path, so the same bits."""
    out = []
    for fused in (0, 2):
        c, model, eng = make(CASE1, fused=fused)
        x, y, eps = mc.case_data(c)
        eng.loss_and_grads(x.cuda(), eps[0].cuda(), 1.0)
        torch.cuda.synchronize()
        out.append(eng.grad.clone())
    assert torch.equal(out[0], out[1])


def test_elbo_terms_and_manifold(gpu_device):
    c, model, eng = make(CASE1)
    x, y, eps = mc.case_data(c)
    o = orc.SVIOracle(state(model), mc.case_config(c), dtype=torch.float64)
    with torch.no_grad():
        ref = orc.elbo(o.p, o.cfg, x.double(), eps[0].double(), 1.0, None, o.grid)
    t = model.elbo_terms(x, eps=eps[0])
    np.testing.assert_allclose(t["loss"], ref["loss"].item(), rtol=RTOL_ELBO)
    np.testing.assert_allclose(t["ll"], ref["ll"].item(), rtol=RTOL_ELBO)
    man = model.manifold2d(3, plot=False)
    assert tuple(man.shape) == (9, 8, 8, 2)
    with pytest.raises(ValueError, match="channels"):
        eng.loss_and_grads(x.permute(0, 3, 1, 2).contiguous().cuda(), eps[0].cuda())      # channel-first: refused, not reshaped


# ------------------------------------------------------------------------------- 2. the other objectives, on case 1's shape
def test_analytic_kl_steps(gpu_device):
    run_steps(CASE1, 2, lambda p, cfg: orc.SVIOracle(p, cfg, lr=LR, dtype=torch.float64, kl="analytic"), dict(kl="analytic"))


def test_three_particles_steps(gpu_device):
    run_steps(CASE1, 2, lambda p, cfg: orc.SVIOracle(p, cfg, lr=LR, dtype=torch.float64, particles=3), dict(particles=3), particles=3)


def test_renyi_steps_with_the_weights_held(gpu_device):
    """RenyiELBO(alpha = 0, num_particles = 3), as tests/test_gpu_renyi.py tests the bound: scalars and weights against the free
    float64 bound, gradients and the Adam step against the reference with the engine's weights held."""
    P, alpha = 3, 0.0
    c, model, eng = make(CASE1, fused=2, particles=P, renyi=alpha)
    b = c["b"]
    x, y, eps = mc.case_data(c, P)
    zl, zs = torch.empty(b, model.z_dim, device="cuda"), torch.empty(b, model.z_dim, device="cuda")
    w = torch.full((P * b,), float("nan"), device="cuda")
    held = None
    for k in range(2):
        tag = "renyi step %d" % k
        eng.loss_and_grads(x.cuda(), eps[k].cuda(), 1.0, z_out=(zl, zs), weights_out=w)
        torch.cuda.synchronize()
        free = orc.SVIOracle(state(model), mc.case_config(c), lr=LR, dtype=torch.float64, particles=P, renyi=alpha)
        of = free.loss_and_grads(x, eps[k], 1.0)
        if held is None:
            held = orc.SVIOracle(state(model), mc.case_config(c), lr=LR, dtype=torch.float64, particles=P, renyi=alpha)
        held.weights = w.detach().cpu().double()
        held.step(x, eps[k], 1.0)
        weight_check(tag, w, of, alpha, RTOL_ELBO)
        check_scalars(eng.scalars.cpu().numpy(), of, tag)
        check_z(zl, zs, of, RTOL_KL, Z_ATOL_MC, tag)
        check_grads(eng, held, tag)
        eng.adam_step()
        check_params_after_adam(model, held, 0, tag)
        reload(model, held, round32=True)


# ------------------------------------------------------------------------------- 3. determinism
@pytest.mark.parametrize("name", [CASE1, "c05_4x4_r_c8_b2_512_512", "c10_28x28_rt_c3_b16"])
def test_repeated_call_is_bit_identical(gpu_device, name):
    c, model, eng = make(name)
    x, y, eps = mc.case_data(c)
    xg, eg = x.cuda(), eps[0].cuda()
    eng.loss_and_grads(xg, eg, 1.0)
    torch.cuda.synchronize()
    first = eng.grad.clone()
    eng.grad.fill_(float("nan"))                                # (every tensor and the four scalars are written again)
    eng.loss_and_grads(xg, eg, 1.0)
    torch.cuda.synchronize()
    for k, v in model.state_dict().items():                     # (per tensor: the flat buffer's alignment padding is never written)
        lo, n = eng._layout[k], v.numel()
        assert torch.equal(first[lo:lo + n], eng.grad[lo:lo + n]), k
    assert torch.equal(first[-4:], eng.grad[-4:]) and torch.isfinite(first[-4:]).all()      # the four scalars


# ------------------------------------------------------------------------------- 4. decode with a transform
@pytest.mark.parametrize("name", [CASE1, "c03_1d16_t_c4_b5_gelu"])
def test_decode_with_angle_shift_scale(gpu_device, name):
    c, model, eng = make(name)
    o = orc.SVIOracle(state(model), mc.case_config(c), dtype=torch.float64)
    z = torch.randn(5, 2, generator=torch.Generator().manual_seed(2))
    dec = model.decode(z, angle=0.3, shift=[0.1, -0.2], scale=1.2)
    assert tuple(dec.shape) == (5,) + tuple(c["dims"]) + (c["C"],)
    want = o.decode(z, None, 0.3, [0.1, -0.2], 1.2, rate=True)
    np.testing.assert_allclose(dec.numpy(), want.numpy(), rtol=1e-4, atol=2e-6)
    plain = o.decode(z, rate=True)
    assert (plain - want).abs().max().item() > 1e-3             # (the transform does something)


# ------------------------------------------------------------------------------- 5. trainer
def test_trainer_history_and_weights_round_trip(gpu_device, tmp_path):
    """SVItrainer(model).step(loader), two epochs of three minibatches of case 1's kind, against SVIOracle.train_epoch driven by
    the same generator: loss_history to 1e-4; evaluate runs; save_weights / load_weights round-trips."""
    c = mc.CASES[CASE1]
    x = mc.images(torch.Generator().manual_seed(0), 18, c["dims"], c["C"])
    loader = pv.utils.init_dataloader(x, batch_size=6)
    model = pv.models.iVAE(c["dims"], 2, c["inv"], seed=1, device="cuda", **mc.model_kwargs(c))
    params0 = state(model)
    tr = pv.trainers.SVItrainer(model, seed=1)
    st = torch.get_rng_state()
    for _ in range(2):
        tr.step(loader)
    torch.cuda.synchronize()
    torch.set_rng_state(st)
    o = orc.SVIOracle(params0, mc.case_config(c), lr=LR)
    want = [o.train_epoch(loader) for _ in range(2)]
    print("trainer: history %s, reference %s" % (tr.loss_history["training_loss"], want))
    np.testing.assert_allclose(tr.loss_history["training_loss"], want, rtol=1e-4)
    assert np.isfinite(tr.evaluate(loader))
    path = str(tmp_path / "mc")
    model.save_weights(path)
    other = pv.models.iVAE(c["dims"], 2, c["inv"], seed=5, device="cuda", **mc.model_kwargs(c))
    other.load_weights(path + ".pt")
    for k, v in model.state_dict().items():
        assert torch.equal(other.state_dict()[k], v), k
    z = torch.randn(4, 2, generator=torch.Generator().manual_seed(2))
    assert torch.equal(other.decode(z), model.decode(z))


def test_bf16_precision_is_refused(gpu_device):
    c, model, eng = make(CASE1)
    with pytest.raises(ValueError, match="channels"):
        pv.trainers.SVItrainer(model, precision="bf16")
