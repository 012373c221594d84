"""
GPU tests (-m gpu) of the Poisson (log link) likelihood for count data: sampler_d="poisson_log" / PV_LIK_POISSON_LOG.

The reference is the project's own oracle (oracle.svi_oracle.likelihood yields torch.distributions.Poisson(exp(min(a, 30)))
for that sampler).  Inputs are counts (tests/_poisson_data.counts: rates 1 .. 3 around a blob per image), drawn from torch.Generator().manual_seed(0): centres, counts,
then the eps draws.  Every step case runs from identical parameters at each step, two steps, Adam between, and is held to the
bars of the existing step tests for the same path (tests/_judge.py).  The reported loss includes the data-only
normaliser C = sum lgamma(x + 1), which the kernels leave to pv_poisson_lognorm.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from conftest import load_golden

import pyroved_amd as pv
from pyroved_amd import _abi
from oracle import svi_oracle as orc
from oracle import bf16_plan as bp
import _poisson_data as pr
from _bf16_judge import judge, GRAD_CEIL, LOSS_CEIL, LOC_CEIL, SELF_CHECK
from _device import cus, kernel_name
from _golden_models import ved_case
from _judge import (RTOL_ELBO, RTOL_KL, RTOL_GRAD, Z_ATOL, LR, rel_l2, state, reload, check_scalars, check_z, check_grads,
                    check_params_after_adam, steps_vs_reference, cpu_threads_16)
from _renyi_cases import weight_check, free_and_held

pytestmark = pytest.mark.gpu

LIK = _abi.LIK["poisson_log"]


# ------------------------------------------------------------------------------- 1. fp32-class steps
@pytest.mark.parametrize("fused", [0, 1, 2])
@pytest.mark.parametrize("name", sorted(pr.STEP_CASES))
def test_poisson_steps_vs_reference(gpu_device, name, fused):
    """Against the float64 reference, at the bars of the existing step tests: loss and s1 2e-5, s2 / s3 / z_loc / z_scale 1e-4,
    every gradient tensor 1e-4 relative L2, parameters after Adam by check_params_after_adam's rule (its 1 % cap on near-zero
    gradient entries is confirmed with the reference alone in tests/test_poisson_cpu.py)."""
    model, cfg, x, y, eps, b = pr.step_case(name, "cuda")
    sampled = pr.STEP_CASES[name].get("sampled", False)
    eng = model.engine(fused=fused)
    o = orc.SVIOracle(state(model), cfg, lr=LR, dtype=torch.float64)
    o.sampled_class = sampled
    zl, zs = torch.empty(b, cfg.z_dim, device="cuda"), torch.empty(b, cfg.z_dim, device="cuda")
    for k in range(2):
        tag = "%s fused=%d step %d" % (name, fused, k)
        if sampled:
            eng.loss_and_grads(x.cuda(), eps[k].cuda(), 1.0, class_onehot=y[k].cuda(), z_out=(zl, zs))
            o.step(x, eps[k], 1.0, y[k])
        else:
            eng.loss_and_grads(x.cuda(), eps[k].cuda(), 1.0, None if y is None else y.cuda(), z_out=(zl, zs))
            o.step(x, eps[k], 1.0, y)
        c_norm = pr.lognorm(x)
        print("%s: C = %.4f of loss %.4f" % (tag, c_norm, o.last["loss"].item()))
        check_scalars(eng.scalars.cpu().numpy(), o.last, tag)
        check_z(zl, zs, o.last, RTOL_KL, Z_ATOL, tag)
        check_grads(eng, o, tag)
        eng.adam_step()
        check_params_after_adam(model, o, fused, tag)
        reload(model, o, round32=True)


# ------------------------------------------------------------------------------- 1b. large counts
# (scale of the counts, decoder.out.bias or None).  28x28 `rt` at B = 24 is 18 816 decoder rows: from 16 384 rows up the size rule
# gives the split-precision path (fused = 2, the default) its fp16 builds, whose staged per-row exponent holds |rate - x| < 2^15
# only — Poisson plans stay on the bf16 three-product kernel instead (pv_plan.hip: plan_sel).  Counts of 3e3 - 3e4 reach just
# under that bound (max |rate - x| = 29 999); counts up to 1e6 with logits around 11 (rates of 6e4) lie far beyond it on both
# sides of rate - x.
LARGE_CASES = {"counts_3e3_to_3e4": (3000.0, None), "counts_to_1e6_logit_11": (1.0e5, 11.0)}


@pytest.mark.parametrize("fused", [2, 3])
@pytest.mark.parametrize("name", sorted(LARGE_CASES))
def test_large_counts_stay_finite_and_accurate(gpu_device, name, fused):
    """fused = 2 (the default path) against the float64 reference at the step tests' bars: loss and s1 2e-5, every gradient tensor
    1e-4 relative L2 — except where the float32 evaluation of the reference itself is further than that from float64 (counts this
    large saturate the tanh encoder's first layer, whose gradient is then a sum of terms 1 - h^2 that cancel in fp32: measured
    6.9e-4 for encoder_z.fc_layers.0.* at counts of 3e4): such a tensor is held to twice the fp32 reference's own error, the rule
    tests/test_gpu_parity.py uses for the conv stacks.  fused = 3 (bf16 operands): loss 1e-4, gradients 3e-2, the bars of
    test_bf16_mode_steps_vs_golden_and_oracle.  On both: every gradient and, after Adam, every parameter is finite."""
    scale, bias = LARGE_CASES[name]
    dims, inv, b = (28, 28), ["r", "t"], 24
    model = pv.models.iVAE(dims, 2, inv, seed=1, device="cuda", **pr.KW)
    if bias is not None:
        sd = state(model)
        sd["decoder.out.bias"].fill_(bias)
        model.load_state_dict(sd)
    cfg = pr.config(dims, inv)
    g = torch.Generator().manual_seed(0)
    x = pr.counts(g, b, dims) * scale
    eps = torch.randn(b, cfg.z_dim, generator=g)
    assert x.max().item() >= 3.0e4 and b * 784 >= 16384
    eng = model.engine(fused=fused)
    eng.loss_and_grads(x.cuda(), eps.cuda(), 1.0)
    torch.cuda.synchronize()
    o = orc.SVIOracle(state(model), cfg, lr=LR, dtype=torch.float64)
    o32 = orc.SVIOracle(state(model), cfg, lr=LR)
    ref, r32 = o.loss_and_grads(x, eps, 1.0), o32.loss_and_grads(x, eps, 1.0)
    s = eng.scalars.cpu().numpy()
    dl = ref["loc"].detach().clamp(max=30).exp().reshape(b, -1) - x.reshape(b, -1).double()
    print("large %s fused=%d: loss %.6e (ref %.6e), max |rate - x| %.3e, max logit %.2f"
          % (name, fused, s[0], ref["loss"].item(), dl.abs().max().item(), ref["loc"].max().item()))
    if bias is None:
        assert 2.0 ** 14 < dl.abs().max().item() < 2.0 ** 15      # (the last binade an fp16 row exponent would hold)
    else:
        assert dl.abs().max().item() > 2.0 ** 19                  # (far beyond it)
    np.testing.assert_allclose(s[0], ref["loss"].item(), rtol=RTOL_ELBO if fused == 2 else 1e-4)
    np.testing.assert_allclose(s[1], ref["ll"].item(), rtol=RTOL_ELBO if fused == 2 else 1e-4)
    for key in o.p:
        got = eng.grad_of(key)
        assert torch.isfinite(got).all(), key
        e32 = rel_l2(o32.p[key].grad, o.p[key].grad)
        bar = max(RTOL_GRAD, 2.0 * e32) if fused == 2 else 3e-2
        err = rel_l2(got, o.p[key].grad)
        print("  %-42s %.3e (bar %.1e; fp32 reference %.3e)" % (key, err, bar, e32))
        assert err < bar, "%s grad %s: rel l2 error %.3e (bar %.1e)" % (name, key, err, bar)
    eng.adam_step()
    torch.cuda.synchronize()
    for key, p in model.state_dict().items():
        assert torch.isfinite(p).all(), key


# ------------------------------------------------------------------------------- 2. throughput precision
# (data_dim, invariances, B, kernel build, guide folds into the decoder launch)
BF16_CASES = {
    "28x28_rt_b256": ((28, 28), ["r", "t"], 256, "w8", True),              # the two-launch hosted step
    "28x28_r_b128": ((28, 28), ["r"], 128, "w8", False),                   # ranges crossing image boundaries
    "8x8_rts_b6": ((8, 8), ["r", "t", "s"], 6, "w4", False),               # the 4-wave build
}
# (gradient rel L2 of the worst tensor, loss relative): at most 4x the worst value measured on MI355X and never above
# tests/_bf16_judge.py's ceilings (gradients 1e-3, loss 1e-5); the measurement is in the comment
BF16_BARS = {
    "28x28_rt_b256": (1.1e-4, 1.2e-7),     # 2.80e-5 (decoder.coord_latent.fc_coord.weight) / 3.2e-8
    "28x28_r_b128": (1.2e-4, 1.5e-7),      # 3.13e-5 (decoder.fc_layers.0.weight) / 3.8e-8
    "8x8_rts_b6": (3.3e-4, 1.7e-7),        # 8.26e-5 (decoder.coord_latent.fc_latent.weight) / 4.4e-8
}
BF16_LOC_BAR = 2.3e-5                      # the forward-only launch's rate: 5.83e-6 / 5.49e-6 / 4.16e-6


def _bf16_setup(name):
    """(The build assertion is tests/test_gpu_bf16_emulated.py's: _device.kernel_name (pv_debug_decoder_kernel_name) restates the library's size rule on
    the host for the `lik` it is given — it shows which BUILD (8-wave / 4-wave, plain bf16) the size selects, not the dispatched
    symbol; for the hosted step it names <true, lik, 0> although the launch that hosts the guide is <true, lik, 2>.  That the
    Poisson instance ran is shown by the numbers: loss, rate and gradients against the Poisson reference.)"""
    dims, inv, b, kernel, fold = BF16_CASES[name]
    model = pv.models.iVAE(dims, 2, inv, seed=1, device="cuda", **pr.KW)
    eng = model.engine(fused=3)
    g = torch.Generator().manual_seed(0)
    x = pr.counts(g, b, dims)
    eps = torch.randn(b, model.z_dim, generator=g)
    assert eng.uses_fused(b)
    folds = bool(_abi.lib().pv_ivae_guide_folds(C.byref(eng._plan(b))))
    assert folds == (fold and cus() == 256), (folds, fold)
    kname = kernel_name(fused=3, units=b * int(np.prod(dims)) // 16, lik=LIK)
    want = "pv_sdec_w8_kernel<true, %d, 0>" % LIK if kernel == "w8" else "pv_sdec_fused_bf16_kernel<true, %d, 0>" % LIK
    assert want in kname, (kname, want)
    return model, eng, x, eps, dims, inv, b, kernel


@pytest.mark.parametrize("name", sorted(BF16_CASES))
def test_poisson_bf16_step_vs_emulated_reference(gpu_device, name):
    """fused = 3 (which build the size rule selects: see _bf16_setup) against the reference that rounds where the kernel rounds (oracle/bf16_plan.py emulates the decoder up to the
    logit; the likelihood is the oracle's), with tests/_bf16_judge.py's judge; then the forward-only launch:
    loss and loc (the rate) against the same emulation."""
    model, eng, x, eps, dims, inv, b, kernel = _bf16_setup(name)
    zl, zs = torch.empty(b, model.z_dim, device="cuda"), torch.empty(b, model.z_dim, device="cuda")
    eng.loss_and_grads(x.cuda(), eps.cuda(), 1.0, z_out=(zl, zs))
    torch.cuda.synchronize()
    params = state(model)

    def reference(plan):
        o = orc.SVIOracle(params, pr.config(dims, inv, bf16_plan=plan), dtype=torch.float64)
        out = o.loss_and_grads(x, eps, 1.0)
        return out, {k: v.grad.detach().clone() for k, v in o.p.items()}
    ref_out, ref_g = reference(bp.Bf16Plan(kernel=kernel, cus=cus()))
    f64_out, f64_g = reference(None)
    grad_bar, loss_bar = BF16_BARS[name]
    assert grad_bar <= GRAD_CEIL and loss_bar <= LOSS_CEIL and BF16_LOC_BAR <= LOC_CEIL
    judge("poisson " + name, eng, ref_out, ref_g, f64_out, f64_g, zl.cpu(), zs.cpu(), grad_bar, loss_bar, SELF_CHECK)
    s = eng.scalars.cpu().numpy()
    np.testing.assert_allclose(s[0], -(s[1] + s[2] - s[3]), rtol=2e-6)
    loc = torch.empty(b, int(np.prod(dims)), device="cuda")
    eng.loss_and_grads(x.cuda(), eps.cuda(), 1.0, want_grads=False, loc_out=loc)
    torch.cuda.synchronize()
    le = abs(eng.scalars[0].item() - ref_out["loss"].item()) / abs(ref_out["loss"].item())
    lo = rel_l2(loc, torch.exp(ref_out["loc"].detach().clamp(max=30)).reshape(b, -1))
    print("[bf16-emulated] poisson %s forward-only: loss %.3e, rate %.3e from the emulation" % (name, le, lo))
    assert le < loss_bar and lo < BF16_LOC_BAR


# ------------------------------------------------------------------------------- 3. the other objectives
OBJ = dict(dims=(8, 8), inv=["r", "t", "s"], b=6, P=3, beta=1.7)


def _obj_inputs(P):
    model = pv.models.iVAE(OBJ["dims"], 2, OBJ["inv"], seed=1, device="cuda", **pr.KW)
    cfg = pr.config(OBJ["dims"], OBJ["inv"])
    g = torch.Generator().manual_seed(0)
    x = pr.counts(g, OBJ["b"], OBJ["dims"])
    eps = [torch.randn(P * OBJ["b"], cfg.z_dim, generator=g) for _ in range(2)]
    return model, cfg, x, eps


@pytest.mark.parametrize("fused", [0, 2])
def test_poisson_analytic_kl_steps_vs_reference(gpu_device, fused):
    """kl="analytic" at the bars of tests/test_gpu_meanfield.py; the reported loss includes C."""
    model, cfg, x, eps = _obj_inputs(1)
    b = OBJ["b"]
    eng = model.engine(fused=fused, kl="analytic")
    o = orc.SVIOracle(state(model), cfg, lr=LR, dtype=torch.float64, kl="analytic")
    steps_vs_reference(eng, model, o, x, None, eps, OBJ["beta"], "poisson analytic fused=%d" % fused, fused, Z_ATOL)


@pytest.mark.parametrize("fused", [0, 2])
def test_poisson_three_particle_steps_vs_reference(gpu_device, fused):
    """particles=3 at the bars of tests/test_gpu_particles.py (the mean over particles of a constant is that constant)."""
    model, cfg, x, eps = _obj_inputs(OBJ["P"])
    b, P = OBJ["b"], OBJ["P"]
    eng = model.engine(fused=fused, particles=P)
    o = orc.SVIOracle(state(model), cfg, lr=LR, dtype=torch.float64, particles=P)
    steps_vs_reference(eng, model, o, x, None, eps, OBJ["beta"], "poisson P=3 fused=%d" % fused, fused, Z_ATOL)


@pytest.mark.parametrize("fused", [0, 2])
def test_poisson_renyi_steps_vs_reference(gpu_device, fused):
    """renyi=0.0 (IWAE), P = 3, at the bars of tests/test_gpu_renyi.py: every L_b shifts by -c_b and the weights are
    unchanged, checked through weights_out."""
    model, cfg, x, eps = _obj_inputs(OBJ["P"])
    b, P, alpha, beta = OBJ["b"], OBJ["P"], 0.0, OBJ["beta"]
    eng = model.engine(fused=fused, particles=P, renyi=alpha)
    zl, zs = torch.empty(b, cfg.z_dim, device="cuda"), torch.empty(b, cfg.z_dim, device="cuda")
    w = torch.full((P * b,), float("nan"), device="cuda")
    o = None
    for k in range(2):
        tag = "poisson renyi fused=%d step %d" % (fused, k)
        eng.loss_and_grads(x.cuda(), eps[k].cuda(), beta, z_out=(zl, zs), weights_out=w)
        torch.cuda.synchronize()
        of, g_free, o = free_and_held(state(model), cfg, P, alpha, x, eps[k], beta, None, w, o)
        check_scalars(eng.scalars.cpu().numpy(), of, tag)
        check_z(zl, zs, of, RTOL_KL, Z_ATOL, tag)
        weight_check(tag, w, of, alpha, RTOL_ELBO)
        check_grads(eng, o, tag + ", the engine's weights held")
        eng.adam_step()
        check_params_after_adam(model, o, fused, tag)
        reload(model, o, round32=True)


# ------------------------------------------------------------------------------- 4. the normaliser
@pytest.mark.parametrize("fused", [0, 2, 3])
def test_normaliser_enters_the_scalars_exactly_once(gpu_device, fused):
    """With want_grads = 0 and again with gradients: scalars[1] differs from the sum of the kernels' unnormalised per-pixel terms
    x a - exp(a) (formed in float64 from the rate the same launch wrote to loc_out) by the float64 C, to 2e-5 of the loss;
    scalars[0] = -(s1 + s2 - s3) still holds; two calls give identical bits."""
    dims, inv, b = (12, 20), ["r", "t", "s"], 6
    model = pv.models.iVAE(dims, 2, inv, seed=1, device="cuda", **pr.KW)
    eng = model.engine(fused=fused)
    g = torch.Generator().manual_seed(0)
    x = pr.counts(g, b, dims)
    eps = torch.randn(b, model.z_dim, generator=g)
    c_norm = pr.lognorm(x)
    loc = torch.empty(b, int(np.prod(dims)), device="cuda")
    for grads in (False, True):
        bits = []
        for _ in range(2):
            eng.grad.zero_()
            eng.loss_and_grads(x.cuda(), eps.cuda(), 1.0, want_grads=grads, loc_out=loc)
            torch.cuda.synchronize()
            bits.append((eng.scalars.clone(), eng.grad.clone()))
        assert torch.equal(bits[0][0], bits[1][0]) and torch.equal(bits[0][1], bits[1][1])
        s = eng.scalars.cpu().double().numpy()
        rate = loc.cpu().double()
        unnorm = (x.double().reshape(b, -1) * torch.log(rate) - rate).sum().item()
        print("normaliser fused=%d grads=%d: s1 %.6f, unnormalised %.6f, difference %.6f, C %.6f, loss %.6f"
              % (fused, grads, s[1], unnorm, unnorm - s[1], c_norm, s[0]))
        assert c_norm > 0.2 * abs(s[0])                                         # (C is not a small part of this loss)
        assert abs((unnorm - s[1]) - c_norm) <= 2e-5 * abs(s[0])
        np.testing.assert_allclose(s[0], -(s[1] + s[2] - s[3]), rtol=2e-6)


# ------------------------------------------------------------------------------- 5. decode / loc_out
@pytest.mark.parametrize("inv,dims", [(["r", "t"], (28, 28)), (["r", "t", "s"], (12, 20)), (None, (8, 8))])
@pytest.mark.parametrize("fused", [0, 1, 2])
def test_decode_and_loc_out_are_the_rate(gpu_device, inv, dims, fused):
    """model.decode (the fused forward-only launch, the layered path, the vanilla decoder) and loc_out of a step: exp(min(a, 30))
    to 1e-4 relative against the float64 reference."""
    b = 5
    model = pv.models.iVAE(dims, 2, inv, seed=2, device="cuda", **pr.KW)
    eng = model.engine(fused=fused)
    cfg = pr.config(dims, inv)
    o = orc.SVIOracle(state(model), cfg, dtype=torch.float64)
    z = torch.randn(b, 2, generator=torch.Generator().manual_seed(2))
    want = torch.exp(o.decode(z).clamp(max=30)).reshape(b, -1)
    got = model.decode(z).reshape(b, -1)
    assert rel_l2(got, want) < 1e-4 and got.min().item() > 0.0
    np.testing.assert_allclose(got.cpu().numpy(), want.numpy(), rtol=1e-4)
    if inv is not None:
        grid = model.manifold2d(3, plot=False)
        assert torch.isfinite(grid).all() and grid.min().item() > 0.0           # rates, not log-rates
    g = torch.Generator().manual_seed(0)
    x = pr.counts(g, b, dims)
    eps = torch.randn(b, cfg.z_dim, generator=g)
    loc = torch.empty(b, int(np.prod(dims)), device="cuda")
    eng.loss_and_grads(x.cuda(), eps.cuda(), 1.0, want_grads=False, loc_out=loc)
    with torch.no_grad():
        ref = o.loss_and_grads(x, eps, 1.0)
    np.testing.assert_allclose(loc.cpu().numpy(), torch.exp(ref["loc"].clamp(max=30)).reshape(b, -1).numpy(), rtol=1e-4)
    z_loc, _ = model.encode(x)
    np.testing.assert_allclose(z_loc.numpy(), ref["z_loc"].numpy(), rtol=1e-4, atol=2e-6)


# ------------------------------------------------------------------------------- 6. VED
@pytest.mark.parametrize("scale", [1.0, 3000.0])
def test_poisson_ved_steps_vs_reference(gpu_device, scale):
    """The ved_16x16_to_32_small_b5 fixture's geometry (only its meta is read), the target y = counts on the target's shape
    (times `scale`: 3000 gives counts of 3e3 - 3e4, |rate - y| beyond fp16's range), sigmoid_d=False, against the float64
    reference at the bars of the VED step tests (tests/test_gpu_meanfield.py, tests/test_gpu_parity.py): loss / s1 2e-5, every
    gradient 1e-4, parameters after Adam by that test's rule.  That rule carries NO cap on the share of near-zero gradient entries
    (those with |g| < 1e-5 max|g| are held to 2e-3 absolute, the rest to 5e-5), unlike the iVAE rule's 1 %: dead leaky-ReLU / ReLU
    units of the conv stacks give many exactly-zero gradients in the reference itself, so a cap would fail on the reference alone;
    hence there is no CPU confirmation of a cap for this case, at either scale."""
    c = ved_case(load_golden("ved_16x16_to_32_small_b5"))
    kw = dict(c["kw"])
    model = pv.models.VED(c["input_dim"], c["output_dim"], latent_dim=c["latent_dim"], seed=1, device="cuda", **kw, **pr.KW)
    cfg = orc.VedConfig(input_dim=c["input_dim"], output_dim=c["output_dim"], latent_dim=c["latent_dim"],
                        hidden_dim_e=kw.get("hidden_dim_e"), hidden_dim_d=kw.get("hidden_dim_d"),
                        activation=kw.get("activation", "lrelu"), sampler="poisson_log", sigmoid_d=False)
    eng = model.engine()
    o = orc.VedOracle(state(model), cfg, dtype=torch.float64)
    b = 5
    g = torch.Generator().manual_seed(0)
    y = pr.counts(g, b, c["output_dim"]).unsqueeze(1) * scale
    x = torch.rand(b, 1, *c["input_dim"], generator=g)
    zl, zs = torch.empty(b, cfg.z_dim, device="cuda"), torch.empty(b, cfg.z_dim, device="cuda")
    for k in range(2):
        eps = torch.randn(b, cfg.z_dim, generator=g)
        eng.loss_and_grads(x.cuda(), eps.cuda(), c["beta"], y.cuda(), z_out=(zl, zs))
        o.step(x, y, eps, c["beta"])
        tag = "poisson ved step %d (C = %.3f)" % (k, pr.lognorm(y))
        check_scalars(eng.scalars.cpu().numpy(), o.last, tag)
        check_z(zl, zs, o.last, RTOL_KL, Z_ATOL, tag)
        check_grads(eng, o, tag)
        eng.adam_step()
        check_params_after_adam(model, o, None, tag, ill_share=None)
        reload(model, o, round32=True)
    dec = model.decode(zl.cpu())
    want = torch.exp(o.decode(zl.cpu()).clamp(max=30))
    np.testing.assert_allclose(dec.numpy().reshape(b, -1), want.numpy().reshape(b, -1), rtol=1e-4)


# ------------------------------------------------------------------------------- 7. trainer, data parallel, user modules
def test_trainer_loss_history_carries_the_normaliser(gpu_device):
    """SVItrainer(iVAE(..., sampler_d="poisson_log", sigmoid_d=False)), two epochs of three minibatches on (8, 8), against
    SVIOracle.train_epoch driven by the same generator: loss_history to 2e-5."""
    dims, inv = (8, 8), ["r", "t"]
    x = pr.counts(torch.Generator().manual_seed(0), 18, dims)
    loader = pv.utils.init_dataloader(x, batch_size=6)
    model = pv.models.iVAE(dims, 2, inv, seed=1, device="cuda", **pr.KW)
    params0 = state(model)
    tr = pv.trainers.SVItrainer(model, seed=1)
    st = torch.get_rng_state()
    for _ in range(2):
        tr.step(loader)
    torch.cuda.synchronize()
    torch.set_rng_state(st)
    o = orc.SVIOracle(params0, pr.config(dims, inv), lr=LR)
    want = [o.train_epoch(loader) for _ in range(2)]
    print("poisson trainer: history %s, reference %s, C per image %.4f" % (tr.loss_history["training_loss"], want, pr.lognorm(x) / 18))
    np.testing.assert_allclose(tr.loss_history["training_loss"], want, rtol=2e-5)
    assert pr.lognorm(x) / 18 > 0.2 * want[0]


@pytest.mark.parametrize("kw", [dict(precision="bf16"), dict(loss="TraceMeanField_ELBO"), dict(num_particles=2),
                                dict(loss="RenyiELBO", num_particles=2)])
def test_trainer_options_pass_the_likelihood_through(gpu_device, kw):
    """precision, objective and particle count need no Poisson-specific code: one epoch each runs, and the recorded loss
    carries the normaliser — it lies within half of C per image of the reference's ELBO at eps = 0 (the objectives differ from
    that value by KL-sized terms, a few units; without C the loss would be a whole C per image lower)."""
    dims, inv = (8, 8), ["r", "t"]
    x = pr.counts(torch.Generator().manual_seed(0), 12, dims)
    loader = pv.utils.init_dataloader(x, batch_size=6)
    model = pv.models.iVAE(dims, 2, inv, seed=1, device="cuda", **pr.KW)
    o = orc.SVIOracle(state(model), pr.config(dims, inv), dtype=torch.float64)
    with torch.no_grad():
        ref = o.loss_and_grads(x, torch.zeros(12, o.cfg.z_dim), 1.0)["loss"].item() / 12
    tr = pv.trainers.SVItrainer(model, seed=1, **kw)
    tr.step(loader)
    got = tr.loss_history["training_loss"][0]
    c_img = pr.lognorm(x) / 12
    print("poisson trainer %s: %.4f (eps = 0 reference %.4f, C per image %.4f)" % (kw, got, ref, c_img))
    assert np.isfinite(got) and abs(got - ref) < 0.5 * c_img


def test_native_data_parallel_step_carries_the_normaliser(gpu_device):
    """pv_ivae_dp_step at world size 1 (loss_and_grads -> all-reduce of [grads | 4 scalars] -> Adam + history) against
    loss_and_grads() + adam_step_hist(): the shard adds its C before the reduction, so history and parameters agree bit for
    bit and the loss is the reference's."""
    from pyroved_amd import dist as pvdist
    comm = pvdist.native_comm(torch.device("cuda", 0))
    dims, inv, b = (8, 8), ["r", "t"], 6
    mk = lambda: pv.models.iVAE(dims, 2, inv, seed=1, device="cuda", **pr.KW)
    ma, mb = mk(), mk()
    ea, eb = ma.engine(fused=2), mb.engine(fused=2)
    o = orc.SVIOracle(state(ma), pr.config(dims, inv), lr=LR, dtype=torch.float64)
    g = torch.Generator().manual_seed(0)
    x = pr.counts(g, b, dims)
    ha, hb = torch.zeros(2, 4, device="cuda"), torch.zeros(2, 4, device="cuda")
    want = []
    for i in range(2):
        eps = torch.randn(b, ma.z_dim, generator=g)
        ea.loss_and_grads(x.cuda(), eps.cuda())
        ea.adam_step_hist(ha[i])
        eb.loss_and_grads(x.cuda(), eps.cuda(), step=True, comm=comm, hist_out=hb[i])
        want.append(o.step(x, eps, 1.0))
    torch.cuda.synchronize()
    assert torch.equal(ha, hb) and torch.equal(ea.flat, eb.flat)
    np.testing.assert_allclose(hb[:, 0].cpu().numpy(), want, rtol=2e-5)


class _UserEncoder(torch.nn.Module):
    def __init__(self, n_in, z_dim):
        super().__init__()
        self.n_in = n_in
        self.l1, self.mu, self.sd = torch.nn.Linear(n_in, 32), torch.nn.Linear(32, z_dim), torch.nn.Linear(32, z_dim)

    def forward(self, x):
        h = torch.tanh(self.l1(x.reshape(-1, self.n_in)))
        return self.mu(h), torch.nn.functional.softplus(self.sd(h))


class _UserDecoder(torch.nn.Module):
    def __init__(self, z_dim, n_out):
        super().__init__()
        self.l1, self.l2 = torch.nn.Linear(z_dim, 32), torch.nn.Linear(32, n_out)

    def forward(self, z):
        return self.l2(torch.tanh(self.l1(z)))


@pytest.mark.parametrize("which", ["conv_encoder", "user_encoder", "user_decoder"])
def test_other_encoders_and_a_user_decoder(gpu_device, which):
    """A conv encoder and user-defined modules with the Poisson likelihood: loss and s1 against the float64 reference at 2e-5
    (conv encoder: the oracle's conv forward; user modules: the same torch modules evaluated in float64), the library-side
    gradients at the bars of the existing tests of these paths (1e-4; 2e-4 with a user-defined decoder; decoder.out.bias under
    a conv encoder on the absolute scale 1e-6 B N of its sum, as test_convenc_steps_vs_golden_and_oracle holds it)."""
    import copy
    b = 5
    torch.manual_seed(5)                           # (the user modules' initial weights)
    g = torch.Generator().manual_seed(0)
    if which == "conv_encoder":
        dims, inv, b = (16, 16), ["r", "t"], 4     # the ivaeconv_16x16_rt_b4 fixture's geometry
        hid = [(4,), (8, 8), (16, 16)]
        model = pv.models.iVAE(dims, 2, inv, seed=1, device="cuda", **pr.KW)
        model.set_encoder(pv.nets.convEncoderNet(dims, latent_dim=model.z_dim, hidden_dim=hid))
        cfg = pr.config(dims, inv, conv_encoder=hid)
    elif which == "user_encoder":
        dims, inv = (8, 8), ["r", "t"]
        model = pv.models.iVAE(dims, 2, inv, seed=1, device="cuda", **pr.KW)
        enc = _UserEncoder(64, model.z_dim)
        model.set_encoder(enc)
        e64 = copy.deepcopy(enc).double().cpu()
        cfg = pr.config(dims, inv, custom_encoder=lambda x: e64(x))
    else:
        dims, inv = (8, 8), None
        model = pv.models.iVAE(dims, 2, inv, seed=1, device="cuda", **pr.KW)
        dec = _UserDecoder(model.z_dim, 64)
        model.set_decoder(dec)
        d64 = copy.deepcopy(dec).double().cpu()
        cfg = pr.config(dims, inv, custom_decoder=lambda z: d64(z))
    x = pr.counts(g, b, dims)
    eps = torch.randn(b, model.z_dim, generator=g)
    eng = model.engine(fused=2)
    params = {k: v for k, v in state(model).items()
              if not (which == "user_encoder" and k.startswith("encoder_z.")) and not (which == "user_decoder" and k.startswith("decoder."))}
    o = orc.SVIOracle(params, cfg, dtype=torch.float64)
    eng.loss_and_grads(x.cuda(), eps.cuda(), 1.0)
    ref = o.loss_and_grads(x, eps, 1.0)
    s = eng.scalars.cpu().numpy()
    print("poisson %s: loss %.6f (ref %.6f)" % (which, s[0], ref["loss"].item()))
    np.testing.assert_allclose(s[0], ref["loss"].item(), rtol=RTOL_ELBO)
    np.testing.assert_allclose(s[1], ref["ll"].item(), rtol=RTOL_ELBO)
    for key in o.p:
        if which == "conv_encoder" and key == "decoder.out.bias":
            assert (eng.grad_of(key).cpu().double() - o.p[key].grad).abs().max().item() < 1e-6 * b * int(np.prod(dims))
            continue
        assert rel_l2(eng.grad_of(key), o.p[key].grad) < (2e-4 if which == "user_decoder" else RTOL_GRAD), key
