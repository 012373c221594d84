"""
GPU tests (-m gpu) of per-observation weights of the likelihood: model.engine(pixel_weights=w) / SVItrainer(model,
pixel_weights=w), pv_ivae_weighted_* in the C ABI — the weighted instances of the fused f32 decoder kernel
(pv_sdec_fused_mc_kernel<GRADS, C, true>, C = 1 .. 8) and the weighted layer-by-layer kernels (pv_out_lik, pv_out_lik_mc,
pv_lik_elem, the weighted Poisson normaliser).

The reference is tests/_pixel_weight_cases.WeightedOracle in float64: orc.elbo for one particle with
ll = (log_prob * w).sum(-1).  Cases, weights, data and eps come from _pixel_weight_cases.  Bars are the project's own for these
kernels (tests/test_gpu_multichannel.py / _fused.py): loss and ll 2e-5 (+ _multichannel_cases.loss_atol), the KL scalars 1e-4, z_loc /
z_scale rtol 1e-4 atol 5e-6, loc_out rtol 1e-4 atol 2e-6, every gradient tensor 1e-4 relative L2 — and each row of
decoder.out.weight and each decoder.out.bias[c] on its own —, parameters after Adam by check_params_after_adam's rule at the
5e-5 bar (its 1 % cap is confirmed with the reference alone in tests/test_pixel_weights_cpu.py).
"""
import numpy as np
import pytest
import torch

import pyroved_amd as pv
from oracle import svi_oracle as orc
import _multichannel_cases as mc
import _pixel_weight_cases as pw
from _judge import RTOL_GRAD, LR, rel_l2, state, steps_vs_reference, cpu_threads_16

pytestmark = pytest.mark.gpu

CASE1 = pw.CASE1


def build(name, w="case", **engine_kw):
    """(case, model, engine): w = "case" the case's weights, None no weights, or a tensor."""
    c = pw.CASES[name]
    model = pv.models.iVAE(c["dims"], 2, c["inv"], seed=1, device="cuda", **mc.model_kwargs(c))
    if isinstance(w, str):
        w = pw.weights(c)
    if w is not None:
        engine_kw["pixel_weights"] = w
    return c, model, model.engine(**engine_kw)


def n_obs(c):
    return int(np.prod(c["dims"])) * c["C"]


def check_output_layer_rows(eng, o, tag):
    """Each row of decoder.out.weight and each decoder.out.bias[c] on its own (rows of weight zero — masked outputs of a vanilla
    decoder — must be exactly zero on both sides)."""
    gw, rw = eng.grad_of("decoder.out.weight").cpu().double(), o.last_grads["decoder.out.weight"]
    gb, rb = eng.grad_of("decoder.out.bias").cpu().double(), o.last_grads["decoder.out.bias"]
    worst = 0.0
    for i in range(rw.shape[0]):
        for got, ref, what in ((gw[i], rw[i], "weight[%d]" % i), (gb[i], rb[i], "bias[%d]" % i)):
            if ref.abs().max().item() == 0.0:
                assert got.abs().max().item() == 0.0, "%s decoder.out.%s: reference gradient is exactly 0" % (tag, what)
                continue
            err = rel_l2(got, ref)
            worst = max(worst, err)
            assert err < RTOL_GRAD, "%s decoder.out.%s: rel error %.3e" % (tag, what, err)
    print("%s: worst decoder.out row / bias entry rel error %.2e" % (tag, worst))


def run_steps(name, engine_kw, want_fused, kl="sampled"):
    kw = dict(engine_kw)
    if kl != "sampled":
        kw["kl"] = kl
    c, model, eng = build(name, **kw)
    b = c["b"]
    used = eng.uses_fused(b)
    print("%s %s: uses_fused %s" % (name, engine_kw, used))
    if want_fused is not None:
        assert used is want_fused
    assert eng.supports_dp_step is False
    x, y, eps = pw.case_data(c)
    o = pw.WeightedOracle(state(model), pw.case_config(c), pw.weights(c), lr=LR, dtype=torch.float64, kl=kl)
    loc = torch.full((b, n_obs(c)), float("nan"), device="cuda")
    steps_vs_reference(eng, model, o, x, y, eps, 1.0, "%s %s %s" % (name, engine_kw, kl), 0, 5e-6, atol=mc.loss_atol(c),
                       checks=[check_output_layer_rows], loc_out=loc)      # (0: the 5e-5 bar after Adam; z atol 5e-6)


# ------------------------------------------------------------------------------- 1. step parity
STEP_PARAMS = [(n, i) for n in sorted(pw.CASES) for i in range(len(pw.CASES[n]["paths"]))]


@pytest.mark.parametrize("name,path", STEP_PARAMS)
def test_steps_vs_reference(gpu_device, name, path):
    """Two steps with Adam between, each from identical float32 parameters, on the path the case table names.  uses_fused is
    asserted for the fused cases up to four channels; above that (paths' None) whatever the instance hook reports is printed."""
    kw, want_fused = pw.CASES[name]["paths"][path]
    run_steps(name, kw, want_fused)


def test_analytic_kl_steps(gpu_device):
    run_steps(CASE1, {}, True, kl="analytic")


# ------------------------------------------------------------------------------- 2. cross-checks on w01
def _scalars_and_grads(eng):
    torch.cuda.synchronize()
    return eng.scalars.clone(), eng.grad.clone()


def _per_tensor_equal(model, eng, a, b):
    for k, v in model.state_dict().items():                     # (per tensor: the flat buffer's alignment padding is never written)
        lo, n = eng._layout[k], v.numel()
        if not torch.equal(a[lo:lo + n], b[lo:lo + n]):
            return False
    return torch.equal(a[-4:], b[-4:])


def test_evaluate_and_repeat(gpu_device):
    """want_grads=False gives the gradient call's four scalars to 2e-6; a repeated call is bit-identical."""
    c, model, eng = build(CASE1)
    x, y, eps = pw.case_data(c)
    xg, eg = x.cuda(), eps[0].cuda()
    eng.loss_and_grads(xg, eg, 1.0)
    s, g = _scalars_and_grads(eng)
    eng.grad.fill_(float("nan"))
    eng.loss_and_grads(xg, eg, 1.0)
    s2, g2 = _scalars_and_grads(eng)
    assert _per_tensor_equal(model, eng, g, g2) and torch.isfinite(s).all()
    eng.scalars.fill_(float("nan"))
    eng.loss_and_grads(xg, eg, 1.0, want_grads=False)
    torch.cuda.synchronize()
    print("evaluate %s, gradient call %s" % (eng.scalars.tolist(), s.tolist()))
    np.testing.assert_allclose(eng.scalars.cpu().numpy(), s.cpu().numpy(), rtol=2e-6)
    t = model.elbo_terms(x, eps=eps[0])                                  # elbo_terms is weighted too
    np.testing.assert_allclose([t["loss"], t["ll"]], s[:2].cpu().numpy(), rtol=2e-6)


def test_step_in_one_call_is_the_two_calls(gpu_device):
    """loss_and_grads(step=True) against loss_and_grads + adam_step: parameters, moments and scalars bit for bit, two steps."""
    out = []
    for one_call in (True, False):
        c, model, eng = build(CASE1)
        x, y, eps = pw.case_data(c)
        sc = torch.zeros(2, 4, device="cuda")
        for k in range(2):
            if one_call:
                eng.loss_and_grads(x.cuda(), eps[k].cuda(), 1.0, scalars_out=sc[k], step=True)
            else:
                eng.loss_and_grads(x.cuda(), eps[k].cuda(), 1.0, scalars_out=sc[k])
                eng.adam_step()
        torch.cuda.synchronize()
        out.append((eng.flat.clone(), eng.m.clone(), eng.v.clone(), sc.clone()))
    for a, b, what in zip(out[0], out[1], ("parameters", "m", "v", "scalars")):
        assert torch.equal(a, b), what


def test_fused_and_layered_agree(gpu_device):
    grads = []
    for kw in ({}, dict(fused=0)):
        c, model, eng = build(CASE1, **kw)
        assert eng.uses_fused(c["b"]) is (not kw)
        x, y, eps = pw.case_data(c)
        eng.loss_and_grads(x.cuda(), eps[0].cuda(), 1.0)
        torch.cuda.synchronize()
        grads.append({k: eng.grad_of(k).clone() for k in model.state_dict()})
    worst = max(rel_l2(grads[0][k], grads[1][k]) for k in grads[0])
    print("fused vs layered weighted gradients: worst rel l2 %.2e" % worst)
    for k in grads[0]:
        assert rel_l2(grads[0][k], grads[1][k]) < RTOL_GRAD, k


# ------------------------------------------------------------------------------- 3. exact checks
SAME_FAMILY = [
    ("layered", "w01_8x8_rts_c1_b6_disc", dict(fused=0), dict(fused=0)),
    ("layered_mc", "w08_7x9_rt_c3_b3_gauss_nosig_72_40_softplus_ramp", dict(fused=0), dict(fused=0)),
    ("vanilla", "w10_8x8_none_c2_b6_soft", dict(fused=0), dict(fused=0)),
    ("fused_channels", "w04_8x8_rts_c2_cdim3_b6_cbern_disc", dict(fused_channels=True), dict(fused_channels=True)),
    ("fused_channels_poisson", "w03_8x8_r_c3_b6_poisson_ramp", dict(fused_channels=True), dict(fused_channels=True)),
    ("one_channel_fused", "w01_8x8_rts_c1_b6_disc", dict(), dict(fused=1)),
]


@pytest.mark.parametrize("tag,name,kw_w,kw_plain", SAME_FAMILY, ids=[s[0] for s in SAME_FAMILY])
def test_ones_are_the_unweighted_step(gpu_device, tag, name, kw_w, kw_plain):
    """Weights of ones: the weighted call's scalars and gradients equal the unweighted call's on the same kernel family to 2e-6.
    (one channel, fused: the weighted instance of the multi-channel kernel against pv_sdec_fused_kernel — two kernels, one
    arithmetic.)"""
    c = pw.CASES[name]
    x, y, eps = pw.case_data(c)
    yg = None if y is None else y.cuda()
    res = []
    for w, kw in ((torch.ones(*c["dims"], c["C"]) if c["C"] > 1 else torch.ones(*c["dims"]), kw_w), (None, kw_plain)):
        _, model, eng = build(name, w=w, **dict(kw))
        eng.loss_and_grads(x.cuda(), eps[0].cuda(), 1.0, yg)
        res.append(_scalars_and_grads(eng) + (model, eng))
    (s1, g1, model, eng), (s0, g0, _, _) = res
    print("%s: bit-identical to the unweighted call: %s" % (tag, _per_tensor_equal(model, eng, g1, g0) and torch.equal(s1, s0)))
    np.testing.assert_allclose(s1.cpu().numpy(), s0.cpu().numpy(), rtol=2e-6)
    for k, v in model.state_dict().items():
        lo, n = eng._layout[k], v.numel()
        assert rel_l2(g1[lo:lo + n], g0[lo:lo + n]) < 2e-6, k


def test_weights_of_two_double_ll(gpu_device):
    c = pw.CASES[CASE1]
    x, y, eps = pw.case_data(c)
    _, _, e2 = build(CASE1, w=torch.full(tuple(c["dims"]), 2.0), fused=1)
    e2.loss_and_grads(x.cuda(), eps[0].cuda(), 1.0)
    s2, _ = _scalars_and_grads(e2)
    _, _, e1 = build(CASE1, w=None, fused=1)
    e1.loss_and_grads(x.cuda(), eps[0].cuda(), 1.0)
    s1, _ = _scalars_and_grads(e1)
    print("ll: weights of 2 %.6f, unweighted %.6f" % (s2[1].item(), s1[1].item()))
    np.testing.assert_allclose(s2[1].item(), 2.0 * s1[1].item(), rtol=2e-6)
    assert torch.equal(s2[2:], s1[2:])


def test_vanilla_mask_zeroes_masked_outputs_exactly(gpu_device):
    """Vanilla decoder, disc mask, 8 x 8, one channel: the gradient entries of decoder.out.weight / .bias of masked outputs are
    exactly 0.0; the unmasked rows meet the 1e-4 bar against the reference."""
    name = "w09_8x8_none_c1_b6_soft"
    c = pw.CASES[name]
    w = pw.weights(c, "disc")
    _, model, eng = build(name, w=w)
    x, y, eps = pw.case_data(c)
    eng.loss_and_grads(x.cuda(), eps[0].cuda(), 1.0)
    torch.cuda.synchronize()
    o = pw.WeightedOracle(state(model), pw.case_config(c), w, lr=LR, dtype=torch.float64)
    o.step(x, eps[0], 1.0)
    masked = w.reshape(-1) == 0
    assert 0 < int(masked.sum()) < masked.numel()
    gw, gb = eng.grad_of("decoder.out.weight").cpu(), eng.grad_of("decoder.out.bias").cpu()
    assert (gw[masked] == 0.0).all() and (gb[masked] == 0.0).all()
    assert (gw[~masked].abs().amax(1) > 0).all() and (gb[~masked] != 0).all()
    check_output_layer_rows(eng, o, "vanilla disc")
    for k in o.p:
        assert rel_l2(eng.grad_of(k), o.last_grads[k]) < RTOL_GRAD, k


# ------------------------------------------------------------------------------- 4. trainer
def test_trainer_history_and_evaluate(gpu_device):
    """SVItrainer(model, pixel_weights=w): two epochs of three minibatches on w01's shape against the reference's loop driven by
    the same generator, loss history to 1e-5; evaluate is weighted."""
    c = pw.CASES[CASE1]
    w = pw.weights(c)
    x = mc.images(torch.Generator().manual_seed(0), 18, c["dims"], 1)[..., 0].contiguous()
    loader = pv.utils.init_dataloader(x, batch_size=6)
    model = pv.models.iVAE(c["dims"], 2, c["inv"], seed=1, device="cuda", **mc.model_kwargs(c))
    params0 = state(model)
    tr = pv.trainers.SVItrainer(model, seed=1, pixel_weights=w)
    assert tr.engine.uses_fused(6) is True
    st = torch.get_rng_state()
    for _ in range(2):
        tr.step(loader)
    got_eval = tr.evaluate(loader)
    torch.cuda.synchronize()
    torch.set_rng_state(st)
    o = pw.WeightedOracle(params0, pw.case_config(c), w, lr=LR, dtype=torch.float64)
    want = [o.train_epoch(loader) for _ in range(2)]
    want_eval = o.evaluate_epoch(loader)
    print("trainer: history %s, reference %s; evaluate %.6f, reference %.6f" % (tr.loss_history["training_loss"], want, got_eval, want_eval))
    np.testing.assert_allclose(tr.loss_history["training_loss"], want, rtol=1e-5)
    np.testing.assert_allclose(got_eval, want_eval, rtol=1e-5)
    plain = orc.SVIOracle(params0, pw.case_config(c), lr=LR, dtype=torch.float64)
    torch.set_rng_state(st)
    assert abs(plain.train_epoch(loader) - want[0]) > 1e-3 * abs(want[0])       # (the weights do something)


# ------------------------------------------------------------------------------- 5. without the keyword nothing changes
def test_without_the_keyword_nothing_changes(gpu_device):
    """The default engine's gradients on w01's model are bit-identical before and after an engine with weights was configured and
    then un-configured with pixel_weights=False."""
    c, model, eng = build(CASE1, w=None)
    x, y, eps = pw.case_data(c)
    xg, eg = x.cuda(), eps[0].cuda()
    assert eng.uses_fused(c["b"]) is True and eng._plan_fused() == 2
    eng.loss_and_grads(xg, eg, 1.0)
    s0, g0 = _scalars_and_grads(eng)
    eng.configure(pixel_weights=pw.weights(c))
    assert eng._plan_fused() == 1
    eng.loss_and_grads(xg, eg, 1.0)
    s1, g1 = _scalars_and_grads(eng)
    assert not torch.equal(s1, s0)
    eng.configure(pixel_weights=False)
    assert eng.pixel_weights is None and eng._plan_fused() == 2
    eng.grad.fill_(float("nan"))
    eng.loss_and_grads(xg, eg, 1.0)
    s2, g2 = _scalars_and_grads(eng)
    assert _per_tensor_equal(model, eng, g0, g2)
