"""
GPU tests (-m gpu) of the categorical likelihood over channels: iVAE(..., channels=C, sampler_d="categorical", sigmoid_d=False)
-> plan.lik = PV_LIK_CATEGORICAL -> pv_out_lik_mc_cat_kernel<C> / pv_lik_elem_cat_kernel<C> (the layer-by-layer kernels,
pyroved_amd/csrc/pv_elementwise.hip) or, with model.engine(fused_channels=True), pv_sdec_fused_mc_cat_kernel<GRADS, C, WEIGHTED>
(pyroved_amd/csrc/pv_sdec_fused_mc.hip).

The reference is the project's float64 oracle with the likelihood of tests/_categorical_cases.py patched in for the test
(fixture categorical_oracle); cases, data and eps are that module's.  Every step cell runs _judge.steps_vs_reference: two steps
with Adam between, each from identical float32 parameters, at tests/_judge.py's constants as they stand — loss and ll 2e-5, the
KL scalars and z 1e-4 (z atol 5e-6 as in the multi-channel files), every gradient tensor 1e-4 relative L2 and, on their own, each
row of decoder.out.weight and each decoder.out.bias[c]; the parameters after Adam at ADAM_BAR[None] = 5e-5.  loc_out is the class
probabilities: against softmax of the reference's logits at check_loc's bars (rtol 1e-4, atol 2e-6), rows summing to 1 within
1e-6.  Every fused cell asserts the kernel through pv_debug_categorical_decoder_kernel_name.  The Renyi cells compose their bars
the way tests/test_gpu_renyi.py does.  tests/test_categorical_cpu.py confirms the condition the parameter check rests on.
"""
import numpy as np
import pytest
import torch

import pyroved_amd as pv
from pyroved_amd import _abi
from oracle import svi_oracle as orc
import _multichannel_cases as mc
import _categorical_cases as cc
import _pixel_weight_cases as pwc
import _image_weight_cases as iwc
from _categorical_cases import categorical_oracle          # noqa: F401  (fixture)
from _judge import (RTOL_ELBO, RTOL_KL, RTOL_GRAD, LR, rel_l2, state, reload, steps_vs_reference, check_scalars, check_z,
                    check_grads, check_params_after_adam, cpu_threads_16)          # noqa: F401  (cpu_threads_16: autouse fixture)
from _renyi_cases import weight_check, free_and_held

pytestmark = pytest.mark.gpu
Z_ATOL_MC = 5e-6


def make(name, route, **engine_kw):
    c = cc.CASES[name]
    model = cc.make_model(c, "cuda")
    return c, model, model.engine(**cc.ENGINE_KW[route], **engine_kw)


def assert_route(eng, c, route, weighted=0):
    """The kernel the call launches, by the library's own hook; uses_fused agrees."""
    for grads in (True, False):
        name = _abi.categorical_decoder_kernel_name(eng._plan(c["b"]), weighted, grads)
        if route == "fused":
            want = "void pv_sdec_fused_mc_cat_kernel<%s, %d, %d>(PvFused)" % ("true" if grads else "false", c["C"], weighted)
            assert name == want, (name, want)
        else:
            kernel = "pv_out_lik_mc_cat_kernel" if c["inv"] else "pv_lik_elem_cat_kernel"
            assert name.startswith("void %s<%d>(" % (kernel, c["C"])) and name.endswith("(layer-by-layer path)"), name
    assert eng.uses_fused(c["b"]) is (route == "fused"), (route, eng.uses_fused(c["b"]))


def check_channels(eng, o, tag):
    """Each class's row of d(decoder.out.weight) and each d(decoder.out.bias)[c] against the reference, on its own (the vanilla
    decoder's rows are (position, class) pairs: the same check over all of them would only repeat check_grads)."""
    gw, gb = eng.grad_of("decoder.out.weight").cpu().double(), eng.grad_of("decoder.out.bias").cpu().double()
    rw, rb = o.last_grads["decoder.out.weight"].double(), o.last_grads["decoder.out.bias"].double()
    assert gw.shape == rw.shape and gb.shape == rb.shape, "%s: decoder.out gradient shapes %s %s" % (tag, gw.shape, rw.shape)
    if gw.shape[0] != o.cfg.channels:
        return
    errs = [(rel_l2(gw[ch], rw[ch]), rel_l2(gb[ch], rb[ch])) for ch in range(gw.shape[0])]
    print("%s: per class (out.weight row, out.bias) %s" % (tag, " ".join("(%.1e %.1e)" % e for e in errs)))
    for ch, (ew, eb) in enumerate(errs):
        assert ew < RTOL_GRAD, "%s decoder.out.weight[%d]: rel l2 error %.3e (bar %.1e)" % (tag, ch, ew, RTOL_GRAD)
        assert eb < RTOL_GRAD, "%s decoder.out.bias[%d]: rel error %.3e (bar %.1e)" % (tag, ch, eb, RTOL_GRAD)


def run_steps(name, route, o_of, engine_kw=None, weighted=0, **outs):
    """steps_vs_reference for one cell; o_of(params, cfg) makes the float64 reference."""
    c, model, eng = make(name, route, **(engine_kw or {}))
    assert_route(eng, c, route, weighted)
    x, y, eps = cc.case_data(c)
    o = o_of(state(model), mc.case_config(c))
    loc = torch.full((c["b"], int(np.prod(c["dims"])) * c["C"]), float("nan"), device="cuda")
    probs = lambda e, o_, tag: cc.check_probs(loc, o_.last["loc"], tag)
    steps_vs_reference(cc.WithLoc(eng, loc), model, o, x, y, eps, 1.0, "%s %s" % (name, route), 0, Z_ATOL_MC,
                       checks=[check_channels, probs], **outs)                  # (0: ADAM_BAR[None])
    return c, model, eng, o, x, y


def plain(kl="sampled"):
    return lambda params, cfg: orc.SVIOracle(params, cfg, lr=LR, dtype=torch.float64, kl=kl)


# ------------------------------------------------------------------------------- 1. steps, both routes
@pytest.mark.parametrize("name,route", cc.STEP_CELLS)
def test_steps_vs_reference(gpu_device, categorical_oracle, name, route):
    run_steps(name, route, plain())


@pytest.mark.parametrize("route", ["fused", "layered"])
def test_analytic_kl_steps(gpu_device, categorical_oracle, route):
    run_steps(cc.CASE1, route, plain("analytic"), dict(kl="analytic"))


def test_63_positions_run_layered_whatever_is_asked(gpu_device):
    c = cc.CASES["k05_7x9_rt_c3_b3_72_40_softplus"]
    eng = cc.make_model(c, "cuda").engine(fused_channels=True)
    assert eng.uses_fused(c["b"]) is False
    assert "layer-by-layer" in _abi.categorical_decoder_kernel_name(eng._plan(c["b"]), 0, 1)


# ------------------------------------------------------------------------------- 2. observation weights
@pytest.mark.parametrize("route", ["fused", "layered"])
def test_shared_disc_mask(gpu_device, categorical_oracle, route):
    c = cc.CASES[cc.CASE1]
    w = pwc.disc(c["dims"], c["C"])
    run_steps(cc.CASE1, route, lambda params, cfg: pwc.WeightedOracle(params, cfg, w, lr=LR, dtype=torch.float64),
              dict(pixel_weights=w), weighted=1)


@pytest.mark.parametrize("route", ["fused", "layered"])
def test_per_image_mask_with_an_all_zero_image(gpu_device, categorical_oracle, route):
    c = cc.CASES[cc.CASE1]
    w = iwc.pdisc(c["b"], c["dims"], c["C"])
    w[2] = 0.0
    _, model, eng, o, x, y = run_steps(cc.CASE1, route,
                                       lambda params, cfg: iwc.ImageWeightedOracle(params, cfg, w, lr=LR, dtype=torch.float64),
                                       dict(image_weights=True), weighted=2, image_weights=w.cuda())
    # image 2 leaves only its KL terms: changing its labels changes nothing but what the encoder makes of them — with the
    # encoder's view held (same x), the reference's ll of that image is exactly 0
    assert o.last["ll_per_sample"][2].item() == 0.0, o.last["ll_per_sample"][2].item()
    eps = cc.case_data(c)[2][0]
    loc = torch.full((c["b"], 64 * c["C"]), float("nan"), device="cuda")
    eng.loss_and_grads(x.cuda(), eps.cuda(), 1.0, image_weights=w.cuda(), loc_out=loc)
    torch.cuda.synchronize()
    assert torch.isfinite(loc).all() and torch.isfinite(eng.grad[:eng.n_flat]).all()


@pytest.mark.parametrize("route", ["fused", "layered"])
def test_weights_of_ones_are_bit_identical_to_the_unweighted_call(gpu_device, route):
    c = cc.CASES[cc.CASE1]
    x, y, eps = cc.case_data(c)
    ones = torch.ones(*c["dims"], c["C"])
    out = []
    for kw, iw in ((dict(), None), (dict(pixel_weights=ones), None), (dict(image_weights=True), ones.expand(c["b"], *ones.shape))):
        _, model, eng = make(cc.CASE1, route, **kw)
        extra = {} if iw is None else dict(image_weights=iw.contiguous().cuda())
        eng.loss_and_grads(x.cuda(), eps[0].cuda(), 1.0, **extra)
        torch.cuda.synchronize()
        out.append((eng.scalars.clone(), eng.grad[:eng.n_flat].clone()))
    for k in (1, 2):
        assert torch.equal(out[0][0], out[k][0]), (route, k, out[0][0].tolist(), out[k][0].tolist())
        assert torch.equal(out[0][1], out[k][1]), (route, k, (out[0][1] - out[k][1]).abs().max().item())


# ------------------------------------------------------------------------------- 3. several particles, the Renyi bound (layered)
def test_particle_steps(gpu_device, categorical_oracle):
    P = 3
    c = cc.CASES[cc.CASE1]
    model = cc.make_model(c, "cuda")
    eng = model.engine(fused=0, particles=P)
    x, y, eps = cc.case_data(c, particles=P)
    o = orc.SVIOracle(state(model), mc.case_config(c), lr=LR, dtype=torch.float64, particles=P)
    steps_vs_reference(eng, model, o, x, y, eps, 1.0, "%s P=%d" % (cc.CASE1, P), 0, Z_ATOL_MC, checks=[check_channels])


@pytest.mark.parametrize("alpha", [0.0, 0.5])
def test_renyi_steps(gpu_device, categorical_oracle, alpha):
    """tests/test_gpu_renyi.py's composition: scalars and z at the project's bars against the free-weight reference, the weights
    at 2 |1 - alpha| 2e-5 max |ll|, the gradients at 1e-4 against the reference with the engine's weights held."""
    P = 3
    c = cc.CASES[cc.CASE1]
    b = c["b"]
    model = cc.make_model(c, "cuda")
    cfg = mc.case_config(c)
    eng = model.engine(fused=0, particles=P, renyi=alpha)
    x, y, eps = cc.case_data(c, particles=P)
    zl, zs = torch.empty(b, cfg.z_dim, device="cuda"), torch.empty(b, cfg.z_dim, device="cuda")
    w = torch.full((P * b,), float("nan"), device="cuda")
    o = None
    for k in range(2):
        tag = "%s alpha=%g step %d" % (cc.CASE1, alpha, k)
        eng.loss_and_grads(x.cuda(), eps[k].cuda(), 1.0, None, z_out=(zl, zs), weights_out=w)
        torch.cuda.synchronize()
        of, g_free, o = free_and_held(state(model), cfg, P, alpha, x, eps[k], 1.0, y, w, o)
        check_scalars(eng.scalars.cpu().numpy(), of, tag)
        check_z(zl, zs, of, RTOL_KL, Z_ATOL_MC, tag)
        weight_check(tag, w, of, alpha, RTOL_ELBO)
        check_grads(eng, o, tag + ", the engine's weights held")
        check_channels(eng, o, tag)
        eng.adam_step()
        check_params_after_adam(model, o, 0, tag)
        reload(model, o)


# ------------------------------------------------------------------------------- 4. stability
@pytest.mark.parametrize("route", ["fused", "layered"])
def test_logits_of_a_hundred(gpu_device, categorical_oracle, route):
    """decoder.out.weight scaled so that |logit| reaches ~100: exp(a) overflows fp32, exp(a - max) does not.  Loss, loc and every
    gradient finite and at the step cells' bars against the float64 reference."""
    c, model, eng = make(cc.CASE1, route)
    with torch.no_grad():
        model.decoder.out.weight.mul_(cc.STABILITY_SCALE)
    eng.bind()                                         # (the flat buffers from the scaled parameters)
    assert_route(eng, c, route)
    x, y, eps = cc.case_data(c)
    o = orc.SVIOracle(state(model), mc.case_config(c), lr=LR, dtype=torch.float64)
    loc = torch.full((c["b"], 64 * c["C"]), float("nan"), device="cuda")
    zl, zs = torch.empty(c["b"], o.cfg.z_dim, device="cuda"), torch.empty(c["b"], o.cfg.z_dim, device="cuda")
    eng.loss_and_grads(x.cuda(), eps[0].cuda(), 1.0, z_out=(zl, zs), loc_out=loc)
    torch.cuda.synchronize()
    o.step(x, eps[0], 1.0)
    tag = "stability %s" % route
    print("%s: largest |logit| in the reference %.1f" % (tag, o.last["loc"].abs().max().item()))
    assert torch.isfinite(eng.scalars).all() and torch.isfinite(eng.grad[:eng.n_flat]).all(), tag
    check_scalars(eng.scalars.cpu().numpy(), o.last, tag)
    check_z(zl, zs, o.last, RTOL_KL, Z_ATOL_MC, tag)
    cc.check_probs(loc, o.last["loc"], tag)
    check_grads(eng, o, tag)
    check_channels(eng, o, tag)


# ------------------------------------------------------------------------------- 5. decode, evaluate, the one-call step, repeats
@pytest.mark.parametrize("name,route", [(cc.CASE1, "fused"), (cc.CASE1, "layered"), (cc.CASE_VANILLA, "layered")])
def test_decode_and_manifold_are_probabilities(gpu_device, categorical_oracle, name, route):
    c, model, eng = make(name, route)
    o = orc.SVIOracle(state(model), mc.case_config(c), dtype=torch.float64)
    z = torch.randn(5, 2, generator=torch.Generator().manual_seed(2))
    kw = dict(angle=0.3, shift=[0.1, -0.2], scale=1.2) if c["inv"] else {}
    dec = model.decode(z, **kw)
    assert tuple(dec.shape) == (5,) + tuple(c["dims"]) + (c["C"],)
    want = o.decode(z, None, 0.3, [0.1, -0.2], 1.2) if c["inv"] else o.decode(z)
    cc.check_probs(dec.reshape(5, -1), want, "%s %s decode" % (name, route))
    man = model.manifold2d(3, plot=False)
    assert tuple(man.shape) == (9,) + tuple(c["dims"]) + (c["C"],)
    np.testing.assert_allclose(man.sum(-1).numpy(), 1.0, rtol=0, atol=1e-6)


@pytest.mark.parametrize("route", ["fused", "layered"])
def test_evaluate_repeat_and_one_call_step(gpu_device, route):
    c = cc.CASES[cc.CASE1]
    x, y, eps = cc.case_data(c)
    xg = x.cuda()
    (_, m1, e1), (_, m2, e2) = make(cc.CASE1, route), make(cc.CASE1, route)
    # a repeated call: the same bits; evaluate: the loss of loss_and_grads(want_grads=False)
    e1.loss_and_grads(xg, eps[0].cuda(), 1.0)
    torch.cuda.synchronize()
    first, s_first = e1.grad[:e1.n_flat].clone(), e1.scalars.clone()
    e1.loss_and_grads(xg, eps[0].cuda(), 1.0)
    torch.cuda.synchronize()
    assert torch.equal(first, e1.grad[:e1.n_flat]) and torch.equal(s_first, e1.scalars) and torch.isfinite(first).all()
    e1.loss_and_grads(xg, eps[0].cuda(), 1.0, want_grads=False)
    torch.cuda.synchronize()
    forward = e1.scalars.clone()
    e1.loss_and_grads(xg, eps[0].cuda(), 1.0, want_grads=False)
    torch.cuda.synchronize()
    assert torch.equal(forward, e1.scalars) and torch.isfinite(forward).all()
    # (the gradient call and the forward-only one sum the same per-row values in different blocked orders: 2e-6, as
    #  tests/test_gpu_multichannel_fused.py holds it)
    np.testing.assert_allclose(forward.cpu().numpy(), s_first.cpu().numpy(), rtol=2e-6)
    # step=True against the two-call sequence: the same bits, over two steps
    for k in range(2):
        e1.loss_and_grads(xg, eps[k].cuda(), 1.0)
        s1 = e1.scalars.clone()
        e1.adam_step()
        hist = torch.zeros(4, device="cuda")
        e2.loss_and_grads(xg, eps[k].cuda(), 1.0, scalars_out=hist, step=True)
        assert torch.equal(s1, hist), (route, k, s1.tolist(), hist.tolist())
        for name, a, b_ in (("params", e1.flat, e2.flat), ("m", e1.m, e2.m), ("v", e1.v, e2.v)):
            assert torch.equal(a, b_), (route, k, name, (a - b_).abs().max().item())


# ------------------------------------------------------------------------------- 6. trainer
def test_trainer_history(gpu_device, categorical_oracle):
    """SVItrainer(model, fused_channels=True).step(loader) for two epochs on the 8x8 case against SVIOracle.train_epoch (float64)
    driven by the same generator, at the loss bar; then evaluate against evaluate_epoch."""
    c = cc.CASES[cc.CASE1]
    x, _, _ = cc.case_data(c)
    loader = pv.utils.init_dataloader(x, batch_size=c["b"])
    model = cc.make_model(c, "cuda")
    params0 = state(model)
    tr = pv.trainers.SVItrainer(model, seed=1, fused_channels=True)
    assert_route(tr.engine, c, "fused")
    st = torch.get_rng_state()
    for _ in range(2):
        tr.step(loader)
    held_out = tr.evaluate(loader)
    torch.cuda.synchronize()
    torch.set_rng_state(st)
    o = orc.SVIOracle(params0, mc.case_config(c), lr=LR, dtype=torch.float64)
    want = [o.train_epoch(loader) for _ in range(2)]
    want_held_out = o.evaluate_epoch(loader)
    print("trainer: history %s, reference %s; evaluate %.6f, reference %.6f"
          % (tr.loss_history["training_loss"], want, held_out, want_held_out))
    np.testing.assert_allclose(tr.loss_history["training_loss"], want, rtol=RTOL_ELBO)
    np.testing.assert_allclose(held_out, want_held_out, rtol=RTOL_ELBO)
