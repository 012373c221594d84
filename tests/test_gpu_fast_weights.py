"""
GPU tests (-m gpu) of fast_weights=True: weighted steps (pixel_weights= / image_weights=) on the weighted instances of the 4-wave
bf16-class fused decoder kernel, pv_sdec_fused_bf16_wt_kernel<GRADS, LIK, PREC> — PV_PLAN_FAST_WEIGHTS in the C ABI.

Cases, weights, references and the plain-bf16 route's bars come from tests/_fast_weight_cases.py.  Every case runs on both routes:
  x3    (fused = 2): float64 WeightedOracle / ImageWeightedOracle, two steps with Adam between, each from identical float32
        parameters, at the constants of tests/_judge.py as they stand — loss and ll 2e-5 (+ _multichannel_cases.loss_atol for the
        continuous Bernoulli), the KL scalars 1e-4, z_loc / z_scale rtol 1e-4 atol 2e-6, loc_out rtol 1e-4 atol 2e-6, every
        gradient tensor 1e-4 relative L2, the parameters after Adam at ADAM_BAR[2] (the 1 % cap on near-zero gradient entries is
        confirmed with the references alone in tests/test_fast_weights_cpu.py);
  bf16  (fused = 3): tests/_bf16_judge.judge against the same oracles over a Config that restates the 4-wave build's roundings
        (oracle/bf16_plan.py, kernel "w4"), two steps, at the case's bars, with the judge's self-check (a tensor more than 1e-3 from
        float64 lies at least 10x closer to the emulation).
Then which kernel ran, the relations between calls, the trainer, and that nothing changes without the keyword.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import pyroved_amd as pv
from pyroved_amd import _abi
import _multichannel_cases as mc
import _pixel_weight_cases as pw
import _image_weight_cases as iwc
import _fast_weight_cases as fw
from _bf16_judge import judge, SELF_CHECK
from _device import cus
from _judge import Z_ATOL, LR, rel_l2, state, steps_vs_reference, cpu_threads_16

pytestmark = pytest.mark.gpu

ROUTES = sorted(fw.ROUTES)
OWN = "f04_8x8_rts_b256_cbern_pramp"           # batch == grid: the own-sample epilogue, Adam riding in the closing launch


def build(c, route, **kw):
    """(model, engine) of a case on a route."""
    model = pv.models.iVAE(c["dims"], 2, c["inv"], seed=1, device="cuda", **mc.model_kwargs(c))
    return model, model.engine(**fw.engine_kw(c, route, **kw))


def check_kernel(eng, c, route):
    """The plan carries the flag and keeps `fused`; the hook names the weighted 4-wave instance of the route's build."""
    plan = eng._plan(c["b"])
    assert plan.flags & _abi.PV_PLAN_FAST_WEIGHTS and plan.fused == fw.ROUTES[route]
    for grads in (True, False):
        name = _abi.weighted_decoder_kernel_name(plan, fw.per_image(c), grads)
        assert name == fw.kernel_name(c, route, grads), name
    assert eng.uses_fused(c["b"]) is True and eng.supports_dp_step is False


def n_obs(c):
    return int(np.prod(c["dims"]))


def _kl_kw(kl):
    return {} if kl == "sampled" else dict(kl=kl)


STEP_PARAMS = [(n, "sampled") for n in sorted(fw.CASES)] + [(n, "analytic") for n in fw.ANALYTIC]


# ------------------------------------------------------------------------------- 1. parity, x3 route
@pytest.mark.parametrize("name,kl", STEP_PARAMS)
def test_x3_steps_vs_reference(gpu_device, name, kl):
    c = fw.CASES[name]
    model, eng = build(c, "x3", **_kl_kw(kl))
    check_kernel(eng, c, "x3")
    x, y, eps = fw.case_data(c)
    o = fw.oracle(c, state(model), "x3", kl, lr=LR)
    loc = torch.full((c["b"], n_obs(c)), float("nan"), device="cuda")
    steps_vs_reference(eng, model, o, x, y, eps, 1.0, "%s x3 %s" % (name, kl), 2, Z_ATOL, atol=mc.loss_atol(c), loc_out=loc,
                       **fw.call_kw(c))


def test_x3_pixel_and_image_weights_together_vs_reference(gpu_device):
    """f01 with pixel_weights AND image_weights: the reference weighs with the product."""
    c = fw.CASES[fw.CASE1]
    p, w = pw.ramp(tuple(c["dims"]), 1)[..., 0], iwc.pdisc(c["b"], tuple(c["dims"]), 1)[..., 0].contiguous()
    w[2] = 0.0
    model = pv.models.iVAE(c["dims"], 2, c["inv"], seed=1, device="cuda", **mc.model_kwargs(c))
    eng = model.engine(fused=2, fast_weights=True, pixel_weights=p, image_weights=True)
    assert _abi.weighted_decoder_kernel_name(eng._plan(c["b"]), 1, 1) == fw.kernel_name(c, "x3")
    x, y, eps = fw.case_data(c)
    o = iwc.ImageWeightedOracle(state(model), fw.config(c), w * p.unsqueeze(0), lr=LR, dtype=torch.float64)
    steps_vs_reference(eng, model, o, x, y, eps, 1.0, "f01 x3 pixel x image", 2, Z_ATOL, image_weights=w.cuda())


# ------------------------------------------------------------------------------- 2. parity, plain-bf16 route
def _reference(c, params, route, kl, x, eps, y):
    o = fw.oracle(c, params, route, kl, cus=cus())
    out = o.loss_and_grads(x, eps, 1.0, y)
    return out, {k: v.grad.detach().clone() for k, v in o.p.items()}


@pytest.mark.parametrize("name,kl", STEP_PARAMS)
def test_bf16_steps_vs_emulation(gpu_device, name, kl):
    """Two steps (the second from the engine's own parameters after its Adam step), each judged against the emulation and
    float64 on the parameters the step started from."""
    c = fw.CASES[name]
    model, eng = build(c, "bf16", **_kl_kw(kl))
    check_kernel(eng, c, "bf16")
    x, y, eps = fw.case_data(c)
    xg, yg = x.cuda(), None if y is None else y.cuda()
    zl, zs = (torch.empty(c["b"], eps[0].shape[1], device="cuda") for _ in range(2))
    grad_bar, loss_bar = fw.BF16_BARS[name]
    for k in range(2):
        params = state(model)
        eng.loss_and_grads(xg, eps[k].cuda(), 1.0, yg, z_out=(zl, zs), **fw.call_kw(c))
        torch.cuda.synchronize()
        ref_out, ref_g = _reference(c, params, "bf16", kl, x, eps[k], y)
        f64_out, f64_g = _reference(c, params, "x3", kl, x, eps[k], y)
        tag = "%s bf16 %s step %d" % (name, kl, k)
        rows = judge(tag, eng, ref_out, ref_g, f64_out, f64_g, zl.cpu(), zs.cpu(), grad_bar, loss_bar, SELF_CHECK)
        print("[fast-weights bf16 measured] %s: worst gradient %.3e, loss %.3e" % (tag, max(r[1] for r in rows[3:]), rows[0][1]))
        eng.adam_step()
        torch.cuda.synchronize()


# ------------------------------------------------------------------------------- 3. relations between calls
def _scalars_and_grads(eng):
    torch.cuda.synchronize()
    return eng.scalars.clone(), eng.grad.clone()


def _per_tensor_equal(model, eng, a, b):
    for k, v in model.state_dict().items():                     # (per tensor: the flat buffer's alignment padding is never written)
        lo, n = eng._layout[k], v.numel()
        if not torch.equal(a[lo:lo + n], b[lo:lo + n]):
            return False
    return torch.equal(a[-4:], b[-4:])


def _inputs(c):
    x, y, eps = fw.case_data(c)
    return x.cuda(), None if y is None else y.cuda(), [e.cuda() for e in eps]


@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("name", [fw.CASE1, OWN, "f05_8x8_r_cdim2_b352_poisson_pramp"])
def test_evaluate_and_repeat(gpu_device, name, route):
    """want_grads=False gives the gradient call's four scalars to 2e-6; a repeated call is bit-identical, outputs poisoned in
    between."""
    c = fw.CASES[name]
    model, eng = build(c, route)
    xg, yg, eps = _inputs(c)
    kw = fw.call_kw(c)
    eng.loss_and_grads(xg, eps[0], 1.0, yg, **kw)
    s, g = _scalars_and_grads(eng)
    eng.grad.fill_(float("nan"))
    eng.scalars.fill_(float("nan"))
    eng.loss_and_grads(xg, eps[0], 1.0, yg, **kw)
    s2, g2 = _scalars_and_grads(eng)
    assert torch.isfinite(s).all() and torch.equal(s, s2) and _per_tensor_equal(model, eng, g, g2)
    eng.scalars.fill_(float("nan"))
    eng.loss_and_grads(xg, eps[0], 1.0, yg, want_grads=False, **kw)
    torch.cuda.synchronize()
    print("%s %s: evaluate %s, gradient call %s" % (name, route, eng.scalars.tolist(), s.tolist()))
    np.testing.assert_allclose(eng.scalars.cpu().numpy(), s.cpu().numpy(), rtol=2e-6)


@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("name", [fw.CASE1, OWN])
def test_step_in_one_call_is_the_two_calls(gpu_device, name, route):
    """loss_and_grads(step=True) against loss_and_grads + adam_step: parameters, moments and scalars bit for bit, two steps."""
    out = []
    c = fw.CASES[name]
    for one_call in (True, False):
        model, eng = build(c, route)
        xg, yg, eps = _inputs(c)
        kw = fw.call_kw(c)
        sc = torch.zeros(2, 4, device="cuda")
        for k in range(2):
            if one_call:
                eng.loss_and_grads(xg, eps[k], 1.0, yg, scalars_out=sc[k], step=True, **kw)
            else:
                eng.loss_and_grads(xg, eps[k], 1.0, yg, scalars_out=sc[k], **kw)
                eng.adam_step()
        torch.cuda.synchronize()
        out.append((eng.flat.clone(), eng.m.clone(), eng.v.clone(), sc.clone()))
    for a, b, what in zip(out[0], out[1], ("parameters", "m", "v", "scalars")):
        assert torch.equal(a, b), what
    assert torch.isfinite(out[0][0]).all() and torch.isfinite(out[0][3]).all()


@pytest.mark.parametrize("route", ROUTES)
def test_pixel_and_image_weights_multiply(gpu_device, route):
    """pixel_weights=p together with image_weights=w equals image_weights=w * p, bit for bit."""
    c = fw.CASES[fw.CASE1]
    xg, yg, eps = _inputs(c)
    w = iwc.pdisc(c["b"], tuple(c["dims"]), 1)[..., 0].contiguous()
    p = pw.ramp(tuple(c["dims"]), 1)[..., 0]
    kw = dict(fused=fw.ROUTES[route], fast_weights=True, image_weights=True)
    mb = pv.models.iVAE(c["dims"], 2, c["inv"], seed=1, device="cuda")
    eb = mb.engine(pixel_weights=p, **kw)
    eb.loss_and_grads(xg, eps[0], 1.0, image_weights=w.cuda())
    s0, g0 = _scalars_and_grads(eb)
    mp = pv.models.iVAE(c["dims"], 2, c["inv"], seed=1, device="cuda")
    ep = mp.engine(**kw)
    ep.loss_and_grads(xg, eps[0], 1.0, image_weights=(w * p.unsqueeze(0)).cuda())
    s1, g1 = _scalars_and_grads(ep)
    assert torch.equal(s0, s1) and _per_tensor_equal(mp, ep, g0, g1)
    ep.loss_and_grads(xg, eps[0], 1.0, image_weights=w.cuda())
    s2, _ = _scalars_and_grads(ep)
    assert not torch.equal(s2, s1)                                     # (the shared weights do something)


@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("name", [fw.CASE1, "f02_1d32_t_b5_gauss_nosig_ramp"])
def test_shared_weights_repeated_per_image(gpu_device, name, route):
    """The shared weights repeated B times as image_weights equal the pixel_weights= call bit for bit: the same kernel instance,
    the index chosen at run time."""
    c = fw.CASES[name]
    xg, yg, eps = _inputs(c)
    ms, es = build(c, route)
    es.loss_and_grads(xg, eps[0], 1.0, yg)
    s0, g0 = _scalars_and_grads(es)
    mi = pv.models.iVAE(c["dims"], 2, c["inv"], seed=1, device="cuda", **mc.model_kwargs(c))
    ei = mi.engine(fused=fw.ROUTES[route], fast_weights=True, image_weights=True)
    assert (_abi.weighted_decoder_kernel_name(ei._plan(c["b"]), 1, 1) == _abi.weighted_decoder_kernel_name(es._plan(c["b"]), 0, 1)
            == fw.kernel_name(c, route))
    ei.loss_and_grads(xg, eps[0], 1.0, yg, image_weights=iwc.shared_as_images(c)[..., 0].contiguous().cuda())
    s1, g1 = _scalars_and_grads(ei)
    assert torch.equal(s0, s1) and _per_tensor_equal(mi, ei, g0, g1)


@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("name", [fw.CASE1, "f07_28x28_rt_b6_gauss_pdisc"])
def test_weights_of_ones_are_the_unweighted_step(gpu_device, name, route):
    """Weights of ones against the unweighted engine forced to the same build (dec_kernel = 1): scalars and every gradient tensor
    to 2e-6 on the x3 route, to the case's bars on the plain-bf16 route; whether they were bit-identical is printed."""
    c = fw.CASES[name]
    xg, yg, eps = _inputs(c)
    mu = pv.models.iVAE(c["dims"], 2, c["inv"], seed=1, device="cuda", **mc.model_kwargs(c))
    eu = mu.engine(fused=fw.ROUTES[route])
    eu.dec_kernel = 1
    eu.loss_and_grads(xg, eps[0], 1.0, yg)
    s0, g0 = _scalars_and_grads(eu)
    mw = pv.models.iVAE(c["dims"], 2, c["inv"], seed=1, device="cuda", **mc.model_kwargs(c))
    ew = mw.engine(fused=fw.ROUTES[route], fast_weights=True, image_weights=True)
    ew.loss_and_grads(xg, eps[0], 1.0, yg, image_weights=torch.ones(c["b"], *c["dims"], device="cuda"))
    s1, g1 = _scalars_and_grads(ew)
    same = torch.equal(s0, s1) and _per_tensor_equal(mw, ew, g0, g1)
    print("%s %s: weights of ones bit-identical to the unweighted dec_kernel = 1 step: %s" % (name, route, same))
    grad_bar, loss_bar = (2e-6, 2e-6) if route == "x3" else fw.BF16_BARS[name]
    np.testing.assert_allclose(s1.cpu().numpy(), s0.cpu().numpy(), rtol=loss_bar)
    for k, v in mw.state_dict().items():
        lo, n = ew._layout[k], v.numel()
        assert rel_l2(g1[lo:lo + n], g0[lo:lo + n]) < grad_bar, k


@pytest.mark.parametrize("route", ROUTES)
def test_zero_weight_rows_give_exact_zeros(gpu_device, route):
    """A zero weight removes a row exactly, whatever its unweighted values: a Poisson model on 8 x 8 with the shared disc mask,
    once with counts of 1e6 at the masked positions (unweighted dL/dlogit ~ -1e6 there) and once with zeros.  The encoder's
    first-layer columns of the masked positions are zeroed, so both runs decode the same z: the four scalars and every gradient are
    bit-identical, but for those columns' own gradient (dW[:, j] sums x_bj, which differs by construction)."""
    dims, b = (8, 8), 6
    mask = pw.disc(dims, 1)[..., 0]
    off = (mask.flatten() == 0)
    assert 0 < int(off.sum()) < mask.numel()
    g = torch.Generator().manual_seed(0)
    x = mc.counts(g, b, dims, 1)[..., 0].contiguous()
    eps = torch.randn(b, 6, generator=g).cuda()                       # (z_dim: 2 + rotation, two shifts, scale)
    res = []
    for big in (1.0e6, 0.0):
        model = pv.models.iVAE(dims, 2, ["r", "t", "s"], seed=1, device="cuda", sampler_d="poisson_log", sigmoid_d=False)
        with torch.no_grad():
            model.encoder_z.fc_layers[0].weight[:, off.cuda()] = 0.0
        eng = model.engine(fused=fw.ROUTES[route], fast_weights=True, pixel_weights=mask)
        xb = torch.where(mask.unsqueeze(0) == 0, torch.full_like(x, big), x).cuda()
        eng.loss_and_grads(xb, eps, 1.0)
        torch.cuda.synchronize()
        res.append((eng.scalars.clone(), {k: eng.grad_of(k).clone() for k in model.state_dict()}))
    (s0, g0), (s1, g1) = res
    print("%s: scalars with 1e6 under the mask %s, with zeros %s" % (route, s0.tolist(), s1.tolist()))
    assert torch.isfinite(s0).all() and torch.equal(s0, s1)
    for k in g0:
        a, c_ = g0[k], g1[k]
        if k == "encoder_z.fc_layers.0.weight":
            a, c_ = a[:, ~off.cuda()], c_[:, ~off.cuda()]
        assert torch.isfinite(a).all() and torch.equal(a, c_), k


# ------------------------------------------------------------------------------- 4. trainer
def test_trainer_history_feeds_and_reference(gpu_device):
    """f01's data as 20 images, batch 6 (a last batch of 2), shuffle=True, two epochs plus evaluate with precision="bf16",
    image_weights=True, fast_weights=True: the history with the device feed equals the one without bit for bit, and both equal
    an emulated-oracle loop over the same loader pass to the case's loss bar."""
    c = fw.CASES[fw.CASE1]
    n = 20
    x = mc.images(torch.Generator().manual_seed(0), n, c["dims"], 1)[..., 0].contiguous()
    w = iwc.pdisc(n, tuple(c["dims"]), 1)[..., 0].contiguous()
    w[5] = 0.0                                                         # one image masked out completely
    loader = pv.utils.init_dataloader(x, w, batch_size=6, shuffle=True)
    hist = []
    for device_feed in (True, False):
        model = pv.models.iVAE(c["dims"], 2, c["inv"], seed=1, device="cuda", **mc.model_kwargs(c))
        params0 = state(model)
        tr = pv.trainers.SVItrainer(model, seed=1, precision="bf16", image_weights=True, fast_weights=True, device_feed=device_feed)
        assert tr.engine.uses_fused(6) is True and tr.engine.fused == 3 and tr.engine.fast_weights is True
        assert _abi.weighted_decoder_kernel_name(tr.engine._plan(6), 1, 1) == fw.kernel_name(c, "bf16")
        st = torch.get_rng_state()
        for _ in range(2):
            tr.step(loader)
        got_eval = tr.evaluate(loader)
        torch.cuda.synchronize()
        assert (tr._feed_cache is not None) == device_feed
        hist.append(tr.loss_history["training_loss"] + [got_eval])
    assert hist[0] == hist[1], hist
    torch.set_rng_state(st)
    o = iwc.ImageWeightedOracle(params0, fw.config(c, "bf16", cus()), w[:1], lr=LR, dtype=torch.float64)

    def epoch(train):
        total = 0.0
        with torch.set_grad_enabled(train):
            for xb, wb in loader:
                o.set_weights(wb)
                total += o.step(xb, o.draw_eps(xb.shape[0]), 1.0, None)
        return total / n
    want = [epoch(True), epoch(True), epoch(False)]
    err = [abs(a - b) / abs(b) for a, b in zip(hist[0], want)]
    print("trainer: history + evaluate %s, reference %s, relative errors %s" % (hist[0], want, err))
    np.testing.assert_allclose(hist[0], want, rtol=fw.BF16_BARS[fw.CASE1][1])


# ------------------------------------------------------------------------------- 5. without the keyword nothing changes
def test_without_the_keyword_nothing_changes(gpu_device):
    """A weighted engine without fast_weights has today's plan: no flag, fused = 1, the weighted f32 kernel's workspace and name;
    its step is bit-identical before and after fast_weights was configured and removed again."""
    c = fw.CASES[fw.CASE1]
    model = pv.models.iVAE(c["dims"], 2, c["inv"], seed=1, device="cuda")
    eng = model.engine(image_weights=True)
    xg, yg, eps = _inputs(c)
    wg = iwc.weights(iwc.CASES[iwc.CASE1]).cuda()
    lib = _abi.lib()
    plan = eng._plan(c["b"])
    assert eng.fast_weights is False and plan.flags == 0 and plan.fused == 1 and eng._plan_fused() == 1 and plan.dec_kernel == 0
    assert eng.uses_fused(c["b"]) is True
    ws0 = eng.ws.numel()
    f32 = _abi.pv_ivae_plan.from_buffer_copy(plan)
    f32.flags = _abi.PV_PLAN_FAST_WEIGHTS                              # (fused == 1: the bit does nothing)
    assert ws0 == lib.pv_ivae_weighted_workspace_bytes(C.byref(plan)) == lib.pv_ivae_weighted_workspace_bytes(C.byref(f32))
    for per_image, grads in ((1, 1), (1, 0), (0, 1)):
        want = "void pv_sdec_fused_mc_kernel<%s, 1, %d>(PvFused)" % ("true" if grads else "false", 2 if per_image else 1)
        assert _abi.weighted_decoder_kernel_name(plan, per_image, grads) == want
    eng.loss_and_grads(xg, eps[0], 1.0, image_weights=wg)
    s0, g0 = _scalars_and_grads(eng)
    eng.configure(fast_weights=True)
    plan = eng._plan(c["b"])
    assert plan.flags == _abi.PV_PLAN_FAST_WEIGHTS and plan.fused == 2
    eng.loss_and_grads(xg, eps[0], 1.0, image_weights=wg)
    s1, g1 = _scalars_and_grads(eng)
    np.testing.assert_allclose(s1.cpu().numpy(), s0.cpu().numpy(), rtol=2e-5)      # (two fp32-class kernels)
    eng.configure(fast_weights=False)
    plan = eng._plan(c["b"])
    assert plan.flags == 0 and plan.fused == 1
    eng.grad.fill_(float("nan"))
    eng.loss_and_grads(xg, eps[0], 1.0, image_weights=wg)
    s2, g2 = _scalars_and_grads(eng)
    assert eng.ws.numel() == ws0 and torch.equal(s0, s2) and _per_tensor_equal(model, eng, g0, g2)
