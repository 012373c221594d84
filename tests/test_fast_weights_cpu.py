"""
fast_weights=True — PV_PLAN_FAST_WEIGHTS in the C ABI: weighted steps on the weighted instances of the 4-wave bf16-class fused decoder
kernel — where no GPU is needed: the flag and the test hook, the routing table at plan level (tests/_plan_kit.py plans: 784
positions x ch observations, batch 16), every ValueError of the engine and the trainer with the configure rollback, the keyword's way
through the trainer, the references the GPU tests use (tests/_fast_weight_cases.py) — the emulated composition, the condition the
parameter check rests on, and that the checked gradients see the weights.
"""
import ctypes as C
import functools
import inspect
import os
import re

import pytest
import torch

from conftest import ROOT

import pyroved_amd as pv
from pyroved_amd import _abi
import _multichannel_cases as mc
import _fast_weight_cases as fw
from _judge import ILL_SHARE, RTOL_GRAD, near_zero_share, rel_l2, state
from _plan_kit import _plan, _vanilla_plan

EINVAL = -1
FLAG = 512
KW = "fast_weights"
NO_ENC_FOLD = 16


# ------------------------------------------------------------------------------- C ABI
def test_flag_hook_and_unchanged_abi():
    src = open(os.path.join(ROOT, "include", "pyroved_amd.h")).read()
    assert re.search(r"^#define PV_PLAN_FAST_WEIGHTS 512$", src, re.M)
    assert _abi.PV_PLAN_FAST_WEIGHTS == FLAG
    assert "pv_debug_weighted_decoder_kernel_name" not in src                       # a test hook, outside the header
    assert "pv_debug_weighted_decoder_kernel_name" not in _abi.SIGNATURES
    assert getattr(_abi.lib(), "pv_debug_weighted_decoder_kernel_name") is not None
    assert _abi.PV_ABI_VERSION == 17 and _abi.lib().pv_version() == 17 and C.sizeof(_abi.pv_ivae_plan) == 2824
    for bit in ("PV_PLAN_ENC_TWO_LAUNCH", "PV_PLAN_NO_SIDE_STREAM", "PV_PLAN_ENC_NO_WAIT", "PV_PLAN_NO_DEC1D", "PV_PLAN_NO_ENC_FOLD",
                "PV_PLAN_ENC_TILED", "PV_PLAN_CONV_X3", "PV_PLAN_GENERIC_TILE_LOOP", "PV_PLAN_FUSED_CHANNELS"):
        assert getattr(_abi, bit) & FLAG == 0, bit


def _answers(p, keep):
    lib = _abi.lib()
    w = C.addressof(keep)
    calls = (lib.pv_ivae_weighted_loss_and_grads(C.byref(p), w, 1, None), lib.pv_ivae_weighted_loss_and_grads(C.byref(p), w, 0, None),
             lib.pv_ivae_weighted_step(C.byref(p), w, None), lib.pv_ivae_weighted_images_loss_and_grads(C.byref(p), w, 1, None),
             lib.pv_ivae_weighted_images_loss_and_grads(C.byref(p), w, 0, None), lib.pv_ivae_weighted_images_step(C.byref(p), w, None))
    assert calls == (EINVAL,) * 6                   # (in scope or not, a plan without buffers is refused before a pointer is touched)
    return (lib.pv_ivae_weighted_workspace_bytes(C.byref(p)), lib.pv_ivae_weighted_uses_fused(C.byref(p)),
            tuple(_abi.weighted_decoder_kernel_name(p, pi, g) for pi in (0, 1) for g in (1, 0)))


def _wt_names(prec):
    return tuple("void pv_sdec_fused_bf16_wt_kernel<%s, 0, %d>(PvFused, PvEncFold, int)" % (g, prec)
                 for _ in (0, 1) for g in ("true", "false"))


def _mc_names(ch):
    return tuple("void pv_sdec_fused_mc_kernel<%s, %d, %d>(PvFused)" % (g, ch, 2 if pi else 1) for pi in (0, 1) for g in ("true", "false"))


LAYERED = ("pv_gemm_kernel (layer-by-layer path)",) * 4
REFUSED = (EINVAL, 0, ("",) * 4)


@pytest.mark.parametrize("fused", (0, 1, 2, 3))
@pytest.mark.parametrize("ch", (1, 2, 3, 8))
def test_routing_table(fused, ch):
    """Flag on and off, dec_kernel 0, 1 and 28: what the workspace query, uses_fused and the name hook answer.  Without the flag:
    today's table.  With it: one channel with fused 2 / 3 and dec_kernel 0 / 1 keeps `fused` on the weighted 4-wave instances and
    takes the workspace of that plan with dec_kernel = 1 and PV_PLAN_NO_ENC_FOLD; fused == 2 elsewhere routes as without the flag;
    fused == 3 elsewhere and dec_kernel > 1 anywhere are PV_EINVAL."""
    lib = _abi.lib()
    keep = C.create_string_buffer(64)
    for dk in (0, 1, 28):
        valid = dk == 0 or (fused == 3 and dk == 1) or (fused == 2 and dk in (1, 28))       # (pv_sdec_fused_sel_valid)
        p = _plan(fused, ch)
        p.dec_kernel = dk
        off = _answers(p, keep)
        if not valid or fused == 3:
            assert off == REFUSED, (fused, ch, dk, off)
        elif ch == 1 and fused in (1, 2):
            assert off[0] > 0 and off[1:] == (1, _mc_names(1)), (fused, ch, dk, off)
            q = _plan(1, 1)
            assert off[0] == lib.pv_ivae_workspace_bytes_for(C.byref(q), 1)
        else:                                           # fused 0, or several channels without PV_PLAN_FUSED_CHANNELS
            assert off[0] > 0 and off[1:] == (0, LAYERED), (fused, ch, dk, off)
        p.flags = FLAG
        on = _answers(p, keep)
        if not valid or dk > 1:
            assert on == REFUSED, (fused, ch, dk, on)
        elif ch == 1 and fused in (2, 3):
            q = _plan(fused, 1)
            q.dec_kernel, q.flags = 1, NO_ENC_FOLD
            want_ws = lib.pv_ivae_workspace_bytes_for(C.byref(q), 1)
            assert want_ws > 0 and on == (want_ws, 1, _wt_names(1 if fused == 2 else 0)), (fused, ch, dk, on)
        else:
            assert on == off, (fused, ch, dk, on, off)
        p.flags = FLAG | _abi.PV_PLAN_FUSED_CHANNELS    # the two bits do not interact
        both = _answers(p, keep)
        p.flags = _abi.PV_PLAN_FUSED_CHANNELS
        if valid and not dk > 1 and not (ch == 1 and fused in (2, 3)):
            assert both == _answers(p, keep)


def test_routing_needs_the_kernels_architecture():
    """Flag set on plans the kernel does not take: fused == 2 routes as without it, fused == 3 stays refused."""
    keep = C.create_string_buffer(64)
    for tag, change in (("positions", lambda p: (setattr(p, "n_pix", 780), setattr(p.enc[0], "in_dim", 780))),
                        ("width", lambda p: (setattr(p.dec[1], "out_dim", 64), setattr(p.out, "in_dim", 64))),
                        ("activation", lambda p: setattr(p.dec[0], "act", _abi.ACT["softplus"]))):
        for fused in (2, 3):
            p = _plan(fused, 1)
            change(p)
            off = _answers(p, keep)
            p.flags = FLAG
            on = _answers(p, keep)
            assert on == off and (fused == 2 or on == REFUSED), (tag, fused, on, off)
            assert fused == 3 or (on[0] > 0 and on[1:] == (0, LAYERED)), (tag, on)
    for fused in (2, 3):
        p = _vanilla_plan(fused)
        off = _answers(p, keep)
        p.flags = FLAG
        assert _answers(p, keep) == off and (fused == 2 or off == REFUSED)


def test_unweighted_queries_ignore_the_flag():
    lib = _abi.lib()
    for fused in (0, 1, 2, 3):
        p, q = _plan(fused, 1), _plan(fused, 1)
        q.flags = FLAG
        for what in (0, 1, 2, 3):
            assert lib.pv_ivae_workspace_bytes_for(C.byref(p), what) == lib.pv_ivae_workspace_bytes_for(C.byref(q), what) > 0
        assert lib.pv_ivae_uses_fused(C.byref(p)) == lib.pv_ivae_uses_fused(C.byref(q))
        assert lib.pv_ivae_guide_folds(C.byref(p)) == lib.pv_ivae_guide_folds(C.byref(q))


# ------------------------------------------------------------------------------- Python: engine and trainer
def model(channels=1, dims=(8, 8), inv=("r", "t", "s"), **kw):
    return pv.models.iVAE(dims, 2, list(inv) if inv else None, channels=channels, seed=1, device="cpu", **kw)


@pytest.fixture
def unbound(monkeypatch):
    """Engines here never reach the device: bind() is stubbed (tests/test_pixel_weights_cpu.py does the same)."""
    from pyroved_amd.engine import IVAEEngine
    monkeypatch.setattr(IVAEEngine, "bind", lambda self: None)


W = dict(image_weights=True)


def test_engine_value_errors():
    def refused(m, match=KW, **kw):
        with pytest.raises(ValueError, match=match):
            m.engine(fast_weights=True, **kw)
        assert m._engine is None                                       # raised before anything was bound
    for fused in (2, 3):
        refused(model(), fused=fused)                                  # no weights
    for fused in (0, 1):
        refused(model(), fused=fused, **W)                             # contradiction
        refused(model(), fused=fused, pixel_weights=torch.ones(8, 8))
    # fused = 3 on a model the kernel does not take: the message names the condition
    refused(model(3), match="channels", fused=3, **W)
    refused(model(inv=None), match="vanilla", fused=3, **W)
    refused(model(hidden_dim_d=[72, 40]), match="two tanh layers of 128", fused=3, **W)
    refused(model(hidden_dim_d=[128, 128, 128]), match="two tanh layers of 128", fused=3, **W)
    refused(model(activation="softplus"), match="two tanh layers of 128", fused=3, **W)
    refused(model(dims=(7, 9), inv=("r", "t")), match="multiple of 16", fused=3, **W)
    for kw in (dict(particles=3), dict(renyi=0.0)):                    # the weighted step's own refusals stay
        refused(model(), match="image_weights", fused=2, **W, **kw)


def test_fused_2_keeps_todays_routing_on_other_models(unbound):
    for m in (model(3), model(inv=None), model(hidden_dim_d=[72, 40]), model(activation="softplus"),
              model(dims=(7, 9), inv=("r", "t"))):
        eng = m.engine(fused=2, fast_weights=True, **W)
        assert eng.fast_weights is True and eng._plan_flags() == 0
        eng2 = m.engine(fast_weights=False)
        assert eng2 is eng and eng._plan_flags() == 0
        assert eng._plan_fused() == (1 if eng.C == 1 else 2)             # (as the same model without the keyword)


def test_plan_bits(unbound):
    for fused in (2, 3):
        for kw in (W, dict(pixel_weights=torch.ones(8, 8)), dict(pixel_weights=torch.ones(8, 8), image_weights=True)):
            eng = model().engine(fused=fused, fast_weights=True, **kw)
            assert (eng._plan_fused(), eng._plan_flags()) == (fused, FLAG) and eng.supports_dp_step is False
    eng = model().engine(fused=2, **W)                                 # without the keyword: today's plan
    assert (eng._plan_fused(), eng._plan_flags(), eng.fast_weights) == (1, 0, False)
    eng = model().engine(fused=2)
    assert (eng._plan_fused(), eng._plan_flags(), eng.supports_dp_step) == (2, 0, True)
    eng = model().engine(fused=2, fast_weights=True, **W)
    eng.dec_kernel = 1
    assert eng._plan_flags() == FLAG
    eng.dec_kernel = 28
    with pytest.raises(ValueError, match=KW):
        eng.configure(lr=1e-3)


def test_configure_sets_removes_and_rolls_back(unbound):
    m = model()
    eng = m.engine(**W)
    assert eng.fast_weights is False and eng._plan_fused() == 1
    eng.ws = "kept"
    eng.configure(fast_weights=False)                                  # off on an engine without it: nothing is reset
    assert eng.ws == "kept"
    eng.configure(fast_weights=True)
    assert eng.fast_weights is True and eng.ws is None and (eng._plan_fused(), eng._plan_flags()) == (2, FLAG)
    eng.configure(lr=2e-3)                                             # None leaves the setting
    assert eng.fast_weights is True
    eng.configure(fused=3)                                             # allowed WITH the keyword
    assert (eng.fused, eng._plan_fused(), eng._plan_flags()) == (3, 3, FLAG)
    for kw in (dict(fused=0), dict(fused=1), dict(image_weights=False)):
        with pytest.raises(ValueError, match=KW):
            eng.configure(**kw)
        assert (eng.fused, eng.image_weights, eng.fast_weights) == (3, True, True)
    with pytest.raises(ValueError, match="image_weights"):             # fused = 3 without the keyword: today's message
        eng.configure(fast_weights=False)
    assert eng.fast_weights is True and eng.fused == 3
    eng.configure(fast_weights=False, fused=2)
    assert (eng.fast_weights, eng._plan_fused(), eng._plan_flags()) == (False, 1, 0)
    with pytest.raises(ValueError, match="image_weights"):
        eng.configure(fused=3)
    e2 = model().engine()                                              # an unweighted engine refuses the keyword and stays as it was
    with pytest.raises(ValueError, match=KW):
        e2.configure(fast_weights=True)
    assert e2.fast_weights is False and e2._plan_flags() == 0
    assert m.engine(fused=3, image_weights=True, fast_weights=True) is eng and eng._plan_flags() == FLAG


def test_trainer_keyword(unbound):
    m = model()
    tr = pv.trainers.SVItrainer(m, image_weights=True, fast_weights=True)
    assert tr.engine.fast_weights is True and (tr.engine.fused, tr.engine._plan_flags()) == (2, FLAG)
    tr = pv.trainers.SVItrainer(m, precision="bf16", pixel_weights=torch.ones(8, 8), fast_weights=True)
    assert (tr.engine.fused, tr.engine._plan_fused(), tr.engine._plan_flags()) == (3, 3, FLAG) and tr.engine.image_weights is False
    tr = pv.trainers.SVItrainer(m, image_weights=True)                 # a later trainer without the keyword: today's route
    assert tr.engine.fast_weights is False and (tr.engine._plan_fused(), tr.engine._plan_flags()) == (1, 0)
    for kw in (dict(precision="bf16", image_weights=True), dict(precision="bf16", pixel_weights=torch.ones(8, 8))):
        with pytest.raises(ValueError, match="weights"):               # without the keyword: today's refusals, today's messages
            pv.trainers.SVItrainer(model(), **kw)
    for kw in (dict(), dict(precision="bf16"), dict(fused=0, image_weights=True), dict(fused=1, image_weights=True)):
        with pytest.raises(ValueError, match=KW):
            pv.trainers.SVItrainer(model(), fast_weights=True, **kw)
    with pytest.raises(ValueError, match="multiple of 16"):
        pv.trainers.SVItrainer(model(dims=(7, 9), inv=("r", "t")), precision="bf16", image_weights=True, fast_weights=True)
    for bad in (1, "yes", torch.ones(1)):
        with pytest.raises(ValueError, match=KW):
            pv.trainers.SVItrainer(model(), image_weights=True, fast_weights=bad)


def test_keyword_reaches_the_engine_through_the_trainer():
    """A recording stand-in for model.engine: the trainer hands the keyword on (False when it was not given, so that a later
    trainer on the same model is back on today's route)."""
    class Eng:
        device = torch.device("cpu")
        grads_live = False

        def reset_optimizer(self):
            pass

    class Model(torch.nn.Module):
        device, channels = "cpu", 1

        def __init__(self):
            super().__init__()
            self.calls = []

        def engine(self, **kw):
            self.calls.append(kw)
            return Eng()
    m = Model()
    pv.trainers.SVItrainer(m, image_weights=True, fast_weights=True, precision="bf16")
    pv.trainers.SVItrainer(m, image_weights=True)
    assert m.calls[0]["fast_weights"] is True and m.calls[0]["fused"] == 3 and m.calls[0]["image_weights"] is True
    assert m.calls[1]["fast_weights"] is False and m.calls[1]["fused"] == 2


def test_pyro_objects_refuse_the_keyword():
    from pyroved_amd.trainers import svi
    assert re.search(r'bad = \[k for k in \([^)]*"fast_weights"', inspect.getsource(svi.SVItrainer.__init__))
    try:
        import pyro.optim as poptim
    except ImportError:
        with pytest.raises(TypeError):
            pv.trainers.SVItrainer(model(), optimizer=object(), fast_weights=True)
        return
    with pytest.raises(ValueError, match=KW):
        pv.trainers.SVItrainer(model(), optimizer=poptim.Adam({"lr": 1e-3}), fast_weights=True)


# ------------------------------------------------------------------------------- the references
def _params(c):
    m = pv.models.iVAE(c["dims"], 2, c["inv"], seed=1, device="cpu", **mc.model_kwargs(c))
    return state(m)


@functools.lru_cache(maxsize=None)
def _two_steps(name, route):
    """The reference's gradients of two steps, each from float32-rounded parameters (what the GPU step tests do), on a 256-CU
    partition: [{key: grad}, {key: grad}]."""
    c = fw.CASES[name]
    x, y, eps = fw.case_data(c)
    o = fw.oracle(c, _params(c), route, cus=256)
    out = []
    for k in range(2):
        o.step(x, eps[k], 1.0, y)
        out.append(o.last_grads)
        mc.round_to_float32(o)
    return out


def _grads(c, route, w):
    x, y, eps = fw.case_data(c)
    o = fw.oracle(c, _params(c), route, cus=256, w=w)
    o.loss_and_grads(x, eps[0], 1.0, y)
    return {k: v.grad.detach().clone() for k, v in o.p.items()}


def test_case_table():
    assert len(fw.CASES) == 8 and set(fw.BF16_BARS) == set(fw.CASES) and set(fw.ANALYTIC) <= set(fw.CASES)
    for name, c in fw.CASES.items():
        n = 1
        for d in c["dims"]:
            n *= d
        assert c["C"] == 1 and n % 16 == 0 and "hidden_d" not in c and c.get("activation", "tanh") == "tanh", name
        w = fw.weights(c)
        assert tuple(w.shape) == ((c["b"],) if fw.per_image(c) else ()) + tuple(c["dims"]), name
        assert bool((w == 0).any()) and bool((w > 0).any()), name
        if fw.per_image(c):
            assert float(w[2].abs().max()) == 0.0 and float(w[1].abs().max()) > 0.0, name     # image 2 contributes KL terms only
        grad_bar, loss_bar = fw.BF16_BARS[name]
        assert 0 < grad_bar <= 1e-3 and 2.4e-7 <= loss_bar <= 1e-5, name


@pytest.mark.parametrize("name", [fw.CASE1, "f03_6x8_rt_b171_pdisc", "f05_8x8_r_cdim2_b352_poisson_pramp"])
def test_exact_emulation_is_the_plain_weighted_reference(name):
    """The weighted oracles over a Config with Bf16Plan(exact=True) — every rounding off — equal the plain weighted oracles to
    float64 rounding: the composition the plain-bf16 route's reference rests on adds nothing but the roundings."""
    c = fw.CASES[name]
    x, y, eps = fw.case_data(c)
    res = []
    for route, exact in (("x3", False), ("bf16", True)):
        o = fw.oracle(c, _params(c), route, cus=256, exact=exact)
        out = o.loss_and_grads(x, eps[0], 1.0, y)
        res.append((out, {k: v.grad.detach().clone() for k, v in o.p.items()}))
    (a, ga), (b, gb) = res
    for k in ("loss", "ll", "logpz", "logqz"):
        assert abs(a[k].item() - b[k].item()) <= 1e-12 * abs(a[k].item()), k
    for k in ga:
        assert rel_l2(gb[k], ga[k]) < 1e-11, (k, rel_l2(gb[k], ga[k]))


@pytest.mark.parametrize("route", sorted(fw.ROUTES))
@pytest.mark.parametrize("name", sorted(fw.CASES))
def test_gpu_step_cases_keep_near_zero_gradient_entries_below_one_percent(name, route):
    """check_params_after_adam caps near-zero gradient entries at 1 % per tensor and needs every gradient tensor non-zero: a
    condition on the inputs, confirmed here with the references alone over the two steps the GPU tests take."""
    worst = 0.0
    for k, grads in enumerate(_two_steps(name, route)):
        for key, g in grads.items():
            assert float(g.abs().max()) > 0.0, (name, route, k, key)
            share = near_zero_share(g)
            worst = max(worst, share)
            assert share < ILL_SHARE, (name, route, k, key, share)
    print("%s %s: worst share of near-zero gradient entries %.4f" % (name, route, worst))


@pytest.mark.parametrize("route", sorted(fw.ROUTES))
@pytest.mark.parametrize("name", sorted(fw.CASES))
def test_checked_gradients_see_the_weights(name, route):
    """Not blind: with the per-image weights rolled by one image, or the weights replaced by ones, at least one gradient tensor
    the GPU tests check moves by >= 5x its bar."""
    c = fw.CASES[name]
    bar = RTOL_GRAD if route == "x3" else fw.BF16_BARS[name][0]
    g0 = _two_steps(name, route)[0]
    w = fw.weights(c)
    others = [("ones", torch.ones_like(w))]
    if fw.per_image(c):
        others.append(("rolled", torch.roll(w, 1, 0)))
    for tag, wo in others:
        g1 = _grads(c, route, wo)
        moved = max(rel_l2(g1[k], g0[k]) for k in g0)
        print("%s %s %s: the most moved gradient tensor moved %.3e (bar %.1e)" % (name, route, tag, moved, bar))
        assert moved >= 5 * bar, (name, route, tag, moved)
