"""
CPU tests (-m "not gpu") of fused_any_size / PV_PLAN_FUSED_TAIL: a spatial model whose positions are no multiple of 16 on the
fused f32 decoder kernel's tail form (pyroved_amd/csrc/pv_sdec_fused_mc.hip: pv_sdec_fused_mc_tail_kernel).

What runs without a GPU: the library's host-side answers for flagged plans (pv_ivae_uses_fused, pv_ivae_weighted_uses_fused and
the workspace queries), the engine's settings (the plan's `fused` and flag bit, the refusals, a refused configure leaving no
trace) and the trainer's keyword.  The kernel itself: tests/test_gpu_any_size.py.
"""
import ctypes as C

import pytest
import torch

import pyroved_amd as pv
from pyroved_amd import _abi
from _plan_kit import _plan
from _engine_settings_cases import unbound, settings_of, plan_of

TAIL = _abi.PV_PLAN_FUSED_TAIL
CH = _abi.PV_PLAN_FUSED_CHANNELS


def plan(pos, fused, flags=0, channels=1, lik="bernoulli"):
    """tests/_plan_kit's fused-architecture plan with `pos` positions of `channels` observations, batch 16."""
    p = _plan(fused, channels)
    p.n_pix = pos * channels
    p.enc[0].in_dim = pos * channels
    p.flags = flags
    p.lik = {**_abi.LIK, **_abi.LIK_JOINT}[lik]
    if lik in ("poisson_log", "categorical"):
        p.sigmoid_out = 0
    return p


def answers(p):
    lib = _abi.lib()
    r = C.byref(p)
    return (lib.pv_ivae_uses_fused(r), lib.pv_ivae_weighted_uses_fused(r), lib.pv_ivae_workspace_bytes(r),
            lib.pv_ivae_weighted_workspace_bytes(r), tuple(lib.pv_ivae_workspace_bytes_for(r, w) for w in (1, 2, 3)))


# ------------------------------------------------------------------------------- the library's host side
def test_abi_is_unchanged():
    assert _abi.lib().pv_version() == _abi.PV_ABI_VERSION == 17 and TAIL == 1024


def test_flagged_63_position_plan_runs_fused():
    """7 x 9 = 63 positions, fused = 1: layered without the bit (the routing the older tests pin), fused with it — and the fused
    layout, four rows of 16 per sample, is another size than the layered one."""
    off, on = answers(plan(63, 1)), answers(plan(63, 1, TAIL))
    assert off[0] == 0 and off[1] == 0
    assert on[0] == 1, "pv_ivae_uses_fused"
    assert on[1] == 1, "pv_ivae_weighted_uses_fused"
    assert on[2] > 0 and on[3] > 0 and all(v > 0 for v in on[4])
    # (at this size the fused layout — one record of 34 560 floats per workgroup, 64 workgroups — outweighs the layered one's
    #  per-row activations)
    assert on[4][0] > off[4][0] and on[3] > off[3] and on[2] > off[2], "the training step's workspace: the fused layout"
    # the same plan padded by hand to 64 positions has the same decoder layout; what differs is the encoder's 63-wide input
    full = answers(plan(64, 1))
    assert full[0] == 1 and abs(on[4][0] - full[4][0]) <= 64 * 1024


def test_flagged_workspace_is_larger_than_the_unpadded_fused_layout_would_be():
    """The padded rows take room: 17 positions occupy 32 rows per sample, so the step's workspace of the flagged plan is larger
    than that of the 16-position plan on the same kernel family by at least the per-row buffers of 16 more rows per sample
    (llrow + 4 rowtp: 5 floats per row, batch 16)."""
    a, b = answers(plan(17, 1, TAIL)), answers(plan(16, 1))
    assert a[0] == b[0] == 1
    assert a[4][0] - b[4][0] >= 16 * 16 * 5 * 4


@pytest.mark.parametrize("fused", [0, 2, 3])
def test_the_bit_is_fused_1_only(fused):
    assert answers(plan(63, fused, TAIL)) == answers(plan(63, fused))


@pytest.mark.parametrize("fused", [0, 1, 2, 3])
def test_a_multiple_of_16_answers_identically(fused):
    assert answers(plan(64, fused, TAIL)) == answers(plan(64, fused))
    assert answers(plan(784, fused, TAIL)) == answers(plan(784, fused))


def test_channels_need_both_bits_and_seven_stay_layered():
    for ch in (2, 3, 8):
        assert answers(plan(63, 1, TAIL, ch)) == answers(plan(63, 1, 0, ch)), "C > 1 without PV_PLAN_FUSED_CHANNELS"
        assert answers(plan(63, 1, CH, ch))[0] == 0
        on = answers(plan(63, 1, TAIL | CH, ch))
        assert on[0] == 1 and on[1] == 1, ch
    # seven channels: the tail instance spills and is not built (profiles/any_size_resource_usage.txt)
    assert answers(plan(63, 1, TAIL | CH, 7)) == answers(plan(63, 1, CH, 7))
    assert answers(plan(64, 1, TAIL | CH, 7))[0] == 1


def test_what_keeps_todays_routing():
    # the categorical likelihood
    assert answers(plan(63, 1, TAIL | CH, 3, "categorical")) == answers(plan(63, 1, CH, 3, "categorical"))
    # a discrete latent (jiVAE)
    a, b = _plan(1, 1, discrete_dim=3), _plan(1, 1, discrete_dim=3)
    for p in (a, b):
        p.n_pix = p.enc[0].in_dim = 63
    a.flags = TAIL
    assert answers(a) == answers(b)
    # other decoders: 72 / 40, softplus
    a, b = plan(63, 1, TAIL), plan(63, 1)
    for p in (a, b):
        p.fc_coord.out_dim = p.fc_latent.out_dim = p.dec[0].in_dim = 72
        p.dec[0].out_dim = p.dec[1].in_dim = 40
    assert answers(a) == answers(b)
    a, b = plan(63, 1, TAIL), plan(63, 1)
    for p in (a, b):
        p.dec[0].act = p.dec[1].act = _abi.ACT["softplus"]
    assert answers(a) == answers(b)
    # the other per-value likelihoods do take it
    for lik in ("gaussian", "continuous_bernoulli", "poisson_log"):
        assert answers(plan(63, 1, TAIL, 1, lik))[:2] == (1, 1), lik


# ------------------------------------------------------------------------------- the engine's settings
def ivae(dims, **kw):
    return pv.models.iVAE(dims, 2, ["r", "t"] if len(dims) == 2 else ["t"], seed=1, device="cpu", **kw)


def engine(model, **kw):
    model._engine = None
    with unbound():
        return model.engine(**kw)


@pytest.mark.parametrize("fused", [1, 2])
def test_engine_sets_fused_1_and_the_bit(fused):
    eng = engine(ivae((7, 9)), fused=fused, fused_any_size=True)
    assert eng._plan_fused() == 1 and eng._plan_flags() & TAIL and eng.supports_dp_step is False
    eng = engine(ivae((8, 8)), fused=fused, fused_any_size=True)
    assert eng._plan_fused() == fused and not eng._plan_flags() & TAIL and eng.supports_dp_step is True
    eng = engine(ivae((7, 9)), fused=fused)
    assert eng._plan_fused() == fused and not eng._plan_flags() & TAIL and eng.fused_any_size is False


def test_engine_keeps_todays_routing_elsewhere():
    for model, kw in ((ivae((7, 9), hidden_dim_d=[72, 40]), {}),
                      (ivae((7, 9), activation="softplus"), {}),
                      (ivae((7, 9), channels=3), {}),                                    # several channels without fused_channels
                      (ivae((7, 9), channels=7), dict(fused_channels=True)),
                      (ivae((7, 9), channels=3, sampler_d="categorical", sigmoid_d=False), dict(fused_channels=True)),
                      (pv.models.iVAE((7, 9), 2, None, seed=1, device="cpu"), {}),        # vanilla decoder
                      (pv.models.jiVAE((7, 9), 2, 3, ["r"], seed=1, device="cpu"), {})):
        plain, flagged = engine(model, **kw), None
        want = plan_of(plain)
        flagged = engine(model, fused_any_size=True, **kw)
        assert plan_of(flagged) == want, type(model).__name__
    eng = engine(ivae((7, 9), channels=3), fused_channels=True, fused_any_size=True)
    assert eng._plan_fused() == 1 and eng._plan_flags() & TAIL and eng._plan_flags() & CH
    for kw in (dict(pixel_weights=torch.ones(7, 9)), dict(image_weights=True), dict(kl="analytic")):
        eng = engine(ivae((7, 9)), fused_any_size=True, **kw)
        assert eng._plan_fused() == 1 and eng._plan_flags() & TAIL, kw


@pytest.mark.parametrize("kw", [dict(fused=0), dict(fused=3), dict(particles=2), dict(renyi=0.0, particles=2), dict(renyi=0.5)])
def test_refusals(kw):
    with pytest.raises(ValueError, match="fused_any_size"):
        engine(ivae((7, 9)), fused_any_size=True, **kw)


def test_not_for_other_engines():
    ss = pv.models.ssiVAE((7, 9), 2, 3, ["r"], seed=1, device="cpu")
    ss._engine = None
    with unbound():
        with pytest.raises(ValueError, match="fused_any_size"):
            ss.engine(fused_any_size=True)


@pytest.mark.parametrize("change", [dict(fused=0), dict(fused=3), dict(particles=3), dict(renyi=0.0)])
def test_a_refused_configure_leaves_the_engine_as_it_was(change):
    eng = engine(ivae((7, 9)), fused_any_size=True)
    sentinel = eng.ws = object()
    before = (settings_of(eng), eng.fused_any_size, plan_of(eng))
    with unbound():
        with pytest.raises(ValueError, match="fused_any_size"):
            eng.configure(**change)
    assert (settings_of(eng), eng.fused_any_size, plan_of(eng)) == before and eng.ws is sentinel


def test_configure_switches_it_and_drops_the_workspace():
    eng = engine(ivae((7, 9)))
    eng.ws = object()
    with unbound():
        eng.configure(fused_any_size=True)
    assert eng.ws is None and eng._plan_fused() == 1 and eng._plan_flags() & TAIL
    eng.ws = sentinel = object()
    with unbound():
        eng.configure(fused_any_size=True, lr=2e-3)                # no change of the setting: the workspace stays
    assert eng.ws is sentinel
    with unbound():
        eng.configure(fused_any_size=False)
    assert eng.ws is None and eng._plan_fused() == 2 and not eng._plan_flags() & TAIL


def test_trainer_keyword():
    with unbound():
        for kw in (dict(precision="bf16"), dict(fused=3), dict(fused=0), dict(num_particles=2), dict(loss="RenyiELBO")):
            m = ivae((7, 9))
            with pytest.raises(ValueError, match="fused_any_size"):
                pv.trainers.SVItrainer(m, fused_any_size=True, **kw)
        with pytest.raises(ValueError, match="fused_any_size"):
            pv.trainers.SVItrainer(ivae((7, 9)), fused_any_size=1)
        tr = pv.trainers.SVItrainer(ivae((7, 9)), fused_any_size=True)
        assert tr.engine._plan_fused() == 1 and tr.engine._plan_flags() & TAIL
        tr = pv.trainers.SVItrainer(ivae((7, 9)))
        assert tr.engine._plan_fused() == 2 and not tr.engine._plan_flags() & TAIL


def test_a_later_trainer_without_the_keyword_is_back_on_the_default_route():
    """The trainer passes the setting every time, like fused_channels: an engine that an earlier trainer switched to the tail
    form does not keep it when the next trainer of the same model does not ask for it."""
    with unbound():
        m = ivae((7, 9))
        m._engine = None
        tr = pv.trainers.SVItrainer(m, fused_any_size=True)
        assert tr.engine._plan_fused() == 1 and tr.engine._plan_flags() & TAIL
        tr.engine.ws = object()
        tr2 = pv.trainers.SVItrainer(m)
        assert tr2.engine is tr.engine and tr2.engine.fused_any_size is False and tr2.engine.ws is None
        assert tr2.engine._plan_fused() == 2 and not tr2.engine._plan_flags() & TAIL
