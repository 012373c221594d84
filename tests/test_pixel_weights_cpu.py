"""
Per-observation weights of the likelihood — pv_ivae_weighted_* in the C ABI, pixel_weights= in Python — where no GPU is needed:
the four symbols and the unchanged ABI, what the workspace query refuses and which kernel family pv_ivae_weighted_uses_fused
reports (host arithmetic), every ValueError of the engine and the trainer with the configure rollback, the reference
(tests/_pixel_weight_cases.WeightedOracle) against orc.elbo, and the condition the GPU step tests' parameter check rests on.
Plans are tests/_plan_kit.py's: 784 positions x ch observations, batch 16.
"""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT

import pyroved_amd as pv
from pyroved_amd import _abi
from oracle import svi_oracle as orc
import _multichannel_cases as mc
import _pixel_weight_cases as pw
from _judge import ILL_SHARE, near_zero_share, state
from _plan_kit import _plan, _vanilla_plan

EINVAL = -1
FLAG = _abi.PV_PLAN_FUSED_CHANNELS
SYMBOLS = ("pv_ivae_weighted_workspace_bytes", "pv_ivae_weighted_uses_fused", "pv_ivae_weighted_loss_and_grads",
           "pv_ivae_weighted_step")


# ------------------------------------------------------------------------------- C ABI
def test_symbols_and_unchanged_abi():
    src = open(os.path.join(ROOT, "include", "pyroved_amd.h")).read()
    lib = _abi.lib()
    for name in SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, src), "%s is not declared in the header" % name
        assert name in _abi.SIGNATURES and getattr(lib, name) is not None
    assert re.search(r"pv_ivae_weighted_loss_and_grads\(const pv_ivae_plan\* plan, const float\* pixel_w, int want_grads, void\* stream\)", src)
    assert re.search(r"pv_ivae_weighted_step\(const pv_ivae_plan\* plan, const float\* pixel_w, void\* stream\)", src)
    assert _abi.PV_ABI_VERSION == 17 and lib.pv_version() == 17 and C.sizeof(_abi.pv_ivae_plan) == 2824


def _conv_plan():
    p = _plan(0, 1)                                                 # Conv2d(1 -> 4, k 3) on 28 x 28
    p.n_pix, p.n_enc, p.n_enc_ops, p.enc_ndim = 784, 0, 1, 2
    p.enc_in_dim[0] = p.enc_in_dim[1] = 28
    op = _abi.pv_op()
    op.kind, op.cin, op.cout, op.ksize, op.act, op.w_off, op.b_off = _abi.OP["conv"], 1, 4, 3, _abi.ACT["lrelu"], 0, 36
    p.enc_ops[0] = op
    p.head.in_dim = 4 * 784
    return p


def test_workspace_query_refusals():
    lib = _abi.lib()
    ws = lambda p: lib.pv_ivae_weighted_workspace_bytes(C.byref(p))
    for ch in range(1, 9):
        for fused in (0, 1, 2):
            assert ws(_plan(fused, ch)) > 0, (fused, ch)
        assert ws(_plan(3, ch)) == EINVAL                                   # the bf16 throughput kernels
    assert ws(_vanilla_plan(2)) > 0 and ws(_vanilla_plan(0)) > 0
    assert lib.pv_ivae_workspace_bytes(C.byref(_plan(0, 1, discrete_dim=3))) > 0
    assert ws(_plan(0, 1, discrete_dim=3)) == EINVAL                        # jiVAE
    assert lib.pv_ivae_workspace_bytes(C.byref(_conv_plan())) > 0
    assert ws(_conv_plan()) == EINVAL                                       # conv encoder
    for field in ("ext_encoder", "ext_decoder"):
        p = _plan(0, 1)
        setattr(p, field, 1)
        assert lib.pv_ivae_workspace_bytes(C.byref(p)) > 0 and ws(p) == EINVAL, field
    keep = C.create_string_buffer(64)
    for field in ("row_w", "row_elbo", "dy", "class_onehot"):
        p = _plan(0, 1)
        if field == "dy":
            p.c_dim = 1
            p.fc_latent.in_dim = 3
            p.enc[0].in_dim += 1
        if field != "class_onehot":
            setattr(p, field, C.addressof(keep))
            assert lib.pv_ivae_workspace_bytes(C.byref(p)) > 0
        else:
            p.class_onehot = C.addressof(keep)
        assert ws(p) == EINVAL, field
    assert ws(_plan(0, 9)) == EINVAL and ws(_plan(0, 0)) == EINVAL          # what every query refuses
    # the calls themselves: refused before any pointer is touched; a null pixel_w forwards (and that call refuses the empty plan)
    for p in (_plan(3, 1), _plan(0, 1, discrete_dim=3)):
        assert lib.pv_ivae_weighted_loss_and_grads(C.byref(p), C.addressof(keep), 1, None) == EINVAL
        assert lib.pv_ivae_weighted_step(C.byref(p), C.addressof(keep), None) == EINVAL
    assert lib.pv_ivae_weighted_loss_and_grads(C.byref(_plan(2, 1)), C.addressof(keep), 1, None) == EINVAL     # no buffers
    assert lib.pv_ivae_weighted_loss_and_grads(C.byref(_plan(2, 1)), None, 1, None) == EINVAL
    assert lib.pv_ivae_weighted_step(C.byref(_plan(2, 1)), None, None) == EINVAL


def test_routing():
    """pv_ivae_weighted_uses_fused and the step layout's size: the weighted fused f32 kernel for one channel with fused 1 or 2 and
    for 2 .. 8 channels with the flag and fused == 1; the layered kernels everywhere else."""
    lib = _abi.lib()
    uses = lambda p: lib.pv_ivae_weighted_uses_fused(C.byref(p))
    ws = lambda p: lib.pv_ivae_weighted_workspace_bytes(C.byref(p))
    step = lambda p: lib.pv_ivae_workspace_bytes_for(C.byref(p), 1)

    def flagged(fused, ch):
        p = _plan(fused, ch)
        p.flags |= FLAG
        return p
    assert uses(_plan(0, 1)) == 0 and ws(_plan(0, 1)) == step(_plan(0, 1))
    for fused in (1, 2):                                                    # one channel: the f32 kernel's layout, flag or not
        assert uses(_plan(fused, 1)) == 1 and uses(flagged(fused, 1)) == 1
        assert ws(_plan(fused, 1)) == ws(flagged(fused, 1)) == step(_plan(1, 1))
    assert uses(_plan(3, 1)) == 0
    for ch in range(2, 9):
        for fused in (0, 1, 2):                                             # unflagged: layered
            assert uses(_plan(fused, ch)) == 0 and ws(_plan(fused, ch)) == step(_plan(0, ch))
        assert uses(flagged(1, ch)) == lib.pv_ivae_uses_fused(C.byref(flagged(1, ch))) == 1
        assert ws(flagged(1, ch)) == step(flagged(1, ch)) < step(_plan(0, ch))
        assert uses(flagged(0, ch)) == 0 and uses(flagged(2, ch)) == 0      # as unweighted: the flag works with fused == 1
    p = _plan(2, 1)                                                         # 63 positions (7 x 9): not a multiple of 16
    p.n_pix = p.enc[0].in_dim = 63
    assert uses(p) == 0 and ws(p) > 0
    p = _plan(2, 1)                                                         # a 72 / 40 decoder
    p.fc_coord.out_dim = p.fc_latent.out_dim = p.dec[0].in_dim = 72
    p.dec[0].out_dim = p.dec[1].in_dim = 40
    assert uses(p) == 0 and ws(p) > 0
    p = _plan(2, 1)                                                         # softplus
    p.dec[0].act = p.dec[1].act = _abi.ACT["softplus"]
    assert uses(p) == 0
    assert uses(_vanilla_plan(2)) == 0
    assert uses(_plan(2, 1, discrete_dim=3)) == 0 and uses(_conv_plan()) == 0      # out of scope: 0


# ------------------------------------------------------------------------------- Python: engine and trainer
def model(channels=1, **kw):
    return pv.models.iVAE((8, 8), 2, ["r", "t", "s"], channels=channels, seed=1, device="cpu", **kw)


W = torch.ones(8, 8)


def test_value_errors_name_the_keyword():
    bad = [torch.ones(8, 7), torch.ones(64), torch.ones(8, 8, 2), -torch.ones(8, 8), torch.zeros(8, 8),
           torch.full((8, 8), float("nan")), torch.full((8, 8), float("inf")), torch.zeros(8, 8, dtype=torch.bool)]
    for w in bad:
        m = model()
        with pytest.raises(ValueError, match="pixel_weights"):
            m.engine(pixel_weights=w)
        assert m._engine is None                                       # raised before anything was bound
        with pytest.raises(ValueError, match="pixel_weights"):
            pv.trainers.SVItrainer(model(), pixel_weights=w)
    m = model(3)
    for w in (torch.ones(8, 8, 2), torch.ones(3, 8, 8)):               # channel-first: refused, not reshaped
        with pytest.raises(ValueError, match="pixel_weights"):
            m.engine(pixel_weights=w)
    for kw in (dict(num_particles=3), dict(loss="RenyiELBO"), dict(precision="bf16"), dict(fused=3)):
        with pytest.raises(ValueError, match="pixel_weights"):
            pv.trainers.SVItrainer(model(), pixel_weights=W, **kw)
    for kw in (dict(particles=3), dict(particles=3, renyi=0.0), dict(renyi=0.0), dict(fused=3)):
        m = model()
        with pytest.raises(ValueError, match="pixel_weights"):
            m.engine(pixel_weights=W, **kw)
        assert m._engine is None


def test_other_models_and_networks_are_refused():
    j = pv.models.jiVAE((8, 8), 2, 3, ["r"], seed=1, device="cpu")
    with pytest.raises(ValueError, match="pixel_weights"):
        pv.trainers.SVItrainer(j, pixel_weights=W, enumerate_parallel=True)
    with pytest.raises(ValueError, match="pixel_weights"):
        j.engine(pixel_weights=W)
    v = pv.models.VED((8, 8), (8, 8), seed=1, device="cpu")
    with pytest.raises(ValueError, match="pixel_weights"):
        pv.trainers.SVItrainer(v, pixel_weights=W)
    s = pv.models.ssiVAE((8, 8), 2, 3, ["r"], seed=1, device="cpu")
    with pytest.raises(ValueError, match="pixel_weights"):
        s.engine(pixel_weights=W)
    m = model()
    m.set_encoder(pv.nets.convEncoderNet((8, 8), m.z_dim, 1, hidden_dim=[(4,)]))
    with pytest.raises(ValueError, match="pixel_weights"):
        m.engine(pixel_weights=W)

    class Enc(torch.nn.Module):
        def forward(self, x):
            return x.reshape(x.shape[0], -1)[:, :5], torch.ones(x.shape[0], 5)
    m = model()
    m.set_encoder(Enc())
    with pytest.raises(ValueError, match="pixel_weights"):
        m.engine(pixel_weights=W)


def test_pyro_objects_refuse_the_keyword():
    """The keyword belongs to the HIP path: with a Pyro optimizer object it is a ValueError (a TypeError where pyro-ppl is missing,
    raised before the keyword list is looked at — as for every keyword of that list)."""
    try:
        import pyro.optim as poptim
    except ImportError:
        with pytest.raises(TypeError):
            pv.trainers.SVItrainer(model(), optimizer=object(), pixel_weights=W)
        import inspect
        from pyroved_amd.trainers import svi
        assert re.search(r'bad = \[k for k in \([^)]*"pixel_weights"', inspect.getsource(svi.SVItrainer.__init__))
        return
    with pytest.raises(ValueError, match="pixel_weights"):
        pv.trainers.SVItrainer(model(), optimizer=poptim.Adam({"lr": 1e-3}), pixel_weights=W)


@pytest.fixture
def unbound(monkeypatch):
    """Engines here never reach the device: bind() is stubbed (tests/test_multichannel_fused_cpu.py does the same)."""
    from pyroved_amd.engine import IVAEEngine
    monkeypatch.setattr(IVAEEngine, "bind", lambda self: None)


def test_accepted_forms(unbound):
    disc = pw.disc((8, 8), 1)[..., 0]
    for w in (disc, disc.numpy(), disc.bool(), disc.double(), disc.unsqueeze(-1), disc.to(torch.int64)):
        eng = model().engine(pixel_weights=w)
        t = eng.pixel_weights
        assert t.dtype == torch.float32 and t.is_contiguous() and tuple(t.shape) == (64,)
        assert torch.equal(t, disc.reshape(-1))
    eng = model(3).engine(pixel_weights=disc)                          # data_dim: the same weight in every channel
    assert torch.equal(eng.pixel_weights.reshape(8, 8, 3), disc.unsqueeze(-1).expand(8, 8, 3))
    r = pw.ramp((8, 8), 3)
    eng = model(3).engine(pixel_weights=r)
    assert torch.equal(eng.pixel_weights, r.reshape(-1))


def test_plan_bits_and_dp(unbound):
    for fused in (1, 2):
        eng = model().engine(fused=fused, pixel_weights=W)
        assert eng._plan_fused() == 1 and eng.supports_dp_step is False
        assert model().engine(fused=fused)._plan_fused() == fused and model().engine(fused=fused).supports_dp_step is True
    assert model().engine(fused=0, pixel_weights=W)._plan_fused() == 0
    eng = model(3).engine(pixel_weights=W)                             # several channels: as without weights
    assert (eng._plan_fused(), eng._plan_flags()) == (2, 0)
    eng = model(3).engine(pixel_weights=W, fused_channels=True)
    assert (eng._plan_fused(), eng._plan_flags()) == (1, FLAG)


def test_configure_sets_removes_and_rolls_back(unbound):
    m = model()
    eng = m.engine()
    assert eng.pixel_weights is None and eng._plan_fused() == 2 and eng.supports_dp_step is True
    eng.ws = "stale"
    eng.configure(pixel_weights=W)
    assert eng.pixel_weights is not None and eng.ws is None and eng._plan_fused() == 1 and eng.supports_dp_step is False
    eng.configure(lr=2e-3)                                             # None leaves the setting
    assert eng.pixel_weights is not None
    for kw in (dict(fused=3), dict(particles=2), dict(renyi=0.5)):
        with pytest.raises(ValueError, match="pixel_weights"):
            eng.configure(**kw)
        assert (eng.fused, eng.particles, eng.renyi) == (2, 1, None) and eng.pixel_weights is not None
    keep = eng.pixel_weights
    with pytest.raises(ValueError, match="pixel_weights"):
        eng.configure(pixel_weights=torch.zeros(8, 8))
    assert eng.pixel_weights is keep
    eng.ws = "stale"
    eng.configure(pixel_weights=False)
    assert eng.pixel_weights is None and eng.ws is None and eng._plan_fused() == 2 and eng.supports_dp_step is True
    eng.configure(fused=3)
    with pytest.raises(ValueError, match="pixel_weights"):
        eng.configure(pixel_weights=W)
    assert eng.pixel_weights is None and eng.fused == 3
    assert m.engine(fused=2, pixel_weights=W) is eng and eng.pixel_weights is not None      # model.engine(...) on an existing engine


def test_trainer_keyword(unbound):
    m = model()
    tr = pv.trainers.SVItrainer(m, pixel_weights=pw.disc((8, 8), 1)[..., 0].bool())
    assert tr.engine.pixel_weights is not None and tr.engine._plan_fused() == 1
    tr = pv.trainers.SVItrainer(m)                                     # a later trainer without the keyword: unweighted again
    assert tr.engine.pixel_weights is None and tr.engine._plan_fused() == 2


# ------------------------------------------------------------------------------- the reference
def _case(name):
    c = pw.CASES[name]
    m = pv.models.iVAE(c["dims"], 2, c["inv"], seed=1, device="cpu", **mc.model_kwargs(c))
    return c, m, pw.case_data(c)


@pytest.mark.parametrize("name", ["w01_8x8_rts_c1_b6_disc", "w03_8x8_r_c3_b6_poisson_ramp", "w04_8x8_rts_c2_cdim3_b6_cbern_disc",
                                  "w10_8x8_none_c2_b6_soft"])
@pytest.mark.parametrize("kl", ["sampled", "analytic"])
def test_reference_with_ones_is_the_plain_oracle(name, kl):
    """Weights of ones: orc.elbo's loss, terms and gradients bit for bit.  Weights of 2: the ll slot doubles, the KL slots stay."""
    c, m, (x, y, eps) = _case(name)
    n = int(np.prod(c["dims"])) * c["C"]
    plain = orc.SVIOracle(state(m), pw.case_config(c), dtype=torch.float64, kl=kl)
    ones = pw.WeightedOracle(state(m), pw.case_config(c), torch.ones(n), dtype=torch.float64, kl=kl)
    two = pw.WeightedOracle(state(m), pw.case_config(c), torch.full((n,), 2.0), dtype=torch.float64, kl=kl)
    for o in (plain, ones, two):
        o.step(x, eps[0], 1.0, y)
    for k in ("loss", "ll", "logpz", "logqz"):
        assert torch.equal(ones.last[k], plain.last[k]), k
    assert set(plain.last) <= set(ones.last)
    for k, g in plain.last_grads.items():
        assert torch.equal(ones.last_grads[k], g), k
    torch.testing.assert_close(two.last["ll"], 2.0 * plain.last["ll"], rtol=1e-14, atol=0.0)
    assert torch.equal(two.last["logpz"], plain.last["logpz"]) and torch.equal(two.last["logqz"], plain.last["logqz"])


def test_reference_weights_reach_the_right_values():
    """A weight of zero on one observed value removes exactly that value's log-probability from ll — for (position, channel)
    indexing, channel-last."""
    c, m, (x, y, eps) = _case("w03_8x8_r_c3_b6_poisson_ramp")
    cfg = pw.case_config(c)
    with torch.no_grad():
        full = orc.elbo({k: v.double() for k, v in state(m).items()}, cfg, x.double(), eps[0].double())
        lp = orc.likelihood(cfg, full["loc"].reshape(6, -1)).log_prob(x.double().reshape(6, -1)).reshape(6, 8, 8, 3)
        w = torch.ones(8, 8, 3)
        w[2, 5, 1] = 0.0
        o = pw.WeightedOracle(state(m), cfg, w, dtype=torch.float64)
        out = o.loss_and_grads(x, eps[0])
    torch.testing.assert_close(out["ll"], full["ll"] - lp[:, 2, 5, 1].sum(), rtol=1e-12, atol=1e-12)


# ------------------------------------------------------------------------------- the GPU step cases' condition
def test_gpu_step_cases_keep_near_zero_gradient_entries_below_one_percent():
    """tests/_judge.py's check_params_after_adam holds entries with |g_ref| < 1e-5 max|g_ref| to 2 lr only, on
    the condition that they are fewer than 1 % of a tensor and that no tensor's gradient vanishes: confirmed here with the float64
    reference alone, at every case over its two steps (each from float32-rounded parameters, as there), case 1 also with the
    analytic KL.  Measured worst share: 0.78 % (w01, analytic KL, step 1: one entry of 128); every other case <= 0.39 %."""
    torch.set_num_threads(min(8, torch.get_num_threads()))
    worst = 0.0
    for name, c in sorted(pw.CASES.items()):
        for kl in (("sampled", "analytic") if name == pw.CASE1 else ("sampled",)):
            _, m, (x, y, eps) = _case(name)
            o = pw.WeightedOracle(state(m), pw.case_config(c), pw.weights(c), dtype=torch.float64, kl=kl)
            for k in range(2):
                o.step(x, eps[k], 1.0, y)
                for key, g in o.last_grads.items():
                    assert g.norm().item() > 0.0, "%s %s step %d %s: zero gradient" % (name, kl, k, key)
                    share = near_zero_share(g)
                    worst = max(worst, share)
                    assert share < ILL_SHARE, "%s %s step %d %s: %.2f %% near-zero gradient entries" % (name, kl, k, key, 100 * share)
                mc.round_to_float32(o)
    print("worst near-zero share: %.3f %%" % (100 * worst))
