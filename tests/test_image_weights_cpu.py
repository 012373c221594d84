"""
Per-image observation weights of the likelihood — pv_ivae_weighted_images_* in the C ABI, image_weights= in Python — where no GPU
is needed: the two symbols and the unchanged ABI, what the calls refuse, every ValueError of the engine and the trainer with the
configure rollback, the accepted forms, utils.weights_from_nan, the trainer handing every batch its own rows (a recording
stand-in engine: shuffled loader, device feed on and off, the shard bounds of two ranks), the reference
(tests/_image_weight_cases.ImageWeightedOracle) against WeightedOracle, and the condition the GPU step tests' parameter check
rests on.  Plans are tests/_plan_kit.py's: 784 positions x ch observations, batch 16.
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
from pyroved_amd import dist as pvdist
from oracle import svi_oracle as orc
import _multichannel_cases as mc
import _pixel_weight_cases as pw
import _image_weight_cases as iwc
from _judge import ILL_SHARE, near_zero_share, state
from _plan_kit import _plan, _vanilla_plan

EINVAL = -1
SYMBOLS = ("pv_ivae_weighted_images_loss_and_grads", "pv_ivae_weighted_images_step")
KW = "image_weights"


# ------------------------------------------------------------------------------- C ABI
def test_symbols_and_unchanged_abi():
    src = open(os.path.join(ROOT, "include", "pyroved_amd.h")).read()
    lib = _abi.lib()
    for name in SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, src), "%s is not declared in the header" % name
        assert name in _abi.SIGNATURES and getattr(lib, name) is not None
    assert re.search(r"int pv_ivae_weighted_images_loss_and_grads\(const pv_ivae_plan\* plan, const float\* image_w, int want_grads, "
                     r"void\* stream\);", src)
    assert re.search(r"int pv_ivae_weighted_images_step\(const pv_ivae_plan\* plan, const float\* image_w, void\* stream\);", src)
    # the shared-weight declarations, character for character
    for decl in ("int64_t pv_ivae_weighted_workspace_bytes(const pv_ivae_plan* plan);",
                 "int pv_ivae_weighted_uses_fused(const pv_ivae_plan* plan);",
                 "int pv_ivae_weighted_loss_and_grads(const pv_ivae_plan* plan, const float* pixel_w, int want_grads, void* stream);",
                 "int pv_ivae_weighted_step(const pv_ivae_plan* plan, const float* pixel_w, void* stream);"):
        assert decl in src, decl
    assert _abi.PV_ABI_VERSION == 17 and lib.pv_version() == 17 and C.sizeof(_abi.pv_ivae_plan) == 2824
    assert _abi.SIGNATURES["pv_ivae_weighted_images_step"] == _abi.SIGNATURES["pv_ivae_weighted_step"]
    assert _abi.SIGNATURES["pv_ivae_weighted_images_loss_and_grads"] == _abi.SIGNATURES["pv_ivae_weighted_loss_and_grads"]


def _conv_plan():
    p = _plan(0, 1)                                                 # Conv2d(1 -> 4, k 3) on 28 x 28
    p.n_pix, p.n_enc, p.n_enc_ops, p.enc_ndim = 784, 0, 1, 2
    p.enc_in_dim[0] = p.enc_in_dim[1] = 28
    op = _abi.pv_op()
    op.kind, op.cin, op.cout, op.ksize, op.act, op.w_off, op.b_off = _abi.OP["conv"], 1, 4, 3, _abi.ACT["lrelu"], 0, 36
    p.enc_ops[0] = op
    p.head.in_dim = 4 * 784
    return p


def _refused_plans():
    """(tag, plan) for everything pv_ivae_weighted_* refuses (tests/test_pixel_weights_cpu.py's matrix)."""
    keep = C.create_string_buffer(64)
    out = [("bf16 c%d" % ch, _plan(3, ch)) for ch in range(1, 9)]
    out += [("jiVAE", _plan(0, 1, discrete_dim=3)), ("conv", _conv_plan())]
    for field in ("ext_encoder", "ext_decoder"):
        p = _plan(0, 1)
        setattr(p, field, 1)
        out.append((field, p))
    for field in ("row_w", "row_elbo", "dy", "class_onehot"):
        p = _plan(0, 1)
        if field == "dy":
            p.c_dim = 1
            p.fc_latent.in_dim = 3
            p.enc[0].in_dim += 1
        setattr(p, field, C.addressof(keep))
        out.append((field, p))
    out += [("9 channels", _plan(0, 9)), ("0 channels", _plan(0, 0))]
    return out, keep


def test_calls_refuse_what_the_shared_weight_calls_refuse():
    """PV_EINVAL exactly where pv_ivae_weighted_* returns it, before any pointer is touched; a null image_w forwards to the
    unweighted call (which refuses the empty plan); pv_ivae_weighted_workspace_bytes answers for these calls."""
    lib = _abi.lib()
    plans, keep = _refused_plans()
    w = C.addressof(keep)
    for tag, p in plans:
        assert lib.pv_ivae_weighted_workspace_bytes(C.byref(p)) == EINVAL, tag
        assert lib.pv_ivae_weighted_images_loss_and_grads(C.byref(p), w, 1, None) == EINVAL, tag
        assert lib.pv_ivae_weighted_images_step(C.byref(p), w, None) == EINVAL, tag
        assert lib.pv_ivae_weighted_loss_and_grads(C.byref(p), w, 1, None) == EINVAL, tag
    for ch in range(1, 9):
        for fused in (0, 1, 2):                                             # in scope: the query answers, the call wants buffers
            p = _plan(fused, ch)
            assert lib.pv_ivae_weighted_workspace_bytes(C.byref(p)) > 0
            assert lib.pv_ivae_weighted_images_loss_and_grads(C.byref(p), w, 1, None) == EINVAL
    assert lib.pv_ivae_weighted_workspace_bytes(C.byref(_vanilla_plan(2))) > 0
    assert lib.pv_ivae_weighted_images_loss_and_grads(C.byref(_plan(2, 1)), None, 1, None) == EINVAL
    assert lib.pv_ivae_weighted_images_step(C.byref(_plan(2, 1)), None, None) == EINVAL


# ------------------------------------------------------------------------------- Python: engine and trainer
def model(channels=1, **kw):
    return pv.models.iVAE((8, 8), 2, ["r", "t", "s"], channels=channels, seed=1, device="cpu", **kw)


@pytest.fixture
def unbound(monkeypatch):
    """Engines here never reach the device: bind() is stubbed (tests/test_pixel_weights_cpu.py does the same)."""
    from pyroved_amd.engine import IVAEEngine
    monkeypatch.setattr(IVAEEngine, "bind", lambda self: None)


def test_refused_objectives_precisions_and_switch_values():
    for kw in (dict(num_particles=3), dict(loss="RenyiELBO"), dict(precision="bf16"), dict(fused=3)):
        with pytest.raises(ValueError, match=KW):
            pv.trainers.SVItrainer(model(), image_weights=True, **kw)
    for kw in (dict(particles=3), dict(particles=3, renyi=0.0), dict(renyi=0.0), dict(fused=3)):
        m = model()
        with pytest.raises(ValueError, match=KW):
            m.engine(image_weights=True, **kw)
        assert m._engine is None                                       # raised before anything was bound
    for bad in (torch.ones(6, 8, 8), np.ones((6, 8, 8)), 1, "yes"):    # the switch is a bool: the weights come with every call
        m = model()
        with pytest.raises(ValueError, match=KW):
            m.engine(image_weights=bad)
        assert m._engine is None
        with pytest.raises(ValueError, match=KW):
            pv.trainers.SVItrainer(model(), image_weights=bad)


def test_other_models_and_networks_are_refused():
    j = pv.models.jiVAE((8, 8), 2, 3, ["r"], seed=1, device="cpu")
    with pytest.raises(ValueError, match=KW):
        pv.trainers.SVItrainer(j, image_weights=True, enumerate_parallel=True)
    with pytest.raises(ValueError, match=KW):
        j.engine(image_weights=True)
    v = pv.models.VED((8, 8), (8, 8), seed=1, device="cpu")
    with pytest.raises(ValueError, match=KW):
        pv.trainers.SVItrainer(v, image_weights=True)
    s = pv.models.ssiVAE((8, 8), 2, 3, ["r"], seed=1, device="cpu")
    with pytest.raises(ValueError, match=KW):
        s.engine(image_weights=True)
    m = model()
    m.set_encoder(pv.nets.convEncoderNet((8, 8), m.z_dim, 1, hidden_dim=[(4,)]))
    with pytest.raises(ValueError, match=KW):
        m.engine(image_weights=True)

    class Enc(torch.nn.Module):
        def forward(self, x):
            return x.reshape(x.shape[0], -1)[:, :5], torch.ones(x.shape[0], 5)
    m = model()
    m.set_encoder(Enc())
    with pytest.raises(ValueError, match=KW):
        m.engine(image_weights=True)


def test_pyro_objects_refuse_the_keyword():
    """The keyword belongs to the HIP path: with a Pyro optimizer object it is a ValueError (a TypeError where pyro-ppl is missing,
    raised before the keyword list is looked at — as for every keyword of that list)."""
    try:
        import pyro.optim as poptim
    except ImportError:
        with pytest.raises(TypeError):
            pv.trainers.SVItrainer(model(), optimizer=object(), image_weights=True)
        import inspect
        from pyroved_amd.trainers import svi
        assert re.search(r'bad = \[k for k in \([^)]*"image_weights"', inspect.getsource(svi.SVItrainer.__init__))
        return
    with pytest.raises(ValueError, match=KW):
        pv.trainers.SVItrainer(model(), optimizer=poptim.Adam({"lr": 1e-3}), image_weights=True)


def test_calls_need_the_weights_exactly_when_configured(unbound):
    x, eps = torch.rand(6, 8, 8), torch.randn(6, 5)
    eng = model().engine(image_weights=True)
    with pytest.raises(ValueError, match=KW):
        eng.loss_and_grads(x, eps)                                     # missing
    eng = model().engine()
    with pytest.raises(ValueError, match=KW):
        eng.loss_and_grads(x, eps, image_weights=torch.ones(6, 8, 8))  # unexpected
    eng = model().engine(image_weights=True)
    w = torch.ones(6, 8, 8)
    for extra in (dict(row_w=torch.ones(6)), dict(row_elbo=torch.ones(6)), dict(dy=torch.ones(6, 1)),
                  dict(class_onehot=torch.ones(6, 3)), dict(comm=object(), step=True)):
        with pytest.raises(ValueError, match=KW):
            eng.loss_and_grads(x, eps, image_weights=w, **extra)


def test_wrong_shapes_and_dtypes_name_the_keyword(unbound):
    x, eps = torch.rand(6, 8, 8), torch.randn(6, 5)
    eng = model().engine(image_weights=True)
    for w in (torch.ones(8, 8), torch.ones(5, 8, 8), torch.ones(6, 8, 7), torch.ones(6, 63), torch.ones(6, 8, 8, 2),
              torch.ones(6, 8, 8, dtype=torch.complex64), "mask"):
        with pytest.raises(ValueError, match=KW):
            eng.loss_and_grads(x, eps, image_weights=w)
    eng = model(3).engine(image_weights=True)
    x3 = torch.rand(6, 8, 8, 3)
    for w in (torch.ones(6, 3, 8, 8), torch.ones(6, 8, 8, 2), torch.ones(6, 64)):       # channel-first: refused, not reshaped
        with pytest.raises(ValueError, match=KW):
            eng.loss_and_grads(x3, eps, image_weights=w)


def test_accepted_forms(unbound):
    c = iwc.CASES[iwc.CASE1]
    disc = iwc.weights(c)[..., 0]                                      # (6, 8, 8)
    eng = model().engine(image_weights=True)
    for w in (disc, disc.numpy(), disc.bool(), disc.double(), disc.unsqueeze(-1), disc.to(torch.int64), disc.reshape(6, 64)):
        t = eng._image_weight_tensor(w, 6, 64)
        assert t.dtype == torch.float32 and t.is_contiguous() and tuple(t.shape) == (6, 64)
        assert torch.equal(t, disc.reshape(6, 64))
    eng = model(3).engine(image_weights=True)
    t = eng._image_weight_tensor(disc, 6, 192)                         # (b, *dims): the same weight in every channel
    assert t.is_contiguous() and torch.equal(t.reshape(6, 8, 8, 3), disc.unsqueeze(-1).expand(6, 8, 8, 3))
    r = iwc.pramp(6, (8, 8), 3)
    assert torch.equal(eng._image_weight_tensor(r, 6, 192), r.reshape(6, 192))
    assert torch.equal(eng._image_weight_tensor(r.reshape(6, 192).numpy(), 6, 192), r.reshape(6, 192))


def test_plan_bits_and_dp(unbound):
    for fused in (1, 2):
        eng = model().engine(fused=fused, image_weights=True)
        assert eng._plan_fused() == 1 and eng.supports_dp_step is False
        assert model().engine(fused=fused)._plan_fused() == fused and model().engine(fused=fused).supports_dp_step is True
    assert model().engine(fused=0, image_weights=True)._plan_fused() == 0
    eng = model(3).engine(image_weights=True)                          # several channels: as without weights
    assert (eng._plan_fused(), eng._plan_flags()) == (2, 0)
    eng = model(3).engine(image_weights=True, fused_channels=True)
    assert (eng._plan_fused(), eng._plan_flags()) == (1, _abi.PV_PLAN_FUSED_CHANNELS)


def test_configure_sets_removes_and_rolls_back(unbound):
    m = model()
    eng = m.engine()
    assert eng.image_weights is False and eng._plan_fused() == 2 and eng.supports_dp_step is True
    eng.ws = "kept"
    eng.configure(image_weights=False)                                 # off on an engine without it: nothing is reset
    assert eng.ws == "kept"
    eng.configure(image_weights=True)
    assert eng.image_weights is True and eng.ws is None and eng._plan_fused() == 1 and eng.supports_dp_step is False
    eng.configure(lr=2e-3)                                             # None leaves the setting
    assert eng.image_weights is True
    for kw in (dict(fused=3), dict(particles=2), dict(renyi=0.5)):
        with pytest.raises(ValueError, match=KW):
            eng.configure(**kw)
        assert (eng.fused, eng.particles, eng.renyi) == (2, 1, None) and eng.image_weights is True
    with pytest.raises(ValueError, match=KW):
        eng.configure(image_weights=torch.ones(6, 8, 8))
    assert eng.image_weights is True
    eng.ws = "stale"
    eng.configure(image_weights=False)
    assert eng.image_weights is False and eng.ws is None and eng._plan_fused() == 2 and eng.supports_dp_step is True
    eng.configure(fused=3)
    with pytest.raises(ValueError, match=KW):
        eng.configure(image_weights=True)
    assert eng.image_weights is False and eng.fused == 3
    assert m.engine(fused=2, image_weights=True) is eng and eng.image_weights is True      # model.engine(...) on an existing engine
    eng.configure(pixel_weights=torch.ones(8, 8))                      # the two keywords live side by side
    assert eng.pixel_weights is not None and eng.image_weights is True
    eng.configure(image_weights=False)
    assert eng.pixel_weights is not None and eng._plan_fused() == 1


def test_trainer_keyword(unbound):
    m = model()
    tr = pv.trainers.SVItrainer(m, image_weights=True)
    assert tr.image_weights is True and tr.engine.image_weights is True and tr.engine._plan_fused() == 1
    tr = pv.trainers.SVItrainer(m)                                     # a later trainer without the keyword: unweighted again
    assert tr.image_weights is False and tr.engine.image_weights is False and tr.engine._plan_fused() == 2


# ------------------------------------------------------------------------------- utils.weights_from_nan
def test_weights_from_nan():
    x = torch.rand(4, 8, 8)
    x[0, 1, 2] = x[3, 7, 7] = float("nan")
    x[2] = float("nan")
    keep = x.clone()
    xf, w = pv.utils.weights_from_nan(x)
    assert torch.equal(torch.isnan(x), torch.isnan(keep))              # the input is left alone
    assert xf.shape == x.shape and w.shape == x.shape and w.dtype == x.dtype
    assert torch.isfinite(xf).all() and torch.equal(w, (~torch.isnan(keep)).float())
    assert torch.equal(xf[w == 1], keep[w == 1]) and (xf[w == 0] == 0.0).all() and w[2].sum() == 0
    xf5, w5 = pv.utils.weights_from_nan(x, fill=0.5)
    assert (xf5[w5 == 0] == 0.5).all() and torch.equal(w5, w)
    xn, wn = pv.utils.weights_from_nan(keep.numpy())                   # an ndarray in, tensors out
    assert torch.equal(xn, xf) and torch.equal(wn, w)
    xi, wi = pv.utils.weights_from_nan(torch.arange(6).reshape(2, 3))  # nothing missing
    assert xi.is_floating_point() and (wi == 1).all()
    for bad in (float("nan"), float("inf")):
        with pytest.raises(ValueError, match="fill"):
            pv.utils.weights_from_nan(x, fill=bad)
    assert "weights_from_nan" in pv.trainers.SVItrainer.__doc__ and "weights_from_nan" in pv.utils.__all__


# ------------------------------------------------------------------------------- the trainer hands every batch its own rows
class Recorder:
    """What SVItrainer needs from an engine (the engine= hook), recording every loss_and_grads call's x, y and image_weights."""
    device = torch.device("cpu")
    grads_live = False
    supports_scalars_out = True

    def __init__(self):
        self.lr = self.betas = self.adam_eps = None
        self.calls = []
        self.grad, self.scalars = torch.zeros(8), torch.zeros(4)

    def reset_optimizer(self):
        pass

    def adam_step(self):
        pass

    def loss_and_grads(self, x, eps, beta=1.0, y=None, want_grads=True, scalars_out=None, image_weights=None, **kw):
        assert not kw, kw
        self.calls.append((x.clone(), None if y is None else y.clone(), None if image_weights is None else image_weights.clone(),
                           eps.shape[0], want_grads))
        if scalars_out is not None:
            scalars_out.zero_()


def _tagged(n, c_dim=0):
    """Image i is filled with i, its weights with i + 0.25, its y with i + 0.5: a row that travelled with another image shows."""
    idx = torch.arange(n, dtype=torch.float32)
    x = idx.reshape(n, 1, 1).expand(n, 8, 8).contiguous()
    y = (idx + 0.5).reshape(n, 1).expand(n, c_dim).contiguous() if c_dim else None
    return x, y, x + 0.25


def _check_rows(calls, c_dim):
    seen = []
    for x, y, w, n_eps, _ in calls:
        assert w is not None and w.shape[0] == x.shape[0] == n_eps and tuple(w.shape[1:]) == (8, 8)
        assert torch.equal(w.reshape(len(w), -1), x.reshape(len(x), -1) + 0.25)
        if c_dim:
            assert torch.equal(y, (x[:, 0, 0] + 0.5).reshape(-1, 1).expand(-1, c_dim))
        else:
            assert y is None
        seen += x[:, 0, 0].tolist()
    return seen


@pytest.mark.parametrize("device_feed", [True, False])
@pytest.mark.parametrize("c_dim", [0, 3])
def test_trainer_passes_each_batch_its_own_rows(device_feed, c_dim):
    n = 20
    m = pv.models.iVAE((8, 8), 2, ["r"], c_dim=c_dim, seed=1, device="cpu")
    x, y, w = _tagged(n, c_dim)
    loader = pv.utils.init_dataloader(*([x, y, w] if c_dim else [x, w]), batch_size=6, shuffle=True)
    eng = Recorder()
    tr = pv.trainers.SVItrainer(m, seed=1, engine=eng, device="cpu", image_weights=True, device_feed=device_feed)
    st = torch.get_rng_state()
    tr.step(loader, loader)
    assert (tr._feed_cache is not None) == device_feed
    assert [c[0].shape[0] for c in eng.calls] == [6, 6, 6, 2] * 2 and [c[4] for c in eng.calls] == [True] * 4 + [False] * 4
    seen = _check_rows(eng.calls, c_dim)
    assert sorted(seen[:n]) == sorted(seen[n:]) == list(range(n)) and seen[:n] != list(range(n))       # shuffled, every image once
    torch.set_rng_state(st)                                            # the order is the loader's own
    want = [b[0][:, 0, 0].tolist() for b in loader]
    assert seen[:n] == [v for b in want for v in b]


@pytest.mark.parametrize("device_feed", [True, False])
def test_trainer_shards_the_weights_with_the_images(monkeypatch, device_feed):
    """World size 2 through the stand-in: every rank's calls hold rows [lo, hi) of each global minibatch — images and weights
    alike — and the two ranks together hold the single-process batches."""
    n = 20
    x, _, w = _tagged(n)

    def run(rank, world):
        monkeypatch.setattr(pvdist, "world", lambda group=None: (rank, world))
        monkeypatch.setattr(pvdist, "sync_replicas", lambda *a, **k: None)
        monkeypatch.setattr(pvdist, "allreduce_sum_", lambda t, group=None: t)
        eng = Recorder()
        tr = pv.trainers.SVItrainer(pv.models.iVAE((8, 8), 2, ["r"], seed=1, device="cpu"), seed=1, engine=eng, device="cpu",
                                    image_weights=True, device_feed=device_feed)
        tr.step(pv.utils.init_dataloader(x, w, batch_size=6, shuffle=True))
        _check_rows(eng.calls, 0)
        return [c[0][:, 0, 0].tolist() for c in eng.calls]
    whole = run(0, 1)
    r0, r1 = run(0, 2), run(1, 2)
    assert [len(b) for b in whole] == [6, 6, 6, 2]
    for b, a0, a1 in zip(whole, r0, r1):
        lo, hi = pvdist.shard_bounds(len(b), 0, 2)
        assert a0 == b[lo:hi] and a1 == b[hi:] and len(a0) > 0 and len(a1) > 0


def test_trainer_batch_arity_and_values():
    m = pv.models.iVAE((8, 8), 2, ["r"], seed=1, device="cpu")
    x, _, w = _tagged(12)
    for device_feed in (True, False):
        for tensors in ([x], [x, w, w]):                               # (x) and (x, y, w) for a model without c_dim
            tr = pv.trainers.SVItrainer(m, seed=1, engine=Recorder(), device="cpu", image_weights=True, device_feed=device_feed)
            with pytest.raises(ValueError, match=KW):
                tr.step(pv.utils.init_dataloader(*tensors, batch_size=6))
        mc3 = pv.models.iVAE((8, 8), 2, ["r"], c_dim=3, seed=1, device="cpu")
        tr = pv.trainers.SVItrainer(mc3, seed=1, engine=Recorder(), device="cpu", image_weights=True, device_feed=device_feed)
        with pytest.raises(ValueError, match=KW):
            tr.step(pv.utils.init_dataloader(x, w, batch_size=6))      # c_dim > 0 wants (x, y, w)
        for bad in (-1.0, float("nan"), float("inf")):
            wb = w.clone()
            wb[7, 3, 3] = bad
            eng = Recorder()
            tr = pv.trainers.SVItrainer(m, seed=1, engine=eng, device="cpu", image_weights=True, device_feed=device_feed)
            with pytest.raises(ValueError, match=KW):
                tr.step(pv.utils.init_dataloader(x, wb, batch_size=6, shuffle=False))
            assert len(eng.calls) == (0 if device_feed else 1)         # the data set once, or the batch that holds the value


# ------------------------------------------------------------------------------- the reference
def _case(name, table=None):
    c = (table or iwc.CASES)[name]
    m = pv.models.iVAE(c["dims"], 2, c["inv"], seed=1, device="cpu", **mc.model_kwargs(c))
    return c, m, pw.case_data(c)


@pytest.mark.parametrize("name", ["w01_8x8_rts_c1_b6_disc", "w03_8x8_r_c3_b6_poisson_ramp", "w04_8x8_rts_c2_cdim3_b6_cbern_disc",
                                  "w10_8x8_none_c2_b6_soft"])
@pytest.mark.parametrize("kl", ["sampled", "analytic"])
def test_reference_with_repeated_shared_weights_is_the_shared_reference(name, kl):
    """The shared weights repeated B times: WeightedOracle's loss, terms and gradients bit for bit."""
    c, m, (x, y, eps) = _case(name, pw.CASES)
    shared = pw.WeightedOracle(state(m), pw.case_config(c), pw.weights(c), dtype=torch.float64, kl=kl)
    per = iwc.ImageWeightedOracle(state(m), pw.case_config(c), iwc.shared_as_images(c), dtype=torch.float64, kl=kl)
    for o in (shared, per):
        o.step(x, eps[0], 1.0, y)
    for k in ("loss", "ll", "logpz", "logqz"):
        assert torch.equal(per.last[k], shared.last[k]), k
    for k, g in shared.last_grads.items():
        assert torch.equal(per.last_grads[k], g), k


def test_reference_weights_reach_the_right_values():
    """A weight of zero on one (image, position, channel) removes exactly that value's log-probability from ll; an image whose
    weights are all zero keeps its KL terms only."""
    c, m, (x, y, eps) = _case("i03_8x8_r_c3_b6_poisson_pramp")
    cfg = pw.case_config(c)
    with torch.no_grad():
        full = orc.elbo({k: v.double() for k, v in state(m).items()}, cfg, x.double(), eps[0].double())
        lp = orc.likelihood(cfg, full["loc"].reshape(6, -1)).log_prob(x.double().reshape(6, -1)).reshape(6, 8, 8, 3)
        w = torch.ones(6, 8, 8, 3)
        w[4, 2, 5, 1] = 0.0
        out = iwc.ImageWeightedOracle(state(m), cfg, w, dtype=torch.float64).loss_and_grads(x, eps[0])
        torch.testing.assert_close(out["ll"], full["ll"] - lp[4, 2, 5, 1], rtol=1e-12, atol=1e-12)
        w = torch.ones(6, 8, 8, 3)
        w[3] = 0.0
        out = iwc.ImageWeightedOracle(state(m), cfg, w, dtype=torch.float64).loss_and_grads(x, eps[0])
        assert out["ll_per_sample"][3].item() == 0.0
        torch.testing.assert_close(out["ll"], full["ll"] - lp[3].sum(), rtol=1e-12, atol=1e-12)
        assert torch.equal(out["logpz"], full["logpz"]) and torch.equal(out["logqz"], full["logqz"])


def test_case_table_is_the_shared_table_with_per_image_makers():
    assert len(iwc.CASES) == len(pw.CASES) == 10
    for (ni, ci), (nw, cw) in zip(sorted(iwc.CASES.items()), sorted(pw.CASES.items())):
        assert ni[1:3] == nw[1:3] and ci["w"] == "p" + cw["w"]
        assert {k: v for k, v in ci.items() if k not in ("w", "zero")} == {k: v for k, v in cw.items() if k != "w"}
        w = iwc.weights(ci)
        assert tuple(w.shape) == (ci["b"],) + tuple(ci["dims"]) + (ci["C"],) and bool((w >= 0).all())
        for i in range(ci["b"]):
            assert (float(w[i].sum()) == 0.0) == (i in ci.get("zero", ()))
    assert iwc.CASES[iwc.CASE1]["zero"] == (2,) and iwc.CASES["i06_16x16_r_c8_b160_pramp"]["zero"] == (0, 159)
    w = iwc.weights(iwc.CASES[iwc.CASE1])
    assert not torch.equal(w[0], w[1])                                 # the discs differ from image to image
    for name in ("i09_8x8_none_c1_b6_psoft", "i10_8x8_none_c2_b6_psoft"):
        assert bool((iwc.weights(iwc.CASES[name]) > 0).all())           # vanilla: strictly positive (see _pixel_weight_cases)


# ------------------------------------------------------------------------------- the GPU step cases' condition
def test_gpu_step_cases_keep_near_zero_gradient_entries_below_one_percent():
    """tests/_judge.py's check_params_after_adam holds entries with |g_ref| < 1e-5 max|g_ref| to 2 lr only, on the condition that
    they are fewer than 1 % of a tensor and that no tensor's gradient vanishes: confirmed here with the float64 reference alone,
    at every case over its two steps (each from float32-rounded parameters, as there), case 1 also with the analytic KL — the
    cases with fully masked images included."""
    torch.set_num_threads(min(8, torch.get_num_threads()))
    worst = 0.0
    for name, c in sorted(iwc.CASES.items()):
        for kl in (("sampled", "analytic") if name == iwc.CASE1 else ("sampled",)):
            _, m, (x, y, eps) = _case(name)
            o = iwc.ImageWeightedOracle(state(m), pw.case_config(c), iwc.weights(c), dtype=torch.float64, kl=kl)
            for k in range(2):
                o.step(x, eps[k], 1.0, y)
                for key, g in o.last_grads.items():
                    assert g.norm().item() > 0.0, "%s %s step %d %s: zero gradient" % (name, kl, k, key)
                    share = near_zero_share(g)
                    worst = max(worst, share)
                    assert share < ILL_SHARE, "%s %s step %d %s: %.2f %% near-zero gradient entries" % (name, kl, k, key, 100 * share)
                mc.round_to_float32(o)
    print("worst near-zero share: %.3f %%" % (100 * worst))
