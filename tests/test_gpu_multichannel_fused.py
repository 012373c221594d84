"""
GPU tests (-m gpu) of multi-channel models on the fused f32 decoder kernel: model.engine(fused_channels=True) /
SVItrainer(model, fused_channels=True) -> plan.fused = 1 + PV_PLAN_FUSED_CHANNELS -> pv_sdec_fused_mc_kernel<GRADS, C> and
pv_sdec_fused_mc_reduce_out (pyroved_amd/csrc/pv_sdec_fused_mc.hip).

The reference is the project's float64 oracle (oracle.svi_oracle, Config(channels=C)).  Cases: tests/_multichannel_fused_cases;
data and eps by tests/_multichannel_cases.case_data (seed 0: data first, then eps).  Every step case runs two steps with Adam
between, each from identical float32 parameters, at the bars of tests/test_gpu_multichannel.py: loss and ll 2e-5 (+ that file's
atol for the continuous Bernoulli), the KL scalars 1e-4, z_loc / z_scale rtol 1e-4 atol 5e-6, loc_out and decode rtol 1e-4 atol
2e-6, every gradient tensor 1e-4 relative L2 — and, on their own, each of the C rows of decoder.out.weight and each
decoder.out.bias[c], so that a swapped or dropped channel slot cannot hide in a norm — and the parameters after Adam by
check_params_after_adam's rule with the 5e-5 bar.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import pyroved_amd as pv
from pyroved_amd import _abi
from oracle import svi_oracle as orc
import _multichannel_cases as mc
import _multichannel_fused_cases as fc
from _judge import RTOL_GRAD, LR, rel_l2, state, steps_vs_reference, cpu_threads_16

pytestmark = pytest.mark.gpu


def make(name, **engine_kw):
    c = fc.CASES[name]
    model = pv.models.iVAE(c["dims"], 2, c["inv"], seed=1, device="cuda", **mc.model_kwargs(c))
    return c, model, model.engine(**engine_kw)


def check_channels(eng, o, tag):
    """Each channel's row of d(decoder.out.weight) and each d(decoder.out.bias)[c] against the reference, on its own."""
    gw, gb = eng.grad_of("decoder.out.weight").cpu().double(), eng.grad_of("decoder.out.bias").cpu().double()
    rw, rb = o.last_grads["decoder.out.weight"].double(), o.last_grads["decoder.out.bias"].double()
    assert gw.shape == rw.shape and gb.shape == rb.shape and gw.shape[0] == gb.shape[0] == o.cfg.channels
    errs = []
    for ch in range(gw.shape[0]):
        ew, eb = rel_l2(gw[ch], rw[ch]), rel_l2(gb[ch], rb[ch])
        errs.append((ew, eb))
    print("%s: per channel (out.weight row, out.bias) %s" % (tag, " ".join("(%.1e %.1e)" % e for e in errs)))
    for ch, (ew, eb) in enumerate(errs):
        assert ew < RTOL_GRAD, "%s decoder.out.weight[%d]: rel l2 error %.3e" % (tag, ch, ew)
        assert eb < RTOL_GRAD, "%s decoder.out.bias[%d]: rel error %.3e" % (tag, ch, eb)


def run_steps(name, oracle_kw=None, engine_kw=None):
    c, model, eng = make(name, fused_channels=True, **(engine_kw or {}))
    b, n_obs = c["b"], int(np.prod(c["dims"])) * c["C"]
    assert eng.uses_fused(b) is True and eng.supports_dp_step is False
    x, y, eps = mc.case_data(c)
    o = orc.SVIOracle(state(model), mc.case_config(c), lr=LR, dtype=torch.float64, **(oracle_kw or {}))
    loc = torch.full((b, n_obs), float("nan"), device="cuda")
    steps_vs_reference(eng, model, o, x, y, eps, 1.0, "%s fused_channels" % name, 0, 5e-6, atol=mc.loss_atol(c),
                       checks=[check_channels], loc_out=loc)       # (0: the 5e-5 bar after Adam; z atol 5e-6)
    return c, model, eng, o, x, y


# ------------------------------------------------------------------------------- 1. steps, then decode from the trained state
@pytest.mark.parametrize("name", sorted(fc.CASES))
def test_steps_vs_reference(gpu_device, name):
    c, model, eng, o, x, y = run_steps(name)
    z_loc, _ = model.encode(*((x,) if y is None else (x, y)))
    zc = z_loc[:, -2:] if c["inv"] else z_loc
    dec = model.decode(zc, y)
    assert tuple(dec.shape) == (c["b"],) + tuple(c["dims"]) + (c["C"],)
    want = o.decode(zc, y, rate=True)
    print("%s: decode max abs error %.2e" % (name, (dec.double() - want).abs().max().item()))
    np.testing.assert_allclose(dec.numpy(), want.numpy(), rtol=1e-4, atol=2e-6)


def test_decode_with_a_transform_and_manifold(gpu_device):
    c, model, eng = make(fc.CASE1, fused_channels=True)
    o = orc.SVIOracle(state(model), mc.case_config(c), dtype=torch.float64)
    z = torch.randn(5, 2, generator=torch.Generator().manual_seed(2))
    dec = model.decode(z, angle=0.3, shift=[0.1, -0.2], scale=1.2)
    want = o.decode(z, None, 0.3, [0.1, -0.2], 1.2, rate=True)
    np.testing.assert_allclose(dec.numpy(), want.numpy(), rtol=1e-4, atol=2e-6)
    assert tuple(model.manifold2d(3, plot=False).shape) == (9, 8, 8, 2)


# ------------------------------------------------------------------------------- 2. the mean-field objective, evaluate
def test_analytic_kl_steps(gpu_device):
    run_steps(fc.CASE1, dict(kl="analytic"), dict(kl="analytic"))


def test_evaluate_gives_the_gradient_calls_scalars(gpu_device):
    c, model, eng = make(fc.CASE1, fused_channels=True)
    x, y, eps = mc.case_data(c)
    xg, eg = x.cuda(), eps[0].cuda()
    eng.loss_and_grads(xg, eg, 1.0)
    with_grads = eng.scalars.clone()
    eng.scalars.fill_(float("nan"))
    eng.loss_and_grads(xg, eg, 1.0, want_grads=False)
    torch.cuda.synchronize()
    print("evaluate: %s, gradient call: %s" % (eng.scalars.tolist(), with_grads.tolist()))
    # the same per-row values from the same forward arithmetic; the two closing launches sum them in different (blocked) orders.
    # 384 rows of one sign: a blocked fp32 sum is off by about log2(n) u = 9 * 6e-8 relative; 2e-6 leaves a factor of four
    np.testing.assert_allclose(eng.scalars.cpu().numpy(), with_grads.cpu().numpy(), rtol=2e-6)


# ------------------------------------------------------------------------------- 3. against the layered kernels
@pytest.mark.parametrize("name", [fc.CASE1, fc.CASE5])
def test_agrees_with_the_layered_kernels(gpu_device, name):
    c = fc.CASES[name]
    x, y, eps = mc.case_data(c)
    grads = []
    for kw in (dict(fused=0), dict(fused_channels=True)):
        _, model, eng = make(name, **kw)
        assert eng.uses_fused(c["b"]) is bool(kw.get("fused_channels"))
        eng.loss_and_grads(x.cuda(), eps[0].cuda(), 1.0)
        torch.cuda.synchronize()
        grads.append({k: eng.grad_of(k).clone() for k in model.state_dict()})
    for k in grads[0]:
        err = rel_l2(grads[1][k], grads[0][k])
        assert err < RTOL_GRAD, "%s %s: fused_channels against layered, rel l2 %.3e" % (name, k, err)


# ------------------------------------------------------------------------------- 4. determinism, the whole step
def test_repeated_call_is_bit_identical(gpu_device):
    c, model, eng = make(fc.CASE6, fused_channels=True)
    x, y, eps = mc.case_data(c)
    xg, eg = x.cuda(), eps[0].cuda()
    eng.loss_and_grads(xg, eg, 1.0)
    torch.cuda.synchronize()
    first = eng.grad.clone()
    eng.loss_and_grads(xg, eg, 1.0)
    torch.cuda.synchronize()
    assert torch.equal(first, eng.grad) and torch.isfinite(first).all()


def test_one_call_step_is_bit_identical(gpu_device):
    """loss_and_grads(step=True) (pv_ivae_step: Adam rides in the step's last gradient launch) against loss_and_grads() +
    adam_step(): parameters, both moments, the zeroed gradients and the scalars, bit for bit over two steps — as
    tests/test_gpu_parity.py::test_one_call_step_is_bit_identical holds it."""
    c = fc.CASES[fc.CASE1]
    x, y, eps = mc.case_data(c)
    (_, m1, e1), (_, m2, e2) = make(fc.CASE1, fused_channels=True), make(fc.CASE1, fused_channels=True)
    xg = x.cuda()
    for k in range(2):
        e1.loss_and_grads(xg, eps[k].cuda(), 1.0)
        s1 = e1.scalars.clone()
        e1.adam_step()
        hist = torch.zeros(4, device="cuda")
        e2.loss_and_grads(xg, eps[k].cuda(), 1.0, scalars_out=hist, step=True)
        assert torch.equal(s1, hist), k
        assert e1.adam_t == e2.adam_t == k + 1
        for name, a, b_ in (("params", e1.flat, e2.flat), ("m", e1.m, e2.m), ("v", e1.v, e2.v),
                            ("grad", e1.grad[:e1.n_flat], e2.grad[:e2.n_flat])):
            assert torch.equal(a, b_), (k, name, (a - b_).abs().max().item())
    # every decoder.out row moved: the optimizer saw channels 1 .. C-1 too
    w0 = pv.models.iVAE(c["dims"], 2, c["inv"], seed=1, device="cpu", **mc.model_kwargs(c)).state_dict()["decoder.out.weight"]
    moved = (m2.state_dict()["decoder.out.weight"].cpu() - w0).abs().amax(dim=1)
    assert (moved > 0).all(), moved


# ------------------------------------------------------------------------------- 5. trainer
def test_trainer_history(gpu_device):
    """SVItrainer(model, fused_channels=True): two epochs over case 1's data against SVIOracle.train_epoch (float64) driven by
    the same generator, loss history to 1e-5; evaluate runs; the refusals raise."""
    c = fc.CASES[fc.CASE1]
    x, _, _ = mc.case_data(c)
    loader = pv.utils.init_dataloader(x, batch_size=c["b"])
    model = pv.models.iVAE(c["dims"], 2, c["inv"], seed=1, device="cuda", **mc.model_kwargs(c))
    params0 = state(model)
    tr = pv.trainers.SVItrainer(model, seed=1, fused_channels=True)
    assert tr.engine.uses_fused(c["b"]) is True
    st = torch.get_rng_state()
    for _ in range(2):
        tr.step(loader)
    torch.cuda.synchronize()
    torch.set_rng_state(st)
    o = orc.SVIOracle(params0, mc.case_config(c), lr=LR, dtype=torch.float64)
    want = [o.train_epoch(loader) for _ in range(2)]
    print("trainer: history %s, reference %s" % (tr.loss_history["training_loss"], want))
    np.testing.assert_allclose(tr.loss_history["training_loss"], want, rtol=1e-5)
    assert np.isfinite(tr.evaluate(loader))
    for kw in (dict(num_particles=3), dict(loss="RenyiELBO"), dict(fused=3), dict(precision="bf16"), dict(fused=0)):
        with pytest.raises(ValueError, match="fused_channels"):
            pv.trainers.SVItrainer(model, fused_channels=True, **kw)


# ------------------------------------------------------------------------------- 6. opt-in; one channel
def test_without_the_keyword_nothing_changes(gpu_device):
    """model.engine() and model.engine(fused=1): layered, the layered kernels' bits."""
    c = fc.CASES[fc.CASE1]
    x, y, eps = mc.case_data(c)
    out = []
    for kw in (dict(fused=0), dict(), dict(fused=1)):
        _, model, eng = make(fc.CASE1, **kw)
        assert eng.uses_fused(c["b"]) is False
        eng.loss_and_grads(x.cuda(), eps[0].cuda(), 1.0)
        torch.cuda.synchronize()
        out.append(eng.grad.clone())
    assert torch.equal(out[0], out[1]) and torch.equal(out[0], out[2])


def test_one_channel_keyword_changes_nothing(gpu_device):
    """channels = 1: the plan struct the library sees is the same bytes with and without the keyword (the two engines' own
    buffer addresses apart), for the default request and for fused = 1."""
    skip = {"params", "grads", "adam_m", "adam_v", "grid", "scalars", "ws", "ws_bytes"}
    for kw in (dict(), dict(fused=1)):
        a = pv.models.iVAE((8, 8), 2, ["r", "t", "s"], seed=1, device="cuda").engine(**kw)
        b = pv.models.iVAE((8, 8), 2, ["r", "t", "s"], seed=1, device="cuda").engine(fused_channels=True, **kw)
        pa, pb = a._plan(6), b._plan(6)
        for name, _ in _abi.pv_ivae_plan._fields_:
            if name in skip:
                continue
            va, vb = getattr(pa, name), getattr(pb, name)
            if isinstance(va, (C.Array, C.Structure)):
                assert bytes(va) == bytes(vb), name
            else:
                assert va == vb, name
        assert a.uses_fused(6) is b.uses_fused(6) is True
