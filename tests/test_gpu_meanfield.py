"""
GPU tests (-m gpu) of the analytic-KL (mean-field) objective: SVItrainer(loss="TraceMeanField_ELBO"),
model.engine(kl="analytic"), pv_ivae_plan.kl_mode / pv_ved_plan.kl_mode = PV_KL_ANALYTIC.

The reference is oracle.svi_oracle with kl="analytic" (its networks and Adam, torch.distributions.kl_divergence for the
KL term).  Every case runs from identical parameters at each step, as tests/test_gpu_parity.py's step tests do, and holds
the kernels to the bars of the same path (tests/_judge.py).
"""
import ctypes as C
import glob
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import GOLDEN, load_golden, make_x, meta_of

import pyroved_amd as pv
from pyroved_amd import _abi
from oracle import svi_oracle as orc
from _golden_models import convenc_model, ved_case
from _variant_cases import VARIANTS, variant_case
from _judge import (RTOL_ELBO, RTOL_KL, RTOL_GRAD, Z_ATOL, LR, rel_l2, state, reload, check_scalars, check_z, check_grads,
                    check_params_after_adam, steps_vs_reference)

pytestmark = pytest.mark.gpu

ROOT_DIR = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEP_CASES = sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(GOLDEN, "ivae_*.npz"))
                    if not p.endswith("_fwd.npz"))
CONVENC_CASES = sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(GOLDEN, "ivaeconv_*.npz")))
VED_CASES = sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(GOLDEN, "ved_*.npz")))
BF16_CASES = ["ivae_28x28_rt_b256", "ivae_28x28_r_b128", "ivae_28x28_r_b32_blobs", "ivae_8x8_rts_b6", "ivae_8x8_r_b6",
              "ivae_1d16_t_b5", "ivae_8x8_rts_b6_randn", "ivae_8x8_rt_b6_beta4"]

# ------------------------------------------------------------------------------- 1. fp32-class parity
@pytest.mark.parametrize("fused", [0, 1, 2])
@pytest.mark.parametrize("name", STEP_CASES)
def test_meanfield_steps_vs_reference(gpu_device, name, fused):
    """The STEP_CASES fixtures' models, x and eps (only meta and eps are read from the .npz) under the analytic-KL objective."""
    gold = load_golden(name)
    meta = meta_of(gold)
    if meta["batch"] > 64:
        torch.set_num_threads(8)
    model = pv.models.iVAE(meta["data_dim"], meta["latent_dim"], meta["invariances"], seed=1, device="cuda")
    cfg = orc.Config(data_dim=meta["data_dim"], latent_dim=meta["latent_dim"], invariances=meta["invariances"])
    eng = model.engine(fused=fused, kl="analytic")
    o = orc.SVIOracle(state(model), cfg, kl="analytic")
    x = make_x(meta["xkind"], meta["batch"], meta["data_dim"])
    eps = [torch.from_numpy(gold["s%d.eps" % k]) for k in range(meta["steps"])]
    steps_vs_reference(eng, model, o, x, None, eps, meta["beta"], "%s fused=%d" % (name, fused), fused, Z_ATOL)


@pytest.mark.parametrize("fused", [0, 1, 2])
@pytest.mark.parametrize("vname", sorted(VARIANTS))
def test_meanfield_model_variants_vs_reference(gpu_device, vname, fused):
    model, cfg, o, x, y, g = variant_case(vname, kl="analytic")
    eng = model.engine(fused=fused, kl="analytic")
    b, data_dim, odt = x.shape[0], cfg.data_dim, o.dtype
    beta = 1.7
    atol = 1e-6 * b * int(np.prod(data_dim)) if odt == torch.float64 else 0.0
    for k in range(2):
        eps = torch.randn(b, cfg.z_dim, generator=g)
        eng.loss_and_grads(x.cuda(), eps.cuda(), beta, None if y is None else y.cuda())
        o.step(x, eps, beta, y)
        tag = "%s fused=%d step %d" % (vname, fused, k)
        check_scalars(eng.scalars.cpu().numpy(), o.last, tag, atol=atol)
        check_grads(eng, o, tag)
        eng.adam_step()
        reload(model, o)


# ------------------------------------------------------------------------------- 2. every guide route
@pytest.mark.parametrize("route", ["fold_request_b256", "per_image_b256", "tiled_b256", "b600"])
@pytest.mark.parametrize("fused", [2, 3])
def test_meanfield_on_every_guide_route(gpu_device, route, fused):
    """28x28 `rt`: the guide hosted in the throughput decoder launch is REFUSED for the analytic form (pv_ivae_guide_folds == 0:
    that kernel sits at 256 VGPRs with spills and computes the sampled form only — DESIGN.md) and the step runs guide launch +
    decoder launch + latent backward; the per-image guide; the tiled one-launch encoder; batch 600, beyond the per-image
    guide's batch limit.  Same numbers on every route."""
    torch.set_num_threads(8)
    b = 600 if route == "b600" else 256
    data_dim, inv = (28, 28), ["r", "t"]
    g = torch.Generator().manual_seed(31)
    x = torch.rand(b, *data_dim, generator=g)
    model = pv.models.iVAE(data_dim, 2, inv, seed=1, device="cuda")
    eng = model.engine(fused=fused, kl="analytic")
    eng.enc_fold = route == "fold_request_b256"
    eng.enc_per_image = route != "tiled_b256"
    eps = torch.randn(b, model.z_dim, generator=torch.Generator().manual_seed(5))
    assert _abi.lib().pv_ivae_guide_folds(C.byref(eng._plan(b))) == 0           # the documented refusal
    if route == "fold_request_b256" and fused == 3 and torch.cuda.get_device_properties(0).multi_processor_count == 256:
        eng.kl = "sampled"
        assert _abi.lib().pv_ivae_guide_folds(C.byref(eng._plan(b))) == 1       # (the sampled form does fold here)
        eng.kl = "analytic"
    zl, zs = torch.empty(b, model.z_dim, device="cuda"), torch.empty(b, model.z_dim, device="cuda")
    eng.loss_and_grads(x.cuda(), eps.cuda(), 1.3, z_out=(zl, zs))
    torch.cuda.synchronize()
    rec = (eng.scalars.clone(), eng.grad.clone())
    eng.loss_and_grads(x.cuda(), eps.cuda(), 1.3, z_out=(zl, zs))
    assert torch.equal(rec[0], eng.scalars) and torch.equal(rec[1], eng.grad)   # bit-reproducible
    cfg = orc.Config(data_dim=data_dim, latent_dim=2, invariances=inv)
    o = orc.SVIOracle(state(model), cfg, kl="analytic")
    o.step(x, eps, 1.3)
    # fused = 3: the throughput precision's bars (test_bf16_mode_steps_vs_golden_and_oracle, batch >= 128)
    tag = "%s fused=%d" % (route, fused)
    check_scalars(eng.scalars.cpu().numpy(), o.last, tag, loss_rtol=1e-4 if fused == 3 else RTOL_ELBO)
    check_z(zl, zs, o.last, RTOL_KL, Z_ATOL, tag)
    check_grads(eng, o, tag, bar=3e-2 if fused == 3 else RTOL_GRAD)
    eng.loss_and_grads(x.cuda(), eps.cuda(), 1.3, want_grads=False)
    np.testing.assert_allclose(eng.scalars.cpu().numpy(), rec[0].cpu().numpy(), rtol=2e-6)


# ------------------------------------------------------------------------------- 3. throughput precision
@pytest.mark.parametrize("name", BF16_CASES)
def test_meanfield_bf16_mode_steps_vs_reference(gpu_device, name):
    """fused=3 with the bars of test_bf16_mode_steps_vs_golden_and_oracle: loss 1e-4 at batch >= 128 and 5e-4 below, gradients
    3e-2, parameters after Adam within 2.5e-3."""
    gold = load_golden(name)
    meta = meta_of(gold)
    if meta["batch"] > 64:
        torch.set_num_threads(8)
    model = pv.models.iVAE(meta["data_dim"], meta["latent_dim"], meta["invariances"], seed=1, device="cuda")
    cfg = orc.Config(data_dim=meta["data_dim"], latent_dim=meta["latent_dim"], invariances=meta["invariances"])
    eng = model.engine(fused=3, kl="analytic")
    assert eng.uses_fused(meta["batch"])
    o = orc.SVIOracle(state(model), cfg, kl="analytic")
    x = make_x(meta["xkind"], meta["batch"], meta["data_dim"])
    b = meta["batch"]
    zl, zs = torch.empty(b, cfg.z_dim, device="cuda"), torch.empty(b, cfg.z_dim, device="cuda")
    for k in range(meta["steps"]):
        eps = torch.from_numpy(gold["s%d.eps" % k])
        eng.loss_and_grads(x.cuda(), eps.cuda(), meta["beta"], z_out=(zl, zs))
        o.step(x, eps, meta["beta"])
        tag = "%s bf16 step %d" % (name, k)
        check_scalars(eng.scalars.cpu().numpy(), o.last, tag, loss_rtol=1e-4 if b >= 128 else 5e-4)
        check_z(zl, zs, o.last, RTOL_KL, Z_ATOL, tag)
        check_grads(eng, o, tag, bar=3e-2)
        eng.adam_step()
        for key, p in model.state_dict().items():
            assert (p.detach().cpu() - o.p[key].detach()).abs().max().item() <= 2.5e-3, key
        reload(model, o)


# ------------------------------------------------------------------------------- 4. other encoders and decoders
@pytest.mark.parametrize("fused", [0, 2])
@pytest.mark.parametrize("name", CONVENC_CASES)
def test_meanfield_convenc_steps_vs_reference(gpu_device, name, fused):
    """The ivaeconv_* fixtures' models with the bars of test_convenc_steps_vs_golden_and_oracle (decoder.out.bias on the
    absolute scale of its cancelling sum).
    The reference is evaluated in float64 (as for ContinuousBernoulli above).  Measured on ivaeconv_64x64_rts_b4, step 1: the
    float32 evaluation of the reference decides ONE leaky-ReLU sign of the conv stack (of 720 896) differently from float64, which
    puts the float32 reference itself 2.4e-4 .. 2.9e-4 from float64 on the first two convolutions' gradients — the HIP gradients
    sit 1e-6 (fused=0) / 2.6e-6 (fused=2) from float64 there, with no decision differing (tests/test_gpu_parity.py's
    CONV_FLIP_FLOOR notes describe the effect at full size).  The bars are unchanged: 1e-4 on every tensor."""
    gold = load_golden(name)
    meta, model, cfg = convenc_model(gold, "cuda")
    eng = model.engine(fused=fused, kl="analytic")
    o = orc.SVIOracle(state(model), cfg, dtype=torch.float64, kl="analytic")
    x = make_x(meta["xkind"], meta["batch"], meta["data_dim"])
    for k in range(meta["steps"]):
        eps = torch.from_numpy(gold["s%d.eps" % k])
        eng.loss_and_grads(x.cuda(), eps.cuda(), meta["beta"])
        o.step(x, eps, meta["beta"])
        tag = "%s fused=%d step %d" % (name, fused, k)
        check_scalars(eng.scalars.cpu().numpy(), o.last, tag)
        check_grads(eng, o, tag, skip=("decoder.out.bias",))
        bound = 1e-6 * meta["batch"] * int(np.prod(meta["data_dim"]))
        assert (eng.grad_of("decoder.out.bias").cpu() - o.last_grads["decoder.out.bias"]).abs().max().item() < bound
        eng.adam_step()
        reload(model, o, round32=True)


@pytest.mark.parametrize("name", VED_CASES)
def test_meanfield_ved_steps_vs_reference(gpu_device, name):
    """The ved_* fixtures' models at the fp32-class precision, bars of test_ved_steps_vs_golden_and_oracle."""
    gold = load_golden(name)
    c = ved_case(gold)
    model = pv.models.VED(c["input_dim"], c["output_dim"], latent_dim=c["latent_dim"], seed=1, device="cuda", **c["kw"])
    cfg = orc.VedConfig(input_dim=c["input_dim"], output_dim=c["output_dim"], latent_dim=c["latent_dim"],
                        hidden_dim_e=c["kw"].get("hidden_dim_e"), hidden_dim_d=c["kw"].get("hidden_dim_d"),
                        activation=c["kw"].get("activation", "lrelu"))
    eng = model.engine(kl="analytic")
    o = orc.VedOracle(state(model), cfg, kl="analytic")
    x, y = torch.from_numpy(gold["x"]), torch.from_numpy(gold["y"])
    b = x.shape[0]
    zl, zs = torch.empty(b, cfg.z_dim, device="cuda"), torch.empty(b, cfg.z_dim, device="cuda")
    for k in range(c["steps"]):
        eps = torch.from_numpy(gold["s%d.eps" % k])
        eng.loss_and_grads(x.cuda(), eps.cuda(), c["beta"], y.cuda(), z_out=(zl, zs))
        o.step(x, y, eps, c["beta"])
        tag = "%s step %d" % (name, k)
        check_scalars(eng.scalars.cpu().numpy(), o.last, tag)
        check_z(zl, zs, o.last, RTOL_KL, Z_ATOL, tag)
        check_grads(eng, o, tag)
        eng.adam_step()
        # (dead relu / lrelu units give many exactly-zero gradients: no bound on how many entries are near zero)
        check_params_after_adam(model, o, None, tag, ill_share=None)
        reload(model, o)


def test_meanfield_ved_bf16_mode_vs_reference(gpu_device):
    """VED at the throughput precision, bars of test_ved_bf16_mode_vs_oracle: ELBO 1e-4, gradients 3e-2 (5e-2 for the first
    encoder layer's weights at batch 4)."""
    gold = load_golden("ved_64x64_to_128_b4")
    c = ved_case(gold)
    model = pv.models.VED(c["input_dim"], c["output_dim"], latent_dim=c["latent_dim"], seed=1, device="cuda", **c["kw"])
    cfg = orc.VedConfig(input_dim=c["input_dim"], output_dim=c["output_dim"], latent_dim=c["latent_dim"])
    eng = model.engine(fused=3, kl="analytic")
    o = orc.VedOracle(state(model), cfg, kl="analytic")
    x, y = torch.from_numpy(gold["x"]), torch.from_numpy(gold["y"])
    for k in range(c["steps"]):
        eps = torch.from_numpy(gold["s%d.eps" % k])
        eng.loss_and_grads(x.cuda(), eps.cuda(), c["beta"], y.cuda())
        ref = o.step(x, y, eps, c["beta"])
        np.testing.assert_allclose(eng.scalars[0].item(), ref, rtol=1e-4)
        for key in o.p:
            err = rel_l2(eng.grad_of(key), o.last_grads[key])
            bar = 5e-2 if key == "encoder_z.feature_extractor.layers.0.weight" else 3e-2
            assert err < bar, "step %d grad %s: rel l2 %.3e" % (k, key, err)
        eng.adam_step()
        reload(model, o)


class _UserEncoder(torch.nn.Module):
    def __init__(self, data_dim, z_dim):
        super().__init__()
        self.data_dim = data_dim
        self.conv = torch.nn.Conv2d(1, 3, 5, padding=2)
        self.fc = torch.nn.Linear(3 * (data_dim[0] // 2) * (data_dim[1] // 2), 24)
        self.mu = torch.nn.Linear(24, z_dim)
        self.sig = torch.nn.Linear(24, z_dim)

    def forward(self, x):
        h = torch.nn.functional.avg_pool2d(torch.nn.functional.gelu(self.conv(x.reshape(-1, 1, *self.data_dim))), 2)
        h = torch.tanh(self.fc(h.flatten(1)))
        return self.mu(h), torch.nn.functional.softplus(self.sig(h)) + 1e-3


class _UserSpatialDecoder(torch.nn.Module):
    def __init__(self, data_dim, latent_dim):
        super().__init__()
        self.data_dim = data_dim
        self.fx = torch.nn.Linear(4, 24)
        self.fz = torch.nn.Linear(latent_dim, 24)
        self.h = torch.nn.Linear(24, 16)
        self.o = torch.nn.Linear(16, 1)

    def forward(self, xc, z):
        feat = torch.cat([torch.sin(3.0 * xc), torch.cos(3.0 * xc)], -1)
        h = torch.nn.functional.gelu(self.fx(feat)) * torch.sigmoid(self.fz(z)).unsqueeze(1)
        return torch.sigmoid(self.o(torch.tanh(self.h(h)))).reshape(-1, *self.data_dim)


class _UserVanillaDecoder(torch.nn.Module):
    def __init__(self, data_dim, z_dim):
        super().__init__()
        self.data_dim = data_dim
        self.a = torch.nn.Linear(z_dim, 20)
        self.b = torch.nn.Linear(20, data_dim[0] * data_dim[1])

    def forward(self, z):
        return torch.sigmoid(self.b(torch.nn.functional.softplus(self.a(z)))).reshape(-1, *self.data_dim)


@pytest.mark.parametrize("which", ["encoder", "decoder", "both"])
@pytest.mark.parametrize("inv", [["r", "t", "s"], None])
def test_meanfield_user_defined_modules(gpu_device, inv, which):
    """A user-defined encoder (ext_head through the head kernels), a user-defined decoder and both (the library keeps the
    reparameterisation and the KL), built as test_user_defined_* build them: loss, ll, the library-side gradients to the
    bars of those tests (RTOL_ELBO; 1e-4 / 2e-4), the modules' own gradients to 2e-4, parameters after Adam to 1e-4."""
    data_dim, b, beta = (8, 8), 6, 1.3
    torch.manual_seed(5)
    model = pv.models.iVAE(data_dim, 2, inv, seed=1, device="cuda")
    mkd = (lambda: _UserSpatialDecoder(data_dim, 2)) if inv else (lambda: _UserVanillaDecoder(data_dim, 2))
    ue = re_ = ud = rd = None
    if which in ("encoder", "both"):
        ue, re_ = _UserEncoder(data_dim, model.z_dim), _UserEncoder(data_dim, model.z_dim)
        re_.load_state_dict(ue.state_dict())
        model.set_encoder(ue)
    if which in ("decoder", "both"):
        ud, rd = mkd(), mkd()
        rd.load_state_dict(ud.state_dict())
        model.set_decoder(ud)
    eng = model.engine(kl="analytic")
    cfg = orc.Config(data_dim=data_dim, latent_dim=2, invariances=inv, custom_encoder=re_, custom_decoder=rd)
    lib_params = {k: v.cpu() for k, v in model.state_dict().items()
                  if not (ue is not None and k.startswith("encoder_z.")) and not (ud is not None and k.startswith("decoder."))}
    o = orc.SVIOracle(lib_params, cfg, kl="analytic")
    user = [m_ for m_ in (ue, ud) if m_ is not None]
    refs = [m_ for m_ in (re_, rd) if m_ is not None]
    ref_params = [q for m_ in refs for q in m_.parameters()]
    ref_opt = torch.optim.Adam(ref_params, lr=LR)
    g = torch.Generator().manual_seed(2)
    x = torch.rand(b, *data_dim, generator=g)
    for k in range(3):
        eps = torch.randn(b, model.z_dim, generator=g)
        eng.loss_and_grads(x.cuda(), eps.cuda(), beta)
        ref_opt.zero_grad()
        o.step(x, eps, beta)
        check_scalars(eng.scalars.cpu().numpy(), o.last, "%s step %d" % (which, k), relation=False)
        check_grads(eng, o, "%s step %d" % (which, k), bar=RTOL_GRAD if which == "encoder" else 2e-4, skip=("decoder.out.bias",))
        named = [(n, q) for m_ in user for n, q in m_.named_parameters()]
        for (n, pu), pr in zip(named, ref_params):
            assert rel_l2(pu.grad, pr.grad) < 2e-4, "%s %s" % (which, n)
        eng.adam_step()
        ref_opt.step()
        for (n, pu), pr in zip(named, ref_params):
            assert rel_l2(pu.detach(), pr.detach()) < 1e-4, "%s %s after Adam" % (which, n)
        sd = {k_: v_.detach() for k_, v_ in o.p.items()}
        if ue is not None:
            sd.update({"encoder_z." + k_: v_ for k_, v_ in re_.state_dict().items()})
        if ud is not None:
            sd.update({"decoder." + k_: v_ for k_, v_ in rd.state_dict().items()})
        model.load_state_dict(sd)


# ------------------------------------------------------------------------------- 5. surfaces
def test_meanfield_trainer_epochs_vs_reference(gpu_device):
    """SVItrainer(model, loss="TraceMeanField_ELBO") over 3 epochs (train + evaluate) against the helper's train_epoch /
    evaluate_epoch driven by the same loaders and seeds; bar of test_trainer_epochs_vs_golden: 1e-4 per epoch."""
    data_dim, inv, batch = (8, 8), ["r", "t", "s"], 16
    train, test = make_x("rand", 80, data_dim, seed=1), make_x("rand", 32, data_dim, seed=2)

    def loaders():
        return pv.utils.init_dataloader(train, batch_size=batch), pv.utils.init_dataloader(test, batch_size=batch)
    model = pv.models.iVAE(data_dim, 2, inv, seed=1, device="cuda")
    init = state(model)
    trainer = pv.trainers.SVItrainer(model, loss="TraceMeanField_ELBO", seed=1)
    assert trainer.engine.kl == "analytic"
    tl, sl = loaders()
    for _ in range(3):
        trainer.step(tl, sl, scale_factor=1.5)
    from pyroved_amd.utils import set_deterministic_mode
    set_deterministic_mode(1)
    o = orc.SVIOracle(init, orc.Config(data_dim=data_dim, latent_dim=2, invariances=inv), kl="analytic")
    tl, sl = loaders()
    want_train, want_test = [], []
    for _ in range(3):
        want_train.append(o.train_epoch(tl, 1.5))
        want_test.append(o.evaluate_epoch(sl, 1.5))
    print("trainer", trainer.loss_history, "reference", want_train, want_test)
    np.testing.assert_allclose(trainer.loss_history["training_loss"], want_train, rtol=1e-4)
    np.testing.assert_allclose(trainer.loss_history["test_loss"], want_test, rtol=1e-4)
    # ... and a trainer with the default objective on the same model goes back to the sampled form
    assert pv.trainers.SVItrainer(model, seed=1).engine.kl == "sampled"


def test_meanfield_reaches_an_existing_engine_and_composes_with_precision(gpu_device):
    model = pv.models.iVAE((8, 8), 2, ["r", "t"], seed=1, device="cuda")
    model.encode(make_x("rand", 4, (8, 8)))                      # creates the engine with default settings
    assert model.engine().kl == "sampled"
    tr = pv.trainers.SVItrainer(model, loss="TraceMeanField_ELBO", seed=1, precision="bf16", lr=5e-3, rng="device")
    assert tr.engine is model.engine() and tr.engine.kl == "analytic" and tr.engine.fused == 3 and tr.engine.lr == 5e-3
    tr.step(pv.utils.init_dataloader(make_x("rand", 64, (8, 8)), batch_size=16), scale_factor=2.0)
    assert np.isfinite(tr.loss_history["training_loss"][0])
    with pytest.raises(ValueError):
        pv.models.jiVAE((8, 8), 2, 3, None, seed=1, device="cuda").engine(kl="analytic")
    ved = pv.models.VED((32, 32), (32,), latent_dim=2, seed=1, device="cuda")
    assert pv.trainers.SVItrainer(ved, loss="TraceMeanField_ELBO", seed=1).engine.kl == "analytic"


@pytest.mark.parametrize("kind", ["ivae_f2", "ivae_f3", "ivae_f0", "cvae", "convenc", "ivae_f2_b256", "ivae_f3_b256"])
def test_meanfield_one_call_step_is_bit_identical(gpu_device, kind):
    """loss_and_grads(step=True) (pv_ivae_step) against loss_and_grads() + adam_step() under the analytic form: parameters, both
    moments, the zeroed gradients and the scalars bit for bit (as test_one_call_step_is_bit_identical)."""
    torch.manual_seed(3)
    b = 256 if kind.endswith("_b256") else 37

    def make():
        if kind == "cvae":
            m = pv.models.iVAE((28, 28), 2, ["r", "t", "s"], c_dim=3, seed=1, device="cuda")
        else:
            m = pv.models.iVAE((28, 28) if kind != "convenc" else (16, 16), 2, ["r", "t"], seed=1, device="cuda")
            if kind == "convenc":
                m.set_encoder(pv.nets.convEncoderNet((16, 16), latent_dim=m.z_dim, hidden_dim=[(8,), (8, 8)]))
        return m, m.engine(fused={"ivae_f3": 3, "ivae_f0": 0, "ivae_f3_b256": 3}.get(kind, 2), kl="analytic")
    (m1, e1), (m2, e2) = make(), make()
    x = torch.rand(b, *m1.data_dim).cuda()
    y = pv.utils.to_onehot(torch.randint(0, 3, (b,)), 3).cuda() if kind == "cvae" else None
    for k in range(3):
        eps = torch.randn(b, m1.z_dim).cuda()
        e1.loss_and_grads(x, eps, 1.2, y)
        s1 = e1.scalars.clone()
        e1.adam_step()
        hist = torch.zeros(4, device="cuda")
        e2.loss_and_grads(x, eps, 1.2, y, scalars_out=hist, step=True)
        assert torch.equal(s1, hist), (kind, k)
        for name, a, b_ in (("params", e1.flat, e2.flat), ("m", e1.m, e2.m), ("v", e1.v, e2.v),
                            ("grad", e1.grad[:e1.n_flat], e2.grad[:e2.n_flat])):
            assert torch.equal(a, b_), (kind, k, name, (a - b_).abs().max().item())
    assert float(e2.grad[:e2.n_flat].abs().sum()) == 0.0


@pytest.mark.parametrize("family", ["ivae", "ved", "ivae_b256_bf16"])
def test_meanfield_steps_replay_from_a_captured_graph(gpu_device, family):
    """A captured step replays with new inputs to the eager results, bit for bit (as test_steps_replay_from_a_captured_graph)."""
    g = torch.Generator().manual_seed(21)
    if family == "ved":
        model = pv.models.VED((32, 32), (32,), latent_dim=2, seed=1, device="cuda")
        eng = model.engine(kl="analytic")
        xs = [torch.rand(8, 1, 32, 32, generator=g).cuda() for _ in range(3)]
        es = [torch.randn(8, 2, generator=g).cuda() for _ in range(3)]
        ys = [torch.rand(8, 1, 32, generator=g).cuda() for _ in range(3)]
        call = lambda x, e, y: eng.loss_and_grads(x, e, 1.0, y)
    else:
        nb = 32 if family == "ivae" else 256
        model = pv.models.iVAE((28, 28), 2, ["r", "t"], seed=1, device="cuda")
        eng = model.engine(fused=2 if family == "ivae" else 3, kl="analytic")
        xs = [torch.rand(nb, 28, 28, generator=g).cuda() for _ in range(3)]
        es = [torch.randn(nb, model.z_dim, generator=g).cuda() for _ in range(3)]
        ys = [None] * 3
        call = lambda x, e, y: eng.loss_and_grads(x, e)
    want = []
    for x, e, y in zip(xs, es, ys):
        call(x, e, y)
        want.append((eng.scalars.clone(), eng.grad.clone()))
    sx, se = xs[0].clone(), es[0].clone()
    sy = ys[0].clone() if ys[0] is not None else None
    call(sx, se, sy)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        call(sx, se, sy)
    for k in (1, 2, 0):
        sx.copy_(xs[k]); se.copy_(es[k])
        if sy is not None:
            sy.copy_(ys[k])
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(eng.scalars, want[k][0]), "replay %d: loss terms differ" % k
        assert torch.equal(eng.grad, want[k][1]), "replay %d: gradients differ" % k


def test_meanfield_trainer_data_parallel_two_ranks_one_gpu(gpu_device):
    """Two ranks (gloo, sharing the GPU) against the single-process run, the bars of test_trainer_data_parallel_two_ranks_one_gpu."""
    worker = os.path.join(ROOT_DIR, "tests", "_dp_gpu_worker_meanfield.py")

    def run(nproc, port):
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(nproc), "--master-addr",
               "127.0.0.1", "--master-port", str(port), worker]
        out = subprocess.run(cmd, cwd=ROOT_DIR, capture_output=True, text=True, timeout=300)
        assert out.returncode == 0, out.stderr[-2000:]
        line = [ln for ln in out.stdout.splitlines() if ln.startswith("RESULT ")][0]
        return json.loads(line[len("RESULT "):])
    one, two = run(1, 29551), run(2, 29553)
    assert one["kl"] == two["kl"] == "analytic"
    np.testing.assert_allclose(two["train"], one["train"], rtol=2e-5)
    np.testing.assert_allclose(two["test"], one["test"], rtol=2e-3, atol=1e-6)
    np.testing.assert_allclose(two["wsum"], one["wsum"], rtol=1e-5)


@pytest.mark.parametrize("fused", [0, 2, 3])
def test_meanfield_elbo_terms_and_row_elbo_agree_with_the_scalars(gpu_device, fused):
    data_dim, inv, b, beta = (16, 16), ["r", "t"], 24, 1.4
    g = torch.Generator().manual_seed(4)
    x, eps = torch.rand(b, *data_dim, generator=g), torch.randn(b, 5, generator=g)
    model = pv.models.iVAE(data_dim, 2, inv, seed=1, device="cuda")
    eng = model.engine(fused=fused, kl="analytic")
    o = orc.SVIOracle(state(model), orc.Config(data_dim=data_dim, latent_dim=2, invariances=inv), kl="analytic")
    o.step(x, eps, beta)
    terms = model.elbo_terms(x, eps=eps, scale_factor=beta)
    tol = 5e-4 if fused == 3 else RTOL_ELBO
    np.testing.assert_allclose(terms["loss"], o.last["loss"].item(), rtol=tol)
    np.testing.assert_allclose(terms["logpz"], o.last["logpz"].item(), rtol=1e-4)
    np.testing.assert_allclose(terms["logqz"], o.last["logqz"].item(), rtol=1e-4)
    np.testing.assert_allclose(terms["loss"], -(terms["ll"] + terms["logpz"] - terms["logqz"]), rtol=2e-6)
    row = torch.empty(b, device="cuda")
    eng.loss_and_grads(x.cuda(), eps.cuda(), beta, row_elbo=row)
    s = eng.scalars.cpu().numpy()
    np.testing.assert_allclose(-row.sum().item(), s[0], rtol=1e-5)
    want = (o.last["ll_per_sample"] - beta * o.last["kl"]).detach().numpy()
    np.testing.assert_allclose(row.cpu().numpy(), want, rtol=5e-4 if fused == 3 else 5e-5, atol=1e-4)
    # per-sample weights scale both halves of every sample's term
    w = torch.rand(b, generator=g)
    eng.loss_and_grads(x.cuda(), eps.cuda(), beta, row_w=w.cuda(), row_elbo=row)
    np.testing.assert_allclose(eng.scalars[0].item(), -(w.numpy() * want).sum(), rtol=5e-4 if fused == 3 else 5e-5)


@pytest.mark.parametrize("fused", [0, 2, 3])
def test_meanfield_differs_from_the_sampled_objective(gpu_device, fused):
    """Guards against a mode that is silently ignored: same inputs, the two objectives give different loss and gradients, and
    each matches its own reference.  How different: the KL slots s2 / s3 are held to 1e-4 of their reference on every path
    (the guide is fp32 everywhere), so the two forms must sit at least ten such bars apart there for the parity tests to tell
    them apart; the losses must differ by exactly what the slots differ by; the head's gradient by ten times the path's
    gradient bar."""
    data_dim, inv, b = (16, 16), ["r", "t", "s"], 32
    g = torch.Generator().manual_seed(9)
    x, eps = torch.rand(b, *data_dim, generator=g), torch.randn(b, 6, generator=g)
    model = pv.models.iVAE(data_dim, 2, inv, seed=1, device="cuda")
    out = {}
    for kl in ("sampled", "analytic", "sampled"):
        eng = model.engine(fused=fused, kl=kl)
        eng.loss_and_grads(x.cuda(), eps.cuda(), 1.0)
        torch.cuda.synchronize()
        rec = (eng.scalars.clone(), eng.grad[:eng.n_flat].clone())
        if kl in out:
            assert torch.equal(out[kl][0], rec[0]) and torch.equal(out[kl][1], rec[1])      # switching back is exact
        out[kl] = rec
    s, a = out["sampled"], out["analytic"]
    assert s[0][1].item() == pytest.approx(a[0][1].item(), rel=1e-6)                         # the likelihood term is shared
    sv, av = s[0].double().cpu().numpy(), a[0].double().cpu().numpy()
    key = "encoder_z.fc11.weight"
    lo, n = eng._layout[key], eng._views[key].numel()
    gdiff = rel_l2(a[1][lo:lo + n], s[1][lo:lo + n])
    print("fused=%d sampled %s analytic %s head-gradient difference %.3e" % (fused, sv, av, gdiff))
    assert abs(av[2] - sv[2]) > 10 * 1e-4 * abs(sv[2]) and abs(av[3] - sv[3]) > 10 * 1e-4 * abs(sv[3])
    assert av[0] != sv[0]
    np.testing.assert_allclose(av[0] - sv[0], (av[3] - av[2]) - (sv[3] - sv[2]), rtol=0, atol=4e-6 * abs(sv[0]))
    assert gdiff > 10 * (3e-2 if fused == 3 else RTOL_GRAD)
    cfg = orc.Config(data_dim=data_dim, latent_dim=2, invariances=inv)
    for kl in ("sampled", "analytic"):
        o = orc.SVIOracle(state(model), cfg, kl=kl)
        ref = o.step(x, eps, 1.0)
        np.testing.assert_allclose(out[kl][0][0].item(), ref, rtol=5e-4 if fused == 3 else RTOL_ELBO)
