"""
GPU tests (-m gpu) of the multi-particle ELBO: SVItrainer(num_particles=P), model.engine(particles=P),
pv_ivae_particles_loss_and_grads / pv_ivae_particles_step.

The reference is oracle.svi_oracle with particles=P (its networks and Adam; one encoder pass, P decoder samples per
image ordered [p][b], the mean over particles).  Inputs are conftest.make_x and eps from a seeded torch.Generator
(tests/_particles_cases.py).  The bars are tests/_judge.py's, the ones every fp32-class path is held to; averaging over
particles loosens none of them.  Shapes are the smallest at which each new piece can go wrong.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from conftest import load_golden, make_x, meta_of

import pyroved_amd as pv
from pyroved_amd import _abi
from oracle import svi_oracle as orc
from oracle import bf16_plan as bp
from _bf16_judge import judge, GRAD_CEIL, LOSS_CEIL, SELF_CHECK, LIK
from _device import cus, kernel_name
from _judge import RTOL_ELBO, RTOL_KL, Z_ATOL, state, check_params_after_adam, steps_vs_reference
from _particles_cases import STEP_CASES, step_case, oracle_of

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------------------- 1. fp32-class steps
@pytest.mark.parametrize("kl", ["sampled", "analytic"])
@pytest.mark.parametrize("fused", [0, 2])
@pytest.mark.parametrize("name", sorted(STEP_CASES))
def test_particle_steps_vs_reference(gpu_device, name, fused, kl):
    """Two Adam steps, each from identical parameters (the oracle's are reloaded after every step)."""
    model, cfg, x, y, eps, b, P = step_case(name, "cuda")
    eng = model.engine(fused=fused, kl=kl, particles=P)
    assert eng.supports_dp_step is False
    o = oracle_of(kl, state(model), cfg, P)
    steps_vs_reference(eng, model, o, x, y, eps, 1.7, "%s fused=%d %s" % (name, fused, kl), fused, Z_ATOL)


# ------------------------------------------------------------------------------- 2. throughput precision
def _bf16_case(which):
    if which == "8x8_rts_b6_p3":
        return (8, 8), ["r", "t", "s"], 6, 3, "rand"
    meta = meta_of(load_golden("ivae_28x28_r_b128"))     # S = P * B = 256 = the decoder grid on a 256-CU device
    assert meta["batch"] == 128
    return meta["data_dim"], meta["invariances"], meta["batch"], 2, meta["xkind"]


@pytest.mark.parametrize("kl", ["sampled", "analytic"])
@pytest.mark.parametrize("which", ["8x8_rts_b6_p3", "28x28_r_b128_p2"])
def test_particle_bf16_step_vs_emulated_reference(gpu_device, which, kl):
    """fused=3 against the reference that rounds where the kernel does (oracle/bf16_plan.py through the particle oracle: the
    decoder's P*B samples take the kernel's unit partition), with the throughput precision's own judge (tests/_bf16_judge.py) and its
    ceilings: loss 1e-5, every gradient tensor 1e-3 relative L2, z_loc / z_scale 1e-5, and a tensor more than 1e-3 from the
    float64 gradient at least 10x closer to the emulation.  28x28 `r`, B = 128, P = 2 has the 256 samples of a batch whose
    guide the decoder launch would host: a fold decided on the sample count computes the wrong guide here."""
    data_dim, inv, b, P, xkind = _bf16_case(which)
    threads = torch.get_num_threads()
    torch.set_num_threads(16)                      # (the float64 references)
    try:
        _bf16_case_body(which, kl, data_dim, inv, b, P, xkind)
    finally:
        torch.set_num_threads(threads)


def _bf16_case_body(which, kl, data_dim, inv, b, P, xkind):
    model = pv.models.iVAE(data_dim, 2, inv, seed=1, device="cuda")
    eng = model.engine(fused=3, kl=kl, particles=P)
    assert eng.uses_fused(b)
    n_pix = int(np.prod(data_dim))
    units = P * b * n_pix // 16
    name = kernel_name(fused=3, units=units, lik=LIK["bernoulli"])
    kernel = "w8" if "pv_sdec_w8_kernel" in name else "w4"
    assert kernel == ("w4" if b == 6 else "w8"), name
    x = make_x(xkind, b, data_dim)
    eps = torch.randn(P * b, model.z_dim, generator=torch.Generator().manual_seed(23))
    zl, zs = torch.empty(b, model.z_dim, device="cuda"), torch.empty(b, model.z_dim, device="cuda")
    eng.loss_and_grads(x.cuda(), eps.cuda(), 1.0, z_out=(zl, zs))
    torch.cuda.synchronize()
    params = state(model)

    def reference(plan):
        cfg = orc.Config(data_dim=data_dim, latent_dim=2, invariances=inv, bf16_plan=plan)
        o = oracle_of(kl, params, cfg, P, dtype=torch.float64)
        out = o.loss_and_grads(x, eps, 1.0)
        return out, {k: v.grad.detach().clone() for k, v in o.p.items()}
    ref_out, ref_g = reference(bp.Bf16Plan(kernel=kernel, cus=cus()))
    f64_out, f64_g = reference(None)
    judge("%s %s" % (which, kl), eng, ref_out, ref_g, f64_out, f64_g, zl.cpu(), zs.cpu(), GRAD_CEIL, LOSS_CEIL, SELF_CHECK)
    s = eng.scalars.cpu().numpy()
    np.testing.assert_allclose(s[0], -(s[1] + s[2] - s[3]), rtol=2e-6)
    np.testing.assert_allclose(s[2], ref_out["logpz"].item(), rtol=RTOL_KL)
    np.testing.assert_allclose(s[3], ref_out["logqz"].item(), rtol=RTOL_KL)


# ------------------------------------------------------------------------------- 3. one encoder pass, P decoder samples
@pytest.mark.parametrize("fused", [0, 2])
@pytest.mark.parametrize("name", ["8x8_rts_b6_p3", "8x8_none_b6_p3", "8x8_rt_cdim3_b6_p2"])
def test_one_encoder_pass_feeds_p_decoder_samples(gpu_device, name, fused):
    """loc[p*B + b] of the particle call is the forward of a one-particle call fed eps[p*B:(p+1)*B] (to 1e-5); z_loc and
    z_scale, (B, z_dim), are the same bits in every call."""
    model, cfg, x, y, eps, b, P = step_case(name, "cuda")
    n_pix = int(np.prod(cfg.data_dim))
    xg, eg, yg = x.cuda(), eps[0].cuda(), None if y is None else y.cuda()
    eng = model.engine(fused=fused, particles=P)
    loc = torch.full((P * b, n_pix), float("nan"), device="cuda")
    zl, zs = torch.empty(b, cfg.z_dim, device="cuda"), torch.empty(b, cfg.z_dim, device="cuda")
    for grads in (True, False):
        loc.fill_(float("nan"))
        eng.loss_and_grads(xg, eg, 1.0, yg, want_grads=grads, z_out=(zl, zs), loc_out=loc)
        torch.cuda.synchronize()
        got = (loc.clone(), zl.clone(), zs.clone(), eng.scalars.clone())
        eng1 = model.engine(particles=1)
        assert eng1 is eng and eng.particles == 1 and eng.supports_dp_step
        ll = 0.0
        for p in range(P):
            loc1 = torch.empty(b, n_pix, device="cuda")
            zl1, zs1 = torch.empty_like(zl), torch.empty_like(zs)
            eng.loss_and_grads(xg, eg[p * b:(p + 1) * b], 1.0, yg, want_grads=grads, z_out=(zl1, zs1), loc_out=loc1)
            torch.cuda.synchronize()
            np.testing.assert_allclose(got[0][p * b:(p + 1) * b].cpu().numpy(), loc1.cpu().numpy(), rtol=0, atol=1e-5)
            assert torch.equal(zl1, got[1]) and torch.equal(zs1, got[2]), "particle %d" % p
            ll += eng.scalars[1].item() / P
        np.testing.assert_allclose(got[3][1].item(), ll, rtol=RTOL_ELBO)
        model.engine(particles=P)


# ------------------------------------------------------------------------------- 4. P = 1 is the old step
@pytest.mark.parametrize("fused", [0, 2, 3])
@pytest.mark.parametrize("shape", ["8x8_rts_b6", "28x28_rt_b256"])
def test_one_particle_is_the_old_step_bit_for_bit(gpu_device, shape, fused):
    """engine(particles=1) and the default engine, and the library's particle entry points called with num_particles = 1
    on the same plan, give bit-identical scalars and flat gradient (28x28 `rt` at batch 256 with fused=3: the step whose
    guide the decoder launch hosts)."""
    data_dim, inv, b = ((8, 8), ["r", "t", "s"], 6) if shape == "8x8_rts_b6" else ((28, 28), ["r", "t"], 256)
    x = make_x("rand", b, data_dim).cuda()
    model = pv.models.iVAE(data_dim, 2, inv, seed=1, device="cuda")
    eps = torch.randn(b, model.z_dim, generator=torch.Generator().manual_seed(3)).cuda()
    eng = model.engine(fused=fused)
    assert eng.particles == 1
    folds = _abi.lib().pv_ivae_guide_folds(C.byref(eng._plan(b)))
    if shape == "28x28_rt_b256" and fused == 3 and cus() == 256:
        assert folds == 1
    eng.loss_and_grads(x, eps, 1.3)
    torch.cuda.synchronize()
    want = (eng.scalars.clone(), eng.grad.clone())
    eng.grad.zero_()
    model.engine(particles=1).loss_and_grads(x, eps, 1.3)
    torch.cuda.synchronize()
    assert torch.equal(eng.scalars, want[0]) and torch.equal(eng.grad, want[1])
    # the C entry points with num_particles = 1 forward to the one-particle ones
    lib = _abi.lib()
    p = eng._plan(b, 1.3)
    assert lib.pv_ivae_particles_workspace_bytes(C.byref(p), 1) == lib.pv_ivae_workspace_bytes_for(C.byref(p), 1)
    eng.grad.zero_()
    p.x, p.eps = x.data_ptr(), eps.data_ptr()
    try:
        _abi.check(lib.pv_ivae_particles_loss_and_grads(C.byref(p), 1, 1, _abi.current_stream()), "particles(1)")
    finally:
        p.x = p.eps = None
    torch.cuda.synchronize()
    assert torch.equal(eng.scalars, want[0]) and torch.equal(eng.grad, want[1])


# ------------------------------------------------------------------------------- 5. the one-call step
@pytest.mark.parametrize("kl", ["sampled", "analytic"])
@pytest.mark.parametrize("fused", [0, 2, 3])
def test_one_call_particle_step_equals_loss_and_grads_plus_adam(gpu_device, fused, kl):
    """loss_and_grads(step=True) (pv_ivae_particles_step) == loss_and_grads() + adam_step(), bit for bit, at P = 3: two steps."""
    data_dim, inv, b, P = (8, 8), ["r", "t", "s"], 6, 3
    x = make_x("rand", b, data_dim).cuda()
    g = torch.Generator().manual_seed(29)
    runs = []
    for one_call in (False, True):
        model = pv.models.iVAE(data_dim, 2, inv, seed=1, device="cuda")
        eng = model.engine(fused=fused, kl=kl, particles=P)
        g.manual_seed(29)
        sc = []
        for _ in range(2):
            eps = torch.randn(P * b, model.z_dim, generator=g).cuda()
            eng.loss_and_grads(x, eps, 1.0, step=one_call)
            sc.append(eng.scalars.clone())
            if not one_call:
                eng.adam_step()
        torch.cuda.synchronize()
        runs.append((eng.flat.clone(), eng.m.clone(), eng.v.clone(), eng.grad[:eng.n_flat].clone(), sc, eng.adam_t))
    a, b_ = runs
    assert a[5] == b_[5] == 2
    for i in range(4):
        assert torch.equal(a[i], b_[i]), ("flat", "m", "v", "grad")[i]
    for s0, s1 in zip(a[4], b_[4]):
        assert torch.equal(s0, s1)
    assert float(a[3].abs().max()) == 0.0                    # zero_grads


# ------------------------------------------------------------------------------- 6. through the trainer
@pytest.mark.parametrize("loss", [None, "TraceMeanField_ELBO"])
def test_trainer_with_three_particles_vs_reference_loop(gpu_device, loss):
    """SVItrainer(model, num_particles=3, seed=1).step(loader), two epochs on 8x8 `rt`, 24 images in batches of 6, against the
    reference loop driven by the same generator: loss_history to 2e-5, the final parameters by check_params_after_adam's
    rule.  (Without the feature the keyword is swallowed and the trainer runs one particle: the losses differ.)"""
    data_dim, inv, P = (8, 8), ["r", "t"], 3
    x = make_x("rand", 24, data_dim, seed=4)
    loader = pv.utils.init_dataloader(x, batch_size=6)
    model = pv.models.iVAE(data_dim, 2, inv, seed=1, device="cuda")
    params0 = state(model)
    tr = pv.trainers.SVItrainer(model, loss=loss, num_particles=P, seed=1)
    assert tr.num_particles == P and tr.engine.particles == P
    st = torch.get_rng_state()
    for _ in range(2):
        tr.step(loader)
    torch.cuda.synchronize()
    torch.set_rng_state(st)
    cfg = orc.Config(data_dim=data_dim, latent_dim=2, invariances=inv)
    o = oracle_of("analytic" if loss else "sampled", params0, cfg, P)
    want = [o.train_epoch(loader) for _ in range(2)]
    print("trainer P=3 %s: history %s, reference %s" % (loss, tr.loss_history["training_loss"], want))
    np.testing.assert_allclose(tr.loss_history["training_loss"], want, rtol=RTOL_ELBO)
    check_params_after_adam(model, o, tr.engine.fused, "trainer %s" % loss)


# ------------------------------------------------------------------------------- 7. reproducibility
@pytest.mark.parametrize("fused", [0, 2, 3])
@pytest.mark.parametrize("name", ["8x8_rts_b6_p3", "1d16_t_b5_p7"])
def test_particle_step_is_bit_reproducible(gpu_device, name, fused):
    """The same step twice from the same state: bit-identical scalars and gradients (every sum over particles runs in a
    fixed order; nothing is accumulated with float atomics)."""
    model, cfg, x, y, eps, b, P = step_case(name, "cuda")
    eng = model.engine(fused=fused, particles=P)
    outs = []
    for _ in range(2):
        eng.grad.zero_()
        eng.loss_and_grads(x.cuda(), eps[0].cuda(), 1.0, None if y is None else y.cuda())
        torch.cuda.synchronize()
        outs.append((eng.scalars.clone(), eng.grad.clone()))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
