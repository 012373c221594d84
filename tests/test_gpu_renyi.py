"""
GPU tests (-m gpu) of the importance-weighted (Renyi / IWAE) bound: SVItrainer(loss="RenyiELBO"),
model.engine(particles=P, renyi=alpha), pv_ivae_renyi_loss_and_grads / pv_ivae_renyi_step.

The reference is oracle.svi_oracle with renyi=alpha (its networks and Adam; one encoder pass, P decoder samples per image
ordered [p][b], the softmax-weighted bound) in float64.  Shapes, seeds and beta are tests/_renyi_cases.py's (the particle tests'
STEP_CASES); tests/test_renyi_cpu.py confirms with the reference alone that their weights are spread (ESS >= 1.9 on some image) and
that the bound sits more than 0.25 nats above the ELBO.

How the bars compose.  Loss, s1 (2e-5), s2 / s3 / z_loc / z_scale (1e-4) and the slot relation (2e-6) are the project's bars
for these paths.  The weights reach theirs through the per-sample likelihood's: each lw inherits the 2e-5 relative bar on
ll, a log-weight is a difference of two lw, so max |log w - log w_ref| <= 2 |1 - alpha| 2e-5 max_s |ll_s| over entries with
w_ref > 1e-6.  The gradients are held to the weighted-sample machinery's 1e-4 relative L2 against the reference evaluated
WITH THE ENGINE'S OWN WEIGHTS held fixed; the error against the free-weight reference is those two composed, printed, and
has no bar of its own.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from conftest import make_x

import pyroved_amd as pv
from pyroved_amd import _abi
from oracle import svi_oracle as orc
from oracle import bf16_plan as bp
from _bf16_judge import judge, GRAD_CEIL, LOSS_CEIL, SELF_CHECK, LIK
from _device import cus, kernel_name
from _judge import (RTOL_ELBO, RTOL_KL, Z_ATOL, LR, rel_l2, state, reload, check_scalars, check_z, check_grads,
                    check_params_after_adam)
from _particles_cases import STEP_CASES
from _renyi_cases import BETA, ALPHAS, case_inputs, weight_check, free_and_held

pytestmark = pytest.mark.gpu

# ------------------------------------------------------------------------------- 1. fp32-class steps
@pytest.mark.parametrize("alpha", ALPHAS)
@pytest.mark.parametrize("fused", [0, 2])
@pytest.mark.parametrize("name", sorted(STEP_CASES))
def test_renyi_steps_vs_reference(gpu_device, name, fused, alpha):
    """Two Adam steps, each from identical parameters (the reference's are loaded into the model after every step).
    The end-to-end gradient error against the free-weight float64 reference is printed (it is the weight bar and
    the held-weight gradient bar composed, and has no bar of its own)."""
    cfg, _, x, y, eps, b, P, beta, model = case_inputs(name, "cuda")
    eng = model.engine(fused=fused, particles=P, renyi=alpha)
    assert eng.supports_dp_step is False and eng.renyi == alpha
    zl, zs = torch.empty(b, cfg.z_dim, device="cuda"), torch.empty(b, cfg.z_dim, device="cuda")
    w = torch.full((P * b,), float("nan"), device="cuda")
    yg = None if y is None else y.cuda()
    worst_e2e, o = 0.0, None
    for k in range(2):
        tag = "%s fused=%d alpha=%g step %d" % (name, fused, alpha, k)
        eng.loss_and_grads(x.cuda(), eps[k].cuda(), beta, yg, z_out=(zl, zs), weights_out=w)
        torch.cuda.synchronize()
        of, g_free, o = free_and_held(state(model), cfg, P, alpha, x, eps[k], beta, y, w, o)
        check_scalars(eng.scalars.cpu().numpy(), of, tag)
        check_z(zl, zs, of, RTOL_KL, Z_ATOL, tag)
        weight_check(tag, w, of, alpha, RTOL_ELBO)
        check_grads(eng, o, tag + ", the engine's weights held")
        worst_e2e = max([worst_e2e] + [rel_l2(eng.grad_of(key), g_free[key]) for key in o.p])
        print("%s: worst gradient rel l2 %.2e end to end (free weights)" % (tag, worst_e2e))
        eng.adam_step()
        check_params_after_adam(model, o, fused, tag)
        reload(model, o)


# ------------------------------------------------------------------------------- 2. throughput precision
@pytest.mark.parametrize("which", ["8x8_rts_b6_p3", "28x28_r_b128_p2"])
def test_renyi_bf16_step_vs_emulated_reference(gpu_device, which):
    """fused=3, alpha = 0, against the reference that rounds where the kernel does (oracle/bf16_plan.py through RenyiOracle),
    with the throughput precision's own judge and ceilings (tests/_bf16_judge.py): loss 1e-5, z_loc / z_scale 1e-5, every gradient tensor
    1e-3 relative L2 — gradients with the engine's weights held, in the emulation and in float64 — and the weight bar with
    that file's LOSS_CEIL in place of 2e-5.  28x28 `r`, B = 128, P = 2 has the 256 samples of a batch whose guide the
    decoder launch would host: it must not fold."""
    threads = torch.get_num_threads()
    torch.set_num_threads(16)                      # (the float64 references)
    try:
        _bf16_body(which)
    finally:
        torch.set_num_threads(threads)


def _bf16_body(which):
    alpha = 0.0
    cfg, params, x, y, eps, b, P, beta, model = case_inputs(which, "cuda")
    eng = model.engine(fused=3, particles=P, renyi=alpha)
    assert eng.uses_fused(b)
    units = P * b * cfg.n_pix // 16
    name = kernel_name(fused=3, units=units, lik=LIK["bernoulli"])
    kernel = "w8" if "pv_sdec_w8_kernel" in name else "w4"
    assert kernel == ("w4" if b == 6 else "w8"), name
    zl, zs = torch.empty(b, cfg.z_dim, device="cuda"), torch.empty(b, cfg.z_dim, device="cuda")
    w = torch.full((P * b,), float("nan"), device="cuda")
    eng.loss_and_grads(x.cuda(), eps[0].cuda(), beta, z_out=(zl, zs), weights_out=w)
    torch.cuda.synchronize()
    wc = w.cpu().double()

    def reference(plan):
        c = orc.Config(data_dim=cfg.data_dim, latent_dim=2, invariances=cfg.invariances, bf16_plan=plan)
        free = orc.SVIOracle(params, c, dtype=torch.float64, particles=P, renyi=alpha)
        with torch.set_grad_enabled(plan is None):           # (float64: also the free-weight gradient, for the end-to-end figure)
            out = free.loss_and_grads(x, eps[0], beta)
        g_free = {k: v.grad.detach().clone() for k, v in free.p.items()} if plan is None else None
        o = orc.SVIOracle(params, c, dtype=torch.float64, particles=P, renyi=alpha)
        o.weights = wc
        o.loss_and_grads(x, eps[0], beta)
        return out, {k: v.grad.detach().clone() for k, v in o.p.items()}, g_free
    ref_out, ref_g, _ = reference(bp.Bf16Plan(kernel=kernel, cus=cus()))
    f64_out, f64_g, f64_free = reference(None)
    tag = "%s renyi" % which
    print("%s: worst gradient rel l2 end to end (free-weight float64 reference) %.2e"
          % (tag, max(rel_l2(eng.grad_of(k), f64_free[k]) for k in f64_free)))
    judge(tag, eng, ref_out, ref_g, f64_out, f64_g, zl.cpu(), zs.cpu(), GRAD_CEIL, LOSS_CEIL, SELF_CHECK)
    weight_check(tag, w, ref_out, alpha, LOSS_CEIL)
    s = eng.scalars.cpu().numpy()
    np.testing.assert_allclose(s[0], -(s[1] + s[2] - s[3]), rtol=2e-6)
    np.testing.assert_allclose(s[2], ref_out["logpz"].item(), rtol=RTOL_KL)
    np.testing.assert_allclose(s[3], ref_out["logqz"].item(), rtol=RTOL_KL)


# ------------------------------------------------------------------------------- 3. with and without gradients
def _run(eng, x, eps, beta, yg, P, b, **kw):
    w = torch.full((P * b,), float("nan"), device="cuda")
    eng.loss_and_grads(x, eps, beta, yg, weights_out=w, **kw)
    torch.cuda.synchronize()
    return eng.scalars.clone(), w


@pytest.mark.parametrize("fused", [0, 2, 3])
@pytest.mark.parametrize("name", ["8x8_rts_b6_p3", "8x8_none_b6_p3", "16x16_r_gauss_b4_p2"])
def test_forward_only_call_gives_the_same_scalars_and_weights(gpu_device, name, fused):
    """want_grads=False == want_grads=True in the four scalars and the weights, bit for bit: the loss of a gradient step is
    that of the forward the weights came from."""
    cfg, _, x, y, eps, b, P, beta, model = case_inputs(name, "cuda")
    eng = model.engine(fused=fused, particles=P, renyi=0.5)
    yg = None if y is None else y.cuda()
    s1, w1 = _run(eng, x.cuda(), eps[0].cuda(), beta, yg, P, b, want_grads=True)
    s0, w0 = _run(eng, x.cuda(), eps[0].cuda(), beta, yg, P, b, want_grads=False)
    assert torch.equal(s0, s1), (s0, s1)
    assert torch.equal(w0, w1)
    assert not torch.isnan(w0).any()


def test_forward_and_training_launches_with_different_weight_images(gpu_device):
    """fused=2 with the fp16 build of the training kernel forced (dec_kernel = 21): its weight images are not the forward-only
    launch's, so the gradient step prepares images twice.  Scalars and weights stay those of the forward-only call bit for
    bit, at the fp32-class bars against the reference; the gradients with the engine's weights held meet that build's bar
    on toy problems, max(2.5e-4, 0.03 / sqrt(rows)) (tests/_judge.py: h2_grad_tol)."""
    from pyroved_amd.engine import IVAEEngine
    name, alpha = "8x8_rts_b6_p3", 0.0
    cfg, _, x, y, eps, b, P, beta, model = case_inputs(name, "cuda")
    IVAEEngine.dec_kernel = 21
    try:
        eng = model.engine(fused=2, particles=P, renyi=alpha)
        assert eng._plan(b).dec_kernel == 21
        s1, w1 = _run(eng, x.cuda(), eps[0].cuda(), beta, None, P, b, want_grads=True)
        grads = {k: eng.grad_of(k).clone() for k in state(model)}
        s0, w0 = _run(eng, x.cuda(), eps[0].cuda(), beta, None, P, b, want_grads=False)
    finally:
        IVAEEngine.dec_kernel = 0
    assert torch.equal(s0, s1) and torch.equal(w0, w1)
    of, _, o = free_and_held(state(model), cfg, P, alpha, x, eps[0], beta, y, w1)
    check_scalars(s1.cpu().numpy(), of, name + " h221")
    weight_check(name + " h221", w1, of, alpha, RTOL_ELBO)
    tol = max(2.5e-4, 0.03 / (P * b * cfg.n_pix) ** 0.5)
    for key in o.p:
        err = rel_l2(grads[key], o.last_grads[key])
        assert err < tol, "grad %s: rel l2 error %.3e (bar %.2e)" % (key, err, tol)


# ------------------------------------------------------------------------------- 4. the one-call step
@pytest.mark.parametrize("fused", [0, 2, 3])
def test_one_call_renyi_step_equals_loss_and_grads_plus_adam(gpu_device, fused):
    """loss_and_grads(step=True) (pv_ivae_renyi_step) == loss_and_grads() + adam_step(), bit for bit, at P = 3: two steps."""
    data_dim, inv, b, P = (8, 8), ["r", "t", "s"], 6, 3
    x = make_x("rand", b, data_dim).cuda()
    g = torch.Generator()
    runs = []
    for one_call in (False, True):
        model = pv.models.iVAE(data_dim, 2, inv, seed=1, device="cuda")
        eng = model.engine(fused=fused, particles=P, renyi=0.0)
        g.manual_seed(29)
        sc = []
        for _ in range(2):
            eps = torch.randn(P * b, model.z_dim, generator=g).cuda()
            w = torch.empty(P * b, device="cuda")
            eng.loss_and_grads(x, eps, BETA, step=one_call, weights_out=w)
            sc.append((eng.scalars.clone(), w))
            if not one_call:
                eng.adam_step()
        torch.cuda.synchronize()
        runs.append((eng.flat.clone(), eng.m.clone(), eng.v.clone(), eng.grad[:eng.n_flat].clone(), sc, eng.adam_t))
    a, b_ = runs
    assert a[5] == b_[5] == 2
    for i in range(4):
        assert torch.equal(a[i], b_[i]), ("flat", "m", "v", "grad")[i]
    for (s0, w0), (s1, w1) in zip(a[4], b_[4]):
        assert torch.equal(s0, s1) and torch.equal(w0, w1)
    assert float(a[3].abs().max()) == 0.0                    # zero_grads


# ------------------------------------------------------------------------------- 5. reproducibility
@pytest.mark.parametrize("fused", [0, 2, 3])
@pytest.mark.parametrize("name", ["8x8_rts_b6_p3", "1d16_t_b5_p7"])
def test_renyi_step_is_bit_reproducible(gpu_device, name, fused):
    """The same step twice from the same state: bit-identical scalars, weights and gradients (the sums over particles run in
    ascending order in one thread; nothing is accumulated with float atomics)."""
    cfg, _, x, y, eps, b, P, beta, model = case_inputs(name, "cuda")
    eng = model.engine(fused=fused, particles=P, renyi=0.0)
    outs = []
    for _ in range(2):
        eng.grad.zero_()
        s, w = _run(eng, x.cuda(), eps[0].cuda(), beta, None if y is None else y.cuda(), P, b)
        outs.append((s, w, eng.grad.clone()))
    for u, v in zip(outs[0], outs[1]):
        assert torch.equal(u, v)


# ------------------------------------------------------------------------------- 6. one particle is the plain step
@pytest.mark.parametrize("fused", [0, 2, 3])
def test_renyi_with_one_particle_is_the_plain_step_bit_for_bit(gpu_device, fused):
    """engine(particles=1, renyi=alpha) and the library's entry points with num_particles = 1 forward to the one-particle
    step: bit-identical scalars and flat gradient, weights all 1."""
    data_dim, inv, b = (8, 8), ["r", "t", "s"], 6
    x = make_x("rand", b, data_dim).cuda()
    model = pv.models.iVAE(data_dim, 2, inv, seed=1, device="cuda")
    eps = torch.randn(b, model.z_dim, generator=torch.Generator().manual_seed(3)).cuda()
    eng = model.engine(fused=fused)
    assert eng.particles == 1 and eng.renyi is None
    eng.loss_and_grads(x, eps, 1.3)
    torch.cuda.synchronize()
    want = (eng.scalars.clone(), eng.grad.clone())
    for alpha in (0.0, 0.5, -1.0):
        eng.grad.zero_()
        w = torch.zeros(b, device="cuda")
        e2 = model.engine(particles=1, renyi=alpha)
        assert e2 is eng and eng.renyi == alpha and not eng.supports_dp_step
        e2.loss_and_grads(x, eps, 1.3, weights_out=w)
        torch.cuda.synchronize()
        assert torch.equal(eng.scalars, want[0]) and torch.equal(eng.grad, want[1])
        assert torch.equal(w, torch.ones(b, device="cuda"))
    model.engine(renyi=False)
    assert eng.renyi is None and eng.supports_dp_step
    lib = _abi.lib()
    p = eng._plan(b, 1.3)
    assert lib.pv_ivae_renyi_workspace_bytes(C.byref(p), 1) == lib.pv_ivae_workspace_bytes_for(C.byref(p), 1)
    eng.grad.zero_()
    p.x, p.eps = x.data_ptr(), eps.data_ptr()
    try:
        _abi.check(lib.pv_ivae_renyi_loss_and_grads(C.byref(p), 1, 0.0, 1, None, _abi.current_stream()), "renyi(1)")
    finally:
        p.x = p.eps = None
    torch.cuda.synchronize()
    assert torch.equal(eng.scalars, want[0]) and torch.equal(eng.grad, want[1])


# ------------------------------------------------------------------------------- 7. through the trainer
def test_trainer_with_three_particles_vs_reference_loop(gpu_device):
    """SVItrainer(model, loss="RenyiELBO", num_particles=3, alpha=0.5, seed=1).step(loader), two epochs on 8x8 `rts`, 18 images
    in batches of 6, against the RenyiOracle loop driven by the same generator: loss_history to 2e-5."""
    data_dim, inv, P, alpha = (8, 8), ["r", "t", "s"], 3, 0.5
    x = make_x("rand", 18, data_dim, seed=4)
    loader = pv.utils.init_dataloader(x, batch_size=6)
    model = pv.models.iVAE(data_dim, 2, inv, seed=1, device="cuda")
    params0 = state(model)
    tr = pv.trainers.SVItrainer(model, loss="RenyiELBO", num_particles=P, alpha=alpha, seed=1)
    assert tr.num_particles == P and tr.engine.particles == P and tr.engine.renyi == alpha
    st = torch.get_rng_state()
    for _ in range(2):
        tr.step(loader)
    torch.cuda.synchronize()
    torch.set_rng_state(st)
    cfg = orc.Config(data_dim=data_dim, latent_dim=2, invariances=inv)
    o = orc.SVIOracle(params0, cfg, lr=LR, dtype=torch.float64, particles=P, renyi=alpha)
    want = [o.train_epoch(loader) for _ in range(2)]
    print("trainer RenyiELBO P=3 alpha=0.5: history %s, reference %s" % (tr.loss_history["training_loss"], want))
    np.testing.assert_allclose(tr.loss_history["training_loss"], want, rtol=RTOL_ELBO)
    # another objective on the same model returns the engine to the ELBO
    tr2 = pv.trainers.SVItrainer(model, seed=1)
    assert tr2.engine is tr.engine and tr2.engine.renyi is None and tr2.engine.particles == 1
