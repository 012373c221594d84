"""
GPU tests (-m gpu) of the held-out log-evidence: pv_logmeanexp_update / pv_logmeanexp_finish, pv_ivae_evidence_accumulate,
engine.log_evidence_chunk, iVAE.log_evidence and SVItrainer.log_evidence.

The reference is the frozen oracle, orc.elbo(..., beta=1, particles=K, renyi=0.0) in float64: bound_per_image is log p^(x_b)
and 1 / sum_k w^2 the effective sample size (tests/_evidence_kit.py, which also states how the project's bars compose:
|d log p^| <= ll_bar max |ll| and |d log ESS| <= 4 ll_bar max |ll|, ll_bar = 2e-5 against float64 for fused 0 / 2 and
LOSS_CEIL = 1e-5 against the reference that rounds where the kernel does for fused 3).
The two generic kernels are judged against float64 torch.logsumexp of the same float32 table at fp32's own precision.  With
u = 2^-24: a term e^(lw - m) carries the rounding of its argument (|d| u, and |d| e^d <= 0.37 of the largest term, which is 1 <=
s), one fp32 exp (2 u) and the K - 1 additions of the running sum (u each), so the sum s is within (2 K + 8) u of exact,
relative, and so is log s in absolute terms (s >= 1); m + (log s - log K) adds two roundings of a value no larger than
max |lw| + log K.  Bar on log p^: (2 K + 8) u + 2 u max |lw|.  ESS = s^2 / q compounds three such sums: 4 (2 K + 8) u relative.
"""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import pyroved_amd as pv
from pyroved_amd import _abi
from oracle import svi_oracle as orc
from _categorical_cases import categorical_oracle          # noqa: F401  (fixture)
from _device import cus
from _judge import RTOL_ELBO, state
from _judge import cpu_threads_16                           # noqa: F401  (autouse fixture: the float64 references)
import _evidence_kit as ek

pytestmark = pytest.mark.gpu
EPS32 = 2.0 ** -24


# ------------------------------------------------------------------------------- 1. the two generic kernels
def lme_gpu(lw, chunks, st0=None):
    """lw (K, B) float32 on the device through pv_logmeanexp_update per chunk and pv_logmeanexp_finish: (log mean, ess, state)."""
    lib = _abi.lib()
    K, B = lw.shape
    st = torch.empty(B, 4, device="cuda") if st0 is None else st0
    k0 = 0
    for i, P in enumerate(chunks):
        c = lw[k0:k0 + P].contiguous()
        k0 += P
        _abi.check(lib.pv_logmeanexp_update(_abi.ptr(c), P, B, _abi.ptr(st), int(i == 0), _abi.current_stream()), "update")
    out, ess = torch.empty(B, device="cuda"), torch.empty(B, device="cuda")
    _abi.check(lib.pv_logmeanexp_finish(_abi.ptr(st), B, K, _abi.ptr(out), _abi.ptr(ess), _abi.current_stream()), "finish")
    torch.cuda.synchronize()
    return out.cpu(), ess.cpu(), st


def lme_check(tag, lw, chunks):
    K = lw.shape[0]
    ev, ess, _ = lme_gpu(lw.cuda(), chunks)
    d = lw.double()
    want = torch.logsumexp(d, 0) - math.log(K)
    w = torch.softmax(d, 0)
    want_ess = 1.0 / (w * w).sum(0)
    sums = (2 * K + 8) * EPS32
    bar = sums + 2 * EPS32 * d.abs().max().item()
    err = (ev.double() - want).abs().max().item()
    eerr = (ess.double() / want_ess - 1).abs().max().item()
    print("%s chunks %s: max |log mean - ref| %.3e (bar %.3e), ESS rel err %.3e (bar %.3e)" % (tag, chunks, err, bar, eerr, 4 * sums))
    assert err <= bar, (tag, chunks, err, bar)
    assert eerr <= 4 * sums, (tag, chunks, eerr)
    assert (ess >= 1 - 1e-5).all() and (ess <= K * (1 + 1e-5)).all()
    return ev, ess


def uneven(K):
    return [K] if K < 3 else [K // 2, K - K // 2 - 1, 1]


@pytest.mark.parametrize("B,K", [(5, 1), (5, 2), (5, 7), (5, 1024), (300, 3)])
def test_logmeanexp_kernels_vs_float64(gpu_device, B, K):
    g = torch.Generator().manual_seed(B * 10007 + K)
    tables = {"normal": torch.randn(K, B, generator=g) * 3.0 - 40.0,
              "spread": torch.randn(K, B, generator=g) * 300.0,                  # rows span far more than 200 nats
              "equal": torch.full((K, B), -7.5),
              "huge": torch.randn(K, B, generator=g).sign() * 1e30}
    for name, lw in tables.items():
        tag = "B=%d K=%d %s" % (B, K, name)
        if name == "huge":
            # +-1e30: the answer is the maximum minus log(K / count of maxima), finite; judged in float64 on the same table
            ev, ess, _ = lme_gpu(lw.cuda(), [K])
            d = lw.double()
            want = torch.logsumexp(d, 0) - math.log(K)
            assert torch.isfinite(ev).all() and torch.isfinite(ess).all(), tag
            np.testing.assert_allclose(ev.double().numpy(), want.numpy(), rtol=2 * EPS32, err_msg=tag)
            for chunks in (uneven(K),):
                ev2, _, _ = lme_gpu(lw.cuda(), chunks)
                np.testing.assert_allclose(ev2.double().numpy(), want.numpy(), rtol=2 * EPS32, err_msg=tag)
            continue
        one = lme_check(tag, lw, [K])
        lme_check(tag, lw, uneven(K))
        if name == "equal":
            assert torch.allclose(one[1], torch.full((B,), float(K)), rtol=1e-6), tag         # ESS = K
            assert torch.allclose(one[0], torch.full((B,), -7.5), rtol=0, atol=1e-6), tag
        if name == "spread" and K > 1:
            assert one[1].median().item() < 1.0 + 1e-3, tag                                    # ESS -> 1


def test_logmeanexp_first_ignores_the_state_and_runs_are_bit_identical(gpu_device):
    g = torch.Generator().manual_seed(3)
    lw = (torch.randn(7, 300, generator=g) * 5.0).cuda()
    runs = []
    for fill in (0.0, float("nan"), 0.0):
        st = torch.full((300, 4), fill, device="cuda")
        ev, ess, st = lme_gpu(lw, [3, 3, 1], st)
        runs.append((ev, ess, st[:, :3].cpu()))
    for a, b in ((runs[0], runs[1]), (runs[0], runs[2])):
        assert all(torch.equal(u, v) for u, v in zip(a, b))


# ------------------------------------------------------------------------------- 2. the evidence against the oracle
def gpu_evidence(eng, x, eps, y, b, chunks, z_dim):
    """eps (K*b, z_dim) rows [k][b] through engine.log_evidence_chunk in `chunks` -> (log p^, ESS) on the CPU."""
    K = eps.shape[0] // b
    e3 = eps.view(K, b, z_dim)
    st, k0 = None, 0
    xg, yg = x.cuda(), None if y is None else y.cuda()
    for i, P in enumerate(chunks):
        st = eng.log_evidence_chunk(xg, e3[k0:k0 + P].contiguous().cuda(), yg, st, first=(i == 0))
        k0 += P
    ev, ess = eng.log_evidence_finish(st, K, True)
    torch.cuda.synchronize()
    return ev.cpu(), ess.cpu()


reference_for = ek.reference_for


CELLS = [("8x8_rts_b6_p3", f) for f in (0, 2, 3)] + [(n, 2) for n in sorted(ek.CASES) if n not in ("8x8_rts_b6_p3",)]


@pytest.mark.parametrize("name,fused", CELLS)
def test_evidence_vs_oracle(gpu_device, categorical_oracle, name, fused):
    """Per image and ESS, one chunk and chunked (the same eps, K = 2 P + 1 particles as P + P + 1), and K = P in one chunk."""
    model, cfg, x, y, _, b, P = ek.make(name, "cuda")
    K = 2 * P + 1
    _, _, _, _, eps, _, _ = ek.make(name, "cpu", particles=K)
    eng = model.engine(fused=fused)
    if name == "16x16_r_b20_p3":
        # the fused launch's workgroup g owns units [g U / G, (g + 1) U / G): one of them must straddle a particle boundary
        for Pk in (P, K):
            U, per = Pk * b * cfg.n_pix // 16, b * cfg.n_pix // 16
            G = min(U, cus())
            assert eng.uses_fused(b) and any(g * U // G < k * per < (g + 1) * U // G for g in range(G) for k in range(1, Pk)), (U, G)
    ref, bar = reference_for(fused, model, cfg, x, eps, y, b, K)
    for chunks in ([K], [P, P, 1]):
        ev, ess = gpu_evidence(eng, x, eps, y, b, chunks, cfg.z_dim)
        ek.check("%s fused=%d chunks %s" % (name, fused, chunks), ev, ess, ref, bar)
        assert (ess >= 1 - 1e-5).all() and (ess <= K * (1 + 1e-5)).all()
        assert (ev.double() >= ref["lw"].mean(0) - bar * ref["ll_max"]).all()          # Jensen, against the oracle's lw
    refP, bar = reference_for(fused, model, cfg, x, eps[:P * b], y, b, P)
    ev, ess = gpu_evidence(eng, x, eps[:P * b], y, b, [P], cfg.z_dim)
    ek.check("%s fused=%d one chunk of P=%d" % (name, fused, P), ev, ess, refP, bar)


# ------------------------------------------------------------------------------- 3. identities
@pytest.mark.parametrize("fused", [0, 2, 3])
def test_one_particle_is_the_one_sample_elbo(gpu_device, fused):
    """K = 1: log p^(x_b) is the image's one-sample ELBO — against the oracle per image, and its sum is -loss of elbo_terms with
    the same eps (two forward paths of the same precision class: the project's loss bar between them); ESS = 1."""
    name = "8x8_rts_b6_p3"
    model, cfg, x, y, eps, b, _ = ek.make(name, "cuda", particles=1)
    eng = model.engine(fused=fused)
    ev, ess = gpu_evidence(eng, x, eps, y, b, [1], cfg.z_dim)
    ref, bar = reference_for(fused, model, cfg, x, eps, y, b, 1)
    ek.check("%s fused=%d K=1" % (name, fused), ev, ess, ref, bar)
    assert torch.equal(ess, torch.ones(b))
    loss = model.elbo_terms(x, eps=eps)["loss"]
    np.testing.assert_allclose(ev.double().sum().item(), -loss, rtol=RTOL_ELBO)


@pytest.mark.parametrize("name,fused", [("8x8_rts_b6_p3", 0), ("8x8_rts_b6_p3", 2), ("8x8_rts_b6_p3", 3), ("8x8_none_b6_p3", 0),
                                        ("8x8_none_b6_p3", 2), ("8x8_r_c3_poisson_b6_p3", 0), ("8x8_r_c3_poisson_b6_p3", 2)])
def test_one_chunk_is_the_renyi_forward(gpu_device, name, fused):
    """The same launches and the same device code for the log-weights: a one-chunk evidence summed over images equals
    -scalars[0] of the alpha = 0 forward-only call on the same eps.  The two form L_b in another order of fp32 operations (the
    Renyi call through normalised weights and their entropy, the evidence through m + log s): tests/_judge.py's bar for the
    same quantity summed two ways among the engine's own results, 2e-6."""
    model, cfg, x, y, eps, b, P = ek.make(name, "cuda")
    eng = model.engine(fused=fused)
    ev, _ = gpu_evidence(eng, x, eps, y, b, [P], cfg.z_dim)
    eng = model.engine(particles=P, renyi=0.0)
    eng.loss_and_grads(x.cuda(), eps.cuda(), 1.0, None if y is None else y.cuda(), want_grads=False)
    got = -eng.scalars[0].item()
    model.engine(particles=1, renyi=False)
    print("%s fused=%d: sum log p^ %.6f, -scalars[0] %.6f" % (name, fused, ev.double().sum().item(), got))
    np.testing.assert_allclose(ev.double().sum().item(), got, rtol=2e-6)


def test_permuting_the_images_permutes_the_output(gpu_device):
    name = "8x8_rts_b6_p3"
    model, cfg, x, y, eps, b, P = ek.make(name, "cuda")
    eng = model.engine(fused=2)
    ev, ess = gpu_evidence(eng, x, eps, y, b, [P], cfg.z_dim)
    perm = torch.tensor([3, 0, 5, 1, 4, 2])
    e3 = eps.view(P, b, cfg.z_dim)[:, perm].reshape(P * b, cfg.z_dim)
    ev2, ess2 = gpu_evidence(eng, x[perm], e3, y, b, [P], cfg.z_dim)
    # (an image's rows move to another workgroup's range of the fused launch: the same values to the fp32-class bar, not the same bits)
    ref = ek.reference(state(model), cfg, x, eps, y, P)
    assert (ev2.double() - ev[perm].double()).abs().max().item() <= 2 * RTOL_ELBO * ref["ll_max"]
    np.testing.assert_allclose(ess2.numpy(), ess[perm].numpy(), rtol=8 * RTOL_ELBO * ref["ll_max"])
    eng0 = model.engine(fused=0)
    a = gpu_evidence(eng0, x, eps, y, b, [P], cfg.z_dim)
    b_ = gpu_evidence(eng0, x, eps, y, b, [P], cfg.z_dim)
    assert torch.equal(a[0], b_[0]) and torch.equal(a[1], b_[1])                  # a run is bit-reproducible


def test_kl_mode_and_beta(gpu_device):
    """An engine trained with the analytic KL evaluates the same evidence (the mode is not consulted), bit for bit."""
    name = "8x8_rts_b6_p3"
    model, cfg, x, y, eps, b, P = ek.make(name, "cuda")
    a = gpu_evidence(model.engine(fused=2, kl="sampled"), x, eps, y, b, [P], cfg.z_dim)
    c = gpu_evidence(model.engine(fused=2, kl="analytic"), x, eps, y, b, [P], cfg.z_dim)
    assert torch.equal(a[0], c[0]) and torch.equal(a[1], c[1])


# ------------------------------------------------------------------------------- 4. the public API
def test_model_and_trainer_log_evidence(gpu_device):
    """n = 10 images in batches of 4, 5 samples in chunks of 2, explicit eps (num_samples, n, z_dim), against the oracle per
    batch; SVItrainer.log_evidence(loader) is its mean; without eps the documented draw order reproduces it."""
    data_dim, inv, n, K = (8, 8), ["r", "t", "s"], 10, 5
    g = torch.Generator().manual_seed(2)
    x = torch.rand(n, *data_dim, generator=g)
    model = pv.models.iVAE(data_dim, 2, inv, seed=1, device="cuda")
    eps = torch.randn(K, n, model.z_dim, generator=g)
    cfg = orc.Config(data_dim=data_dim, latent_dim=2, invariances=inv)
    ev, ess = model.log_evidence(x, num_samples=K, chunk=2, eps=eps, return_ess=True, batch_size=4)
    assert ev.shape == (n,) and ess.shape == (n,) and ev.dtype == torch.float32 and not ev.is_cuda
    ref = ek.reference(state(model), cfg, x, eps.reshape(K * n, -1), None, K)
    ek.check("model.log_evidence", ev, ess, ref, RTOL_ELBO)
    assert torch.equal(model.log_evidence(x, num_samples=K, chunk=2, eps=eps, batch_size=4), ev)
    # drawn eps: batches outer, chunks inner
    torch.manual_seed(9)
    drawn = model.log_evidence(x, num_samples=K, chunk=2, batch_size=4)
    torch.manual_seed(9)
    e2 = torch.empty(K, n, model.z_dim)
    for lo, hi in ((0, 4), (4, 8), (8, 10)):
        for k0, k1 in ((0, 2), (2, 4), (4, 5)):
            e2[k0:k1, lo:hi] = torch.empty(k1 - k0, hi - lo, model.z_dim).normal_()
    assert torch.equal(drawn, model.log_evidence(x, num_samples=K, chunk=2, eps=e2, batch_size=4))
    # the trainer: the mean over the loader's images, here with the loader's batches as the image batches
    tr = pv.trainers.SVItrainer(model, seed=1)
    loader = pv.utils.init_dataloader(x, batch_size=4, shuffle=False)
    torch.manual_seed(9)
    got = tr.log_evidence(loader, num_samples=K, chunk=2)
    torch.manual_seed(9)
    per = torch.cat([model.log_evidence(xb[0], num_samples=K, chunk=2) for xb in loader])
    np.testing.assert_allclose(got, per.double().mean().item(), rtol=1e-12)
    assert abs(got - ref["log_ev"].mean().item()) < 5.0                            # (other eps: the same quantity, not the same draw)


def test_fused_channels_engine_evaluates_on_the_layered_plan(gpu_device):
    import _multichannel_cases as mc
    c = mc.CASES["c01_8x8_rts_c2_b6"]
    x, y, eps = mc.case_data(c, particles=3)
    model = pv.models.iVAE(c["dims"], 2, c["inv"], seed=1, device="cuda", **mc.model_kwargs(c))
    cfg = mc.case_config(c)
    eng = model.engine(fused=2, fused_channels=True)
    assert eng._plan_fused() == 1
    ev, ess = gpu_evidence(eng, x, eps[0], y, c["b"], [3], cfg.z_dim)
    ref = ek.reference(state(model), cfg, x, eps[0], y, 3)
    ek.check("fused_channels", ev, ess, ref, RTOL_ELBO)
    lay = gpu_evidence(model.engine(fused=0, fused_channels=False), x, eps[0], y, c["b"], [3], cfg.z_dim)
    assert torch.equal(lay[0], ev) and torch.equal(lay[1], ess)
    one = pv.models.iVAE((8, 8), 2, ["r"], seed=1, device="cuda")
    x1 = torch.rand(6, 8, 8)
    e1 = torch.randn(3, 6, one.z_dim)
    one.engine(fused=1)                                   # the one-channel f32 kernel has no several-particle form either
    on_fused1 = one.log_evidence(x1, num_samples=3, eps=e1)
    one.engine(fused=0)
    assert torch.equal(on_fused1, one.log_evidence(x1, num_samples=3, eps=e1))


def test_weighted_engine_raises(gpu_device):
    model = pv.models.iVAE((8, 8), 2, ["r"], seed=1, device="cuda")
    model.engine(image_weights=True)
    with pytest.raises(ValueError, match="no kernel applies observation weights to several particles"):
        model.log_evidence(torch.rand(4, 8, 8), num_samples=3)
    with pytest.raises(ValueError, match="no kernel applies observation weights"):
        model.engine().log_evidence_chunk(torch.rand(4, 8, 8).cuda(), torch.randn(3 * 4, model.z_dim).cuda())
