"""
_evidence_kit.py — what the held-out log-evidence tests share (tests/test_log_evidence_cpu.py, tests/test_gpu_log_evidence.py,
tests/test_gpu_log_evidence_workspace.py): the float64 reference, a pure-torch restatement of the chunked estimator, the case
table and the bars.

The reference is the frozen oracle: orc.elbo(..., beta=1, particles=K, renyi=0.0) in float64 — its bound_per_image IS
log p^(x_b) = logsumexp_k lw_kb - log K and 1 / sum_k w_kb^2 its effective sample size; with one particle the oracle has no
bound per image, and log p^(x_b) is the one log-weight, formed here from the oracle's own z_loc / z_scale / z / ll_per_sample.

The bars are the project's (tests/_judge.py, tests/_bf16_judge.py), composed as tests/test_gpu_renyi.py composes them for the
weights.  ll_bar is the relative bar on a log-likelihood: RTOL_ELBO = 2e-5 against float64 for fused 0 / 2, LOSS_CEIL = 1e-5
against the reference that rounds where the kernel does for fused 3.  Every lw inherits it, |d lw| <= ll_bar max_s |ll_s| = D.
  log p^(x_b)  is a log-mean-exp: its derivative in the lw is a convex combination, so |d log p^| <= D.
  ESS_b        = 1 / sum_k w_k^2 with log w_k = lw_k - logsumexp: |d log w| <= 2 D and |d log ESS| <= 2 max |d log w| = 4 D.
Helper modules are not assertion-rewritten: every bare assert carries its tag, value and bar.
"""
import math

import torch

import pyroved_amd as pv
from oracle import svi_oracle as orc
import _multichannel_cases as mc
import _categorical_cases as cc
import _poisson_data as pd
from oracle import bf16_plan as bp
from _bf16_judge import LOSS_CEIL
from _judge import RTOL_ELBO, state

LOG_SQRT_2PI = 0.5 * math.log(2.0 * math.pi)


# ------------------------------------------------------------------------------- the estimator, restated
def chunked_log_mean_exp(lw, chunks):
    """lw (K, B) float64, chunks: sizes summing to K.  The running state per image {m, s, q} exactly as include/pyroved_amd.h
    states it — a chunk's maximum joins m, s is rescaled by e^(m_old - m_new) and q by its square, then the chunk's terms are
    added in ascending p.  Returns (log p^ (B), ESS (B))."""
    K = lw.shape[0]
    assert sum(chunks) == K and all(c >= 1 for c in chunks)
    m = s = q = None
    k0 = 0
    for i, P in enumerate(chunks):
        c = lw[k0:k0 + P]
        k0 += P
        cm = c.max(0).values
        if i == 0:
            m, s, q = cm, torch.zeros_like(cm), torch.zeros_like(cm)
        else:
            mn = torch.maximum(m, cm)
            r = torch.exp(m - mn)
            m, s, q = mn, s * r, q * r * r
        for p in range(P):
            e = torch.exp(c[p] - m)
            s, q = s + e, q + e * e
    return m + torch.log(s) - math.log(K), s * s / q


# ------------------------------------------------------------------------------- the reference
def reference(params, cfg, x, eps, y, K):
    """float64: dict(log_ev (B), ess (B), lw (K, B), ll_max = max_s |ll_s|, out = the oracle's dictionary).  eps (K*B, z_dim),
    rows [k][b]."""
    b = x.shape[0]
    o = orc.SVIOracle(params, cfg, dtype=torch.float64, particles=K, renyi=0.0)
    with torch.no_grad():
        out = o.loss_and_grads(x, eps, 1.0, y)
    zl, zs, z = out["z_loc"].repeat(K, 1), out["z_scale"].repeat(K, 1), out["z"]
    logq = (-((z - zl) ** 2) / (2 * zs ** 2) - torch.log(zs) - LOG_SQRT_2PI).sum(-1)
    logp = (-(z ** 2) / 2 - LOG_SQRT_2PI).sum(-1)
    lw = (out["ll_per_sample"] + logp - logq).view(K, b)
    if K > 1:
        log_ev = out["bound_per_image"]
        ess = 1.0 / (out["weights"].view(K, b) ** 2).sum(0)
        assert torch.allclose(log_ev, torch.logsumexp(lw, 0) - math.log(K), rtol=1e-12, atol=1e-9), "the kit's lw is not the oracle's"
    else:
        log_ev, ess = lw[0], torch.ones(b, dtype=torch.float64)
    return dict(log_ev=log_ev.detach(), ess=ess.detach(), lw=lw.detach(), ll_max=out["ll_per_sample"].abs().max().item(), out=out)


def reference_for(fused, model, cfg, x, eps, y, b, K):
    """(reference, ll_bar): float64 for fused 0 / 2; for fused 3 on the fused kernels the reference that rounds where the 4-wave or
    8-wave bf16 kernel does, at the bf16 judge's loss ceiling."""
    if fused == 3 and model.engine().uses_fused(b) and cfg.channels == 1:
        import dataclasses
        from _device import cus as _cus, kernel_name as _kernel_name
        units = K * b * cfg.n_pix // 16
        kern = "w8" if "pv_sdec_w8_kernel" in _kernel_name(fused=3, units=units, lik=0) else "w4"
        c = dataclasses.replace(cfg, bf16_plan=bp.Bf16Plan(kernel=kern, cus=_cus()))
        return reference(state(model), c, x, eps, y, K), LOSS_CEIL
    return reference(state(model), cfg, x, eps, y, K), RTOL_ELBO


def check(tag, got_ev, got_ess, ref, ll_bar):
    """The two bars of the module docstring, figures printed first."""
    D = ll_bar * ref["ll_max"]
    err = (got_ev.double().cpu() - ref["log_ev"]).abs().max().item()
    lerr = (torch.log(got_ess.double().cpu()) - torch.log(ref["ess"])).abs().max().item()
    print("%s: max |log p^ - ref| %.3e (bar %.3e), max |log ESS - log ref| %.3e (bar %.3e), ESS in [%.3f, %.3f]"
          % (tag, err, D, lerr, 4 * D, got_ess.min().item(), got_ess.max().item()))
    assert torch.isfinite(got_ev).all() and torch.isfinite(got_ess).all(), "%s: non-finite evidence or ESS" % tag
    assert err <= D, "%s: log p^ %.3e from the reference (bar %.3e)" % (tag, err, D)
    assert lerr <= 4 * D, "%s: log ESS %.3e from the reference (bar %.3e)" % (tag, lerr, 4 * D)


# ------------------------------------------------------------------------------- cases: the smallest shapes that reach each path
# name: dict(kind, ...) -> make(name, device) below; b images, P particles per chunk of the one-chunk run
CASES = {
    "8x8_rts_b6_p3": dict(dims=(8, 8), inv=["r", "t", "s"], b=6, P=3),                                     # the three forward kernels
    "1d32_t_gauss_nosig_b5_p4": dict(dims=(32,), inv=["t"], b=5, P=4, kw=dict(sampler_d="gaussian", sigmoid_d=False)),
    "8x8_r_c3_poisson_b6_p3": dict(dims=(8, 8), inv=["r"], b=6, P=3, mc=dict(C=3, sampler="poisson_log", sigmoid_d=False)),
    "8x8_rt_c3_categorical_b6_p2": dict(dims=(8, 8), inv=["r", "t"], b=6, P=2, mc=dict(C=3, **cc.KIND)),
    "8x8_rt_cdim3_b6_p3": dict(dims=(8, 8), inv=["r", "t"], b=6, P=3, kw=dict(c_dim=3)),
    "8x8_none_b6_p3": dict(dims=(8, 8), inv=None, b=6, P=3),                                               # vanilla decoder
    "8x8_rts_gauss_sig002_b6_p3": dict(dims=(8, 8), inv=["r", "t", "s"], b=6, P=3,
                                       kw=dict(sampler_d="gaussian", decoder_sig=0.02)),                   # lw thousands of nats apart
    "16x16_r_b20_p3": dict(dims=(16, 16), inv=["r"], b=20, P=3),                                           # 960 units on 256 workgroups
}


def make(name, device, particles=None):
    """(model, cfg, x, y, eps (P*b, z_dim) rows [p][b], b, P) of a case; data and eps from torch.Generator().manual_seed(0), the
    data first (the multi-channel kits' order)."""
    c = CASES[name]
    b, P = c["b"], c["P"] if particles is None else particles
    if "mc" in c:
        m = dict(dims=c["dims"], inv=c["inv"], b=b, **c["mc"])
        model = pv.models.iVAE(m["dims"], 2, m["inv"], seed=1, device=device, **mc.model_kwargs(m))
        cfg = mc.case_config(m)
        if m.get("sampler") == "poisson_log":            # counts from tests/_poisson_data.py, one draw per channel, channel-last
            g = torch.Generator().manual_seed(0)
            x = torch.stack([pd.counts(g, b, m["dims"]) for _ in range(m["C"])], -1)
            return model, cfg, x, None, torch.randn(P * b, cfg.z_dim, generator=g), b, P
        x, y, eps = cc.case_data(m, particles=P)
        return model, cfg, x, y, eps[0], b, P
    kw = c.get("kw", {})
    model = pv.models.iVAE(c["dims"], 2, c["inv"], seed=1, device=device, **kw)
    cfg = orc.Config(data_dim=tuple(c["dims"]), latent_dim=2, invariances=c["inv"], c_dim=kw.get("c_dim", 0),
                     sampler=kw.get("sampler_d", "bernoulli"), sigmoid_d=kw.get("sigmoid_d", True),
                     **({"decoder_sig": kw["decoder_sig"]} if "decoder_sig" in kw else {}))
    g = torch.Generator().manual_seed(0)
    x = torch.rand(b, *c["dims"], generator=g)
    eps = torch.randn(P * b, cfg.z_dim, generator=g)
    y = None
    if cfg.c_dim:
        y = torch.zeros(b, cfg.c_dim)
        y[torch.arange(b), torch.arange(b) % cfg.c_dim] = 1.0
        x = x.flatten(1)
    return model, cfg, x, y, eps, b, P

