"""
Held-out log-evidence where no GPU is needed: the four new entry points in the C ABI (symbols, the unchanged v17, the evidence
query's scope and refusals, refusals of the call before a pointer is touched), the chunked estimator restated in float64
(tests/_evidence_kit.py) against the frozen oracle's bound_per_image and weights, and the host logic of iVAE.log_evidence on
CPU models: its ValueErrors, the default chunk and the order of the eps draws.
Plans are tests/_plan_kit.py's (784 positions x ch observations, batch 16) in the style of tests/test_objective_cpu.py.
"""
import ctypes as C
import os
import re

import pytest
import torch

from conftest import ROOT

import pyroved_amd as pv
from pyroved_amd import _abi
from oracle import svi_oracle as orc
from _plan_kit import PLAN_FIELDS, CASES as PLAN_CASES, _plan, _small_plan, _vanilla_plan, _params, _inputs
from _categorical_cases import categorical_oracle          # noqa: F401  (fixture)
import _evidence_kit as ek
from test_objective_cpu import _conv_plan, _dy_plan, _with, HOST

EINVAL = -1


# ------------------------------------------------------------------------------- 1. ABI
def test_symbols_header_and_unchanged_abi():
    src = open(os.path.join(ROOT, "include", "pyroved_amd.h")).read()
    lib = _abi.lib()
    for decl in ("int pv_logmeanexp_update(const float* lw /* (P, B) */, int32_t P, int32_t B, float* state, int first, void* stream);",
                 "int64_t pv_ivae_evidence_workspace_bytes(const pv_ivae_plan* plan, int32_t P);",
                 "int pv_ivae_evidence_accumulate(const pv_ivae_plan* plan, int32_t P, float* state, int first, void* stream);"):
        assert decl in src, decl
    assert re.search(r"int pv_logmeanexp_finish\(const float\* state, int32_t B, int64_t K_total, float\* log_mean", src)
    for name in ("pv_logmeanexp_update", "pv_logmeanexp_finish", "pv_ivae_evidence_workspace_bytes", "pv_ivae_evidence_accumulate"):
        assert name in _abi.SIGNATURES and getattr(lib, name) is not None
    assert _abi.PV_ABI_VERSION == 17 and lib.pv_version() == 17
    assert C.sizeof(_abi.pv_ivae_plan) == 2824 and [f[0] for f in _abi.pv_ivae_plan._fields_] == PLAN_FIELDS
    assert C.sizeof(_abi.pv_ivae_objective) == 32


def in_scope():
    out = {}
    for fused in (0, 2, 3):
        for ch in (1, 3):
            out["fused%d-ch%d" % (fused, ch)] = _plan(fused, ch)
        out["fused%d-analytic" % fused] = _with(_plan(fused, 1), kl_mode=_abi.KL["analytic"])     # (the mode is not consulted)
        out["fused%d-poisson" % fused] = _with(_plan(fused, 1), lik=_abi.LIK["poisson_log"], sigmoid_out=0)
    for fused in (0, 2):
        out["vanilla-fused%d" % fused] = _vanilla_plan(fused)
    cat = _with(_plan(0, 3), lik=_abi.PV_LIK_CATEGORICAL, sigmoid_out=0)
    out["categorical"] = cat
    cd = _plan(0, 1)
    cd.c_dim, cd.fc_latent.in_dim = 3, 5
    cd.enc[0].in_dim += 3
    out["c_dim"] = cd
    return out


def out_of_scope():
    out = {"jivae": _small_plan(discrete_dim=3, fused=0), "conv": _conv_plan(), "ext_encoder": _with(_plan(0, 1), ext_encoder=1),
           "ext_decoder": _with(_plan(0, 1), ext_decoder=1), "dy": _dy_plan()}
    for field in ("row_w", "row_elbo", "class_onehot"):
        out[field] = _with(_plan(0, 1), **{field: HOST})
    for ch in (1, 3):
        out["fused1-ch%d" % ch] = _plan(1, ch)
        out["fused1-ch%d+channels" % ch] = _with(_plan(1, ch), flags=_abi.PV_PLAN_FUSED_CHANNELS)
    return out


def test_evidence_query_scope():
    L = _abi.lib()
    for name, p in out_of_scope().items():
        for P in (1, 3):
            assert L.pv_ivae_evidence_workspace_bytes(C.byref(p), P) == EINVAL, (name, P)
    for name, p in in_scope().items():
        sizes = [L.pv_ivae_evidence_workspace_bytes(C.byref(p), P) for P in (1, 2, 16, 1024)]
        assert all(s > 0 for s in sizes) and sizes == sorted(set(sizes)), (name, sizes)           # > 0 and growing with P
        for P in (0, -1, 1025):
            assert L.pv_ivae_evidence_workspace_bytes(C.byref(p), P) == EINVAL, (name, P)
        # forward only: below the training layout of the same particle count (no gradient buffers on the layered kernels)
        if p.fused == 0 or name.startswith("vanilla") or "-ch3" in name:
            assert sizes[2] < L.pv_ivae_particles_workspace_bytes(C.byref(p), 16), name
    assert L.pv_ivae_evidence_workspace_bytes(None, 3) == EINVAL


def test_call_is_refused_before_a_pointer_is_touched():
    """No buffers, a NULL state, a plan out of scope or a particle count out of range: PV_EINVAL, with host addresses standing in
    for the device pointers a refused call must not read."""
    L = _abi.lib()
    for name, p in in_scope().items():
        assert L.pv_ivae_evidence_accumulate(C.byref(p), 3, HOST, 1, None) == EINVAL, name            # no buffers
        q = _with(p, params=HOST, x=HOST, eps=HOST, ws=HOST, ws_bytes=1 << 40, grid=HOST, y=HOST)
        assert L.pv_ivae_evidence_accumulate(C.byref(q), 3, None, 1, None) == EINVAL, name            # NULL state
        for P in (0, 1025):
            assert L.pv_ivae_evidence_accumulate(C.byref(q), P, HOST, 1, None) == EINVAL, (name, P)
        q.ws_bytes = 16
        assert L.pv_ivae_evidence_accumulate(C.byref(q), 3, HOST, 1, None) == -2, name                # PV_EWS
    for name, p in out_of_scope().items():
        q = _with(p, params=HOST, x=HOST, eps=HOST, ws=HOST, ws_bytes=1 << 40, grid=HOST)
        assert L.pv_ivae_evidence_accumulate(C.byref(q), 3, HOST, 1, None) == EINVAL, name
    assert L.pv_logmeanexp_update(None, 3, 5, HOST, 1, None) == EINVAL and L.pv_logmeanexp_update(HOST, 3, 5, None, 1, None) == EINVAL
    assert L.pv_logmeanexp_update(HOST, 0, 5, HOST, 1, None) == EINVAL and L.pv_logmeanexp_update(HOST, 3, 0, HOST, 1, None) == EINVAL
    assert L.pv_logmeanexp_finish(None, 5, 3, HOST, None, None) == EINVAL and L.pv_logmeanexp_finish(HOST, 5, 3, None, None, None) == EINVAL
    assert L.pv_logmeanexp_finish(HOST, 5, 0, HOST, None, None) == EINVAL and L.pv_logmeanexp_finish(HOST, 0, 3, HOST, None, None) == EINVAL


# ------------------------------------------------------------------------------- 2. the estimator
@pytest.mark.parametrize("case", range(len(PLAN_CASES)))
def test_chunked_estimator_equals_the_oracle(case):
    """One chunk, uneven chunks (7 = 3 + 3 + 1) and K = 1, in float64: the restated running state gives the oracle's
    bound_per_image and 1 / sum w^2 to rounding."""
    data_dim, inv, c_dim = PLAN_CASES[case]
    cfg = orc.Config(data_dim=data_dim, latent_dim=2, invariances=inv, c_dim=c_dim)
    params = _params(cfg, c_dim=c_dim)
    b, K = 5, 7
    x, eps, y = _inputs(cfg, b, K, c_dim=c_dim)
    ref = ek.reference(params, cfg, x, eps, y, K)
    for chunks in ([7], [3, 3, 1], [1] * 7, [1, 6]):
        ev, ess = ek.chunked_log_mean_exp(ref["lw"], chunks)
        assert torch.allclose(ev, ref["log_ev"], rtol=1e-13, atol=1e-11), chunks
        assert torch.allclose(ess, ref["ess"], rtol=1e-11), chunks
        assert (ess >= 1 - 1e-12).all() and (ess <= K + 1e-12).all()
    assert (ref["log_ev"] >= ref["lw"].mean(0) - 1e-12).all()                  # Jensen
    x1, eps1, y1 = _inputs(cfg, b, 1, c_dim=c_dim)
    one = ek.reference(params, cfg, x1, eps1, y1, 1)
    ev, ess = ek.chunked_log_mean_exp(one["lw"], [1])
    assert torch.equal(ev, one["lw"][0]) and torch.equal(ess, torch.ones(b, dtype=torch.float64))
    # ... which is the one-sample ELBO per image: its sum is -loss of the plain objective on the same eps
    with torch.no_grad():
        plain = orc.elbo(params, cfg, x1, eps1, 1.0, y1)
    assert abs(ev.sum().item() + plain["loss"].item()) <= 1e-10 * abs(plain["loss"].item())


def test_estimator_survives_spread_and_large_values():
    g = torch.Generator().manual_seed(5)
    lw = torch.randn(7, 4, generator=g, dtype=torch.float64) * 300.0           # rows span far more than 200 nats: ESS -> 1
    ev, ess = ek.chunked_log_mean_exp(lw, [3, 3, 1])
    assert torch.allclose(ev, torch.logsumexp(lw, 0) - torch.log(torch.tensor(7.0, dtype=torch.float64)), rtol=1e-13)
    assert (ess < 1.0 + 1e-6).all()
    ev, ess = ek.chunked_log_mean_exp(torch.full((7, 4), -3.25, dtype=torch.float64), [3, 3, 1])
    assert torch.allclose(ev, torch.full((4,), -3.25, dtype=torch.float64)) and torch.allclose(ess, torch.full((4,), 7.0, dtype=torch.float64))


# ------------------------------------------------------------------------------- 3. host logic on CPU models
def model(**kw):
    return pv.models.iVAE((8, 8), 2, ["r", "t", "s"], seed=1, device="cpu", **kw)


def test_value_errors(monkeypatch):
    from pyroved_amd.engine import IVAEEngine
    monkeypatch.setattr(IVAEEngine, "bind", lambda self: None)         # engines here never reach the device
    m = model()
    x = torch.rand(10, 8, 8)
    with pytest.raises(ValueError, match="num_samples must be >= 1"):
        m.log_evidence(x, num_samples=0)
    with pytest.raises(ValueError, match=r"eps must have shape \(num_samples, n, z_dim\) = \(5, 10, 6\)"):
        m.log_evidence(x, num_samples=5, eps=torch.zeros(5 * 10, 6))
    with pytest.raises(ValueError, match="eps must have shape"):
        m.log_evidence(x, num_samples=5, eps=torch.zeros(5, 10, 5))
    with pytest.raises(ValueError, match="chunk must be in 1 .. 1024"):
        m.log_evidence(x, num_samples=5, chunk=0)
    with pytest.raises(ValueError, match="chunk must be in 1 .. 1024"):
        m.log_evidence(x, num_samples=5000, chunk=1025)
    with pytest.raises(ValueError, match=r"class-conditioned model \(c_dim=3\) needs y"):
        model(c_dim=3).log_evidence(x, num_samples=5)
    for kw, word in ((dict(image_weights=True), "image_weights"), (dict(pixel_weights=torch.ones(8, 8)), "pixel_weights")):
        mw = model()
        mw.engine(**kw)
        with pytest.raises(ValueError, match="configured with %s, and no kernel applies observation weights to several" % word):
            mw.log_evidence(x, num_samples=5)
    for other in (pv.models.jiVAE((8, 8), 2, 3, ["r"], seed=1, device="cpu"), pv.models.VED((8, 8), (8, 8), seed=1, device="cpu"),
                  pv.models.ssiVAE((8, 8), 2, 3, ["r"], seed=1, device="cpu")):
        assert not hasattr(other, "log_evidence"), type(other).__name__


def test_default_chunk_arithmetic():
    """The largest P <= min(num_samples, 1024) with P * batch * positions <= 2^19 rows, at least 1; positions are the spatial
    decoder's grid points and 1 for the vanilla decoder."""
    f = pv.models.iVAE._evidence_chunk
    assert pv.models.iVAE.LOG_EVIDENCE_ROW_CAP == 1 << 19
    assert f(64, 100, 784) == 6 and 6 * 100 * 784 <= 1 << 19 < 7 * 100 * 784
    assert f(5000, 256, 784) == 2 and f(1, 256, 784) == 1 and f(5000, 4, 64) == 1024 and f(5000, 6, 1) == 1024 and f(9, 8, 64) == 9
    assert f(64, 100, 1 << 20) == 1 and f(1, 1, 1) == 1
    assert model()._evidence_positions() == 64 and pv.models.iVAE((8, 8), 2, None, seed=1, device="cpu")._evidence_positions() == 1
    assert pv.models.iVAE((16,), 2, ["t"], channels=3, seed=1, device="cpu")._evidence_positions() == 16


def test_eps_draw_order_and_schedule():
    """Image batches outer, chunks inner, one torch.empty(P, b, z_dim).normal_() on the CPU generator per call; the last batch and
    the last chunk may be smaller; given eps is sliced, not drawn."""
    m = model()
    n, K, chunk, bs = 10, 5, 2, 4
    torch.manual_seed(11)
    got = list(m._evidence_schedule(n, K, chunk, bs, None))
    after = torch.empty(3).normal_()
    torch.manual_seed(11)
    want = []
    for lo, hi in ((0, 4), (4, 8), (8, 10)):
        for k0, k1 in ((0, 2), (2, 4), (4, 5)):
            want.append((lo, hi, k0 == 0, torch.empty(k1 - k0, hi - lo, m.z_dim).normal_()))
    assert torch.equal(after, torch.empty(3).normal_())                        # nothing else is drawn
    assert [(g[0], g[1], g[2]) for g in got] == [(w[0], w[1], w[2]) for w in want]
    assert all(torch.equal(g[3], w[3]) for g, w in zip(got, want))
    eps = torch.randn(K, n, m.z_dim)
    st = torch.get_rng_state()
    given = list(m._evidence_schedule(n, K, chunk, bs, eps))
    assert torch.equal(st, torch.get_rng_state())
    assert torch.equal(torch.cat([torch.cat([g[3] for g in given if g[0] == lo], 0) for lo in (0, 4, 8)], 1), eps)
    # chunk=None: the default per batch
    assert [g[3].shape[0] for g in m._evidence_schedule(3, 5, None, 100, None)] == [5]
