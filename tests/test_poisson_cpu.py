"""
The Poisson (log link) likelihood — sampler_d="poisson_log", PV_LIK_POISSON_LOG — where no GPU is needed: the reference
(oracle.svi_oracle.likelihood, the formulas of tests/_poisson_data.py) against torch.distributions.Poisson and autograd, the sampler and the ABI constants, plan validation
through the library's workspace queries (host arithmetic), what the engines refuse at construction, and the condition the GPU
step tests' parameter check rests on (near-zero gradient entries below 1 % per tensor, with the reference alone).
"""
import ctypes as C
import os
import re

import pytest
import torch
import torch.distributions as td

from conftest import ROOT

import pyroved_amd as pv
from pyroved_amd import _abi
from pyroved_amd.engine import UnsupportedModel
from oracle import svi_oracle as orc
import _poisson_data as pr
from _judge import ILL_SHARE, near_zero_share
from _plan_kit import PLAN_FIELDS, _small_plan


# ------------------------------------------------------------------------------- the reference
def test_formula_and_gradient_equal_torch_poisson_in_float64():
    g = torch.Generator().manual_seed(0)
    a = (2.0 * torch.randn(64, generator=g, dtype=torch.float64)).requires_grad_(True)
    with torch.no_grad():
        a[0], a[1], a[2] = 31.5, 30.0, 29.999                       # above, at and just below the clamp
    x = torch.poisson(torch.full((64,), 3.0, dtype=torch.float64), generator=g)
    x[3], x[4] = 0.0, 2.5                                           # zero counts and non-integers are legal
    lp = td.Poisson(torch.exp(a.clamp(max=30)), validate_args=False).log_prob(x)
    torch.testing.assert_close(pr.log_prob_formula(a.detach(), x), lp.detach(), rtol=1e-13, atol=1e-13)
    (-lp.sum()).backward()
    torch.testing.assert_close(pr.dnll_da_formula(a.detach(), x), a.grad, rtol=1e-13, atol=1e-13)
    assert a.grad[0].item() == 0.0 and a.grad[1].item() != 0.0      # the clamp's gradient: nothing above 30, everything at it
    # the oracle's likelihood is that distribution; every other sampler is what it was, and an unknown one is no sampler
    cfg = orc.Config(data_dim=(8, 8), latent_dim=2, invariances=["r"], sampler="poisson_log", sigmoid_d=False)
    assert orc.POISSON_CLAMP == pr.CLAMP == 30.0
    torch.testing.assert_close(orc.likelihood(cfg, a.detach()).log_prob(x), lp.detach(), rtol=0, atol=0)
    bern = orc.likelihood(orc.Config(data_dim=(8, 8), latent_dim=2, invariances=["r"]), torch.sigmoid(a.detach()))
    assert isinstance(bern, td.Bernoulli)
    with pytest.raises(KeyError):
        orc.likelihood(orc.Config(data_dim=(8, 8), latent_dim=2, invariances=["r"], sampler="poisson"), a.detach())


def test_counts_recipe():
    """x.max() of 7 - 10 and no pixel that is zero in every image, at the GPU tests' shapes."""
    for dims, b in (((8, 8), 6), ((16,), 5), ((16, 16), 4), ((12, 20), 6), ((28, 28), 16)):
        x = pr.counts(torch.Generator().manual_seed(0), b, dims)
        assert x.shape == (b,) + dims and (x >= 0).all() and (x == x.round()).all()
        assert 5 <= x.max().item() <= 12, (dims, x.max().item())
        assert (x.sum(0) > 0).all(), dims
        r = pr.rates(torch.zeros(1, len(dims)), dims)
        assert r.min().item() >= 1.0 and r.max().item() <= 3.0


# ------------------------------------------------------------------------------- sampler and constants
def test_sampler_names():
    s = pv.utils.get_sampler("poisson_log")
    a = torch.tensor([-1.0, 0.5, 40.0])
    d = s(a)
    assert isinstance(d, td.Poisson) and s.name == "poisson_log"
    torch.testing.assert_close(d.rate, torch.exp(a.clamp(max=30)))
    assert d.log_prob(torch.tensor([0.5, 2.0, 1.0])).isfinite().all()           # validate_args=False: non-integers are legal
    with pytest.raises(KeyError):
        pv.utils.get_sampler("poisson")
    for name in ("bernoulli", "continuous_bernoulli", "gaussian"):
        assert pv.utils.get_sampler(name).name == name


def test_abi_constants_and_unchanged_structs():
    lib = _abi.lib()
    assert _abi.PV_ABI_VERSION == 17 and lib.pv_version() == 17
    src = open(os.path.join(ROOT, "include", "pyroved_amd.h")).read()
    m = re.search(r"PV_LIK_POISSON_LOG\s*=\s*(\d+)", src)
    assert m and int(m.group(1)) == 3 == _abi.LIK["poisson_log"]
    assert _abi.LIK == {"bernoulli": 0, "gaussian": 1, "continuous_bernoulli": 2, "poisson_log": 3}
    # the plan structs as they were (bytes on x86-64) and the field list tests/_plan_kit.py pins
    assert [f[0] for f in _abi.pv_ivae_plan._fields_] == PLAN_FIELDS
    assert C.sizeof(_abi.pv_ivae_plan) == 2824 and C.sizeof(_abi.pv_ved_plan) == 3880 and C.sizeof(_abi.pv_layer) == 32


# ------------------------------------------------------------------------------- plan validation (host arithmetic)
def _ivae_plan(fused, lik=3, sigmoid_out=0):
    p = _small_plan(fused=fused)
    p.lik, p.sigmoid_out = lik, sigmoid_out
    return p


def _ved_plan(lik=3, sigmoid_out=0):
    """Conv1d(1 -> 4, k 3) encoder on 16 points; latent_to_features 2 -> 4 x 16; Conv1d(4 -> 4, k 3), Conv1d(4 -> 1, k 1)."""
    v = _abi.pv_ved_plan()
    v.batch, v.ndim_in, v.ndim_out = 4, 1, 1
    v.in_dim[0], v.out_dim[0] = 16, 16
    v.in_ch, v.out_ch, v.z_dim = 1, 1, 2
    v.lik, v.sigmoid_out = lik, sigmoid_out

    def op(cin, cout, k, act, w, b):
        o = _abi.pv_op()
        o.kind, o.cin, o.cout, o.ksize, o.act, o.w_off, o.b_off = _abi.OP["conv"], cin, cout, k, _abi.ACT[act], w, b
        return o

    def layer(i, o, w, b):
        l = _abi.pv_layer()
        l.in_dim, l.out_dim, l.act, l.w_off, l.b_off = i, o, 0, w, b
        return l
    v.n_enc_ops = 1
    v.enc[0] = op(1, 4, 3, "lrelu", 0, 12)
    v.n_dec_ops = 2
    v.dec[0], v.dec[1] = op(4, 4, 3, "lrelu", 16, 64), op(4, 1, 1, None, 68, 72)
    v.head, v.l2f = layer(64, 4, 80, 336), layer(2, 64, 340, 468)
    v.dec_c0 = 4
    v.dec_dim0[0] = 16
    return v


def test_plan_validation_through_the_workspace_queries():
    lib = _abi.lib()
    EINVAL = -1
    for fused in (0, 1, 2, 3):
        p = _ivae_plan(fused)
        assert lib.pv_ivae_workspace_bytes(C.byref(p)) > 0, fused
        assert lib.pv_ivae_particles_workspace_bytes(C.byref(p), 1) > 0, fused
        if fused != 1:                                                  # (fused = 1 has no multi-particle step, whatever the likelihood)
            assert lib.pv_ivae_particles_workspace_bytes(C.byref(p), 3) > 0, fused
            assert lib.pv_ivae_renyi_workspace_bytes(C.byref(p), 3) > 0, fused
        # the training layout grows at its very end only: room for the normaliser's partial sums (1024 doubles)
        step_p, step_b = (lib.pv_ivae_workspace_bytes_for(C.byref(q), 1) for q in (p, _ivae_plan(fused, 0, 1)))
        assert step_p == step_b + 8192, (fused, step_p, step_b)
        assert lib.pv_ivae_workspace_bytes(C.byref(_ivae_plan(fused, 3, 1))) == EINVAL, fused     # sigmoid_out with a log-rate
        p.decoder_sig = -3.0                                            # ignored
        assert lib.pv_ivae_workspace_bytes(C.byref(p)) > 0
    keep = C.create_string_buffer(64)
    for field in ("row_w", "row_elbo", "dy"):
        p = _ivae_plan(2)
        p.c_dim = 1 if field == "dy" else 0
        setattr(p, field, C.addressof(keep))
        assert lib.pv_ivae_workspace_bytes(C.byref(p)) == EINVAL, field
        if field != "dy":
            p.lik, p.sigmoid_out = 0, 1                                 # ... which the Bernoulli plan accepts
            assert lib.pv_ivae_workspace_bytes(C.byref(p)) > 0, field
    assert lib.pv_ivae_workspace_bytes(C.byref(_ivae_plan(2, 4, 0))) == EINVAL                    # no such likelihood
    # the fp16 builds of the split-precision path (dec_kernel 21 / 28) hold |rate - x| < 2^15 only: refused by name for a Poisson
    # plan (by size the library keeps such plans on the bf16 three-product kernel, dec_kernel 1), accepted for the Bernoulli
    for sel, ok in ((0, True), (1, True), (21, False), (28, False)):
        p = _ivae_plan(2)
        p.dec_kernel = sel
        assert (lib.pv_ivae_workspace_bytes(C.byref(p)) > 0) == ok, sel
        q = _ivae_plan(2, 0, 1)
        q.dec_kernel = sel
        assert lib.pv_ivae_workspace_bytes(C.byref(q)) > 0, sel
    assert lib.pv_ved_workspace_bytes(C.byref(_ved_plan())) > 0
    assert lib.pv_ved_workspace_bytes(C.byref(_ved_plan())) == lib.pv_ved_workspace_bytes(C.byref(_ved_plan(0, 1))) + 8192
    assert lib.pv_ved_workspace_bytes(C.byref(_ved_plan(3, 1))) == EINVAL
    # the calls refuse a plan without buffers before they touch a pointer
    assert lib.pv_ivae_loss_and_grads(C.byref(_ivae_plan(2)), 1, None) == EINVAL
    assert lib.pv_ved_loss_and_grads(C.byref(_ved_plan()), 1, None) == EINVAL


# ------------------------------------------------------------------------------- what the engines refuse
def test_engines_refuse_at_construction():
    with pytest.raises(UnsupportedModel, match="sigmoid_d=False"):
        pv.models.iVAE((8, 8), 2, ["r"], sampler_d="poisson_log", seed=1, device="cpu").engine()
    with pytest.raises(UnsupportedModel, match="sigmoid_d=False"):
        pv.models.jiVAE((8, 8), 2, 3, ["r"], sampler_d="poisson_log", seed=1, device="cpu").engine()
    with pytest.raises(UnsupportedModel, match="sigmoid_d=False"):
        pv.models.VED((32, 32), (32,), latent_dim=2, sampler_d="poisson_log", seed=1, device="cpu").engine()
    with pytest.raises(UnsupportedModel, match="sigmoid_d=True"):       # the Bernoullis keep needing the sigmoid
        pv.models.iVAE((8, 8), 2, ["r"], sampler_d="bernoulli", sigmoid_d=False, seed=1, device="cpu").engine()
    with pytest.raises(UnsupportedModel, match="per-image normaliser"):
        pv.models.ssiVAE((8, 8), 2, 3, ["r"], sampler_d="poisson_log", sigmoid_d=False, seed=1, device="cpu").engine()
    with pytest.raises(UnsupportedModel, match="per-image normaliser"):
        pv.models.ss_reg_iVAE((8, 8), 2, 1, ["r"], sampler_d="poisson_log", sigmoid_d=False, seed=1, device="cpu").engine()
    with pytest.raises(KeyError):
        pv.models.iVAE((8, 8), 2, ["r"], sampler_d="poisson", sigmoid_d=False, seed=1, device="cpu")


# ------------------------------------------------------------------------------- the GPU step cases' condition
def test_gpu_step_cases_keep_near_zero_gradient_entries_below_one_percent():
    """tests/_judge.py's check_params_after_adam holds entries with |g| < 1e-5 max|g| to 2 lr only, on the
    condition that they are fewer than 1 % of a tensor: confirmed here with the float64 reference alone, for the
    fp32-class cases of tests/_poisson_data.py over their two steps (the count level matters: at rates of 3 - 12 the tanh encoder saturates and the
    share reaches 2 - 27 % in encoder_z.fc_layers.0.weight)."""
    torch.set_num_threads(min(8, torch.get_num_threads()))
    for name in sorted(pr.STEP_CASES):
        model, cfg, x, y, eps, b = pr.step_case(name, "cpu")
        o = orc.SVIOracle({k: v.detach() for k, v in model.state_dict().items()}, cfg, dtype=torch.float64)
        o.sampled_class = pr.STEP_CASES[name].get("sampled", False)
        for k in range(2):
            o.step(x, eps[k], 1.0, y[k] if isinstance(y, list) else y)
            for key, g in o.last_grads.items():
                share = near_zero_share(g)
                assert share < ILL_SHARE, (name, k, key, share)
