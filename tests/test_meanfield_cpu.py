"""
The analytic-KL (mean-field) objective — SVItrainer(loss="TraceMeanField_ELBO"), engine(kl="analytic"), plan.kl_mode —
where no GPU is needed: the reference itself (oracle.svi_oracle with kl="analytic"), the trainer's argument handling, the ABI
struct and the library's plan validation (host arithmetic).
"""
import ctypes as C
import math
import os
import re

import pytest
import torch

from conftest import ROOT

import pyroved_amd as pv
from pyroved_amd import _abi
from oracle import svi_oracle as orc


def _params(cfg, seed=0):
    """A CPU state_dict of the right shapes for the oracle (no engine, no GPU)."""
    model = pv.models.iVAE(cfg.data_dim, cfg.latent_dim, cfg.invariances, seed=1, device="cpu")
    g = torch.Generator().manual_seed(seed)
    return {k: (v.detach() + 0.05 * torch.randn(v.shape, generator=g)).double() for k, v in model.state_dict().items()}


CASES = [((8, 8), ["r", "t", "s"]), ((28, 28), ["r", "t"]), ((16,), ["t"]), ((8, 8), None)]


@pytest.mark.parametrize("data_dim,inv", CASES)
def test_helper_loss_and_gradients_equal_the_formulas_in_float64(data_dim, inv):
    """loss = -sum log p(x|z) + beta sum KL with KL = 0.5 (sigma^2 + mu^2 - 1) - log sigma; the slots' relation
    loss = -(ll + logpz - logqz) with their analytic expectations; and the latent backward the kernels implement
    (dL/dmu = dz + beta mu, dL/dsigma = dz eps + beta (sigma - 1/sigma)) against autograd."""
    cfg = orc.Config(data_dim=data_dim, latent_dim=2, invariances=inv)
    p = {k: v.clone().requires_grad_(True) for k, v in _params(cfg).items()}
    g = torch.Generator().manual_seed(3)
    b, beta = 5, 1.7
    x = torch.rand(b, *data_dim, generator=g, dtype=torch.float64)
    eps = torch.randn(b, cfg.z_dim, generator=g, dtype=torch.float64)
    out = orc.elbo(p, cfg, x, eps, beta, kl="analytic")
    mu, sig = out["z_loc"], out["z_scale"]
    kl = (0.5 * (sig ** 2 + mu ** 2 - 1.0) - torch.log(sig)).sum()
    want = -out["ll"] + beta * kl
    assert abs(out["loss"].item() - want.item()) <= 1e-12 * abs(want.item())
    slots = -(out["ll"] + out["logpz"] - out["logqz"])
    assert abs(out["loss"].item() - slots.item()) <= 1e-12 * abs(want.item())
    c = 0.5 * math.log(2 * math.pi)
    assert torch.allclose(out["logpz"], beta * (-(mu ** 2 + sig ** 2) / 2 - c).sum(), rtol=1e-13, atol=0)
    assert torch.allclose(out["logqz"], beta * (-0.5 - torch.log(sig) - c).sum(), rtol=1e-13, atol=0)
    # the latent backward: dz = d(-ll)/dz from the decoder, then the two closed forms
    z = out["z"]
    dz, = torch.autograd.grad(-out["ll"], z, retain_graph=True)
    dmu, dsig = torch.autograd.grad(out["loss"], [mu, sig])
    assert (dmu - (dz + beta * mu)).abs().max().item() < 1e-12
    assert (dsig - (dz * eps + beta * (sig - 1.0 / sig))).abs().max().item() < 1e-12


def test_sampled_kl_converges_to_the_analytic_one():
    """The mean over many eps of the SAMPLED oracle's logqz - logpz is beta * KL: 4096 draws on 8x8 `rts`, compared at five
    standard errors of that mean (computed here)."""
    cfg = orc.Config(data_dim=(8, 8), latent_dim=2, invariances=["r", "t", "s"])
    p = _params(cfg)
    g = torch.Generator().manual_seed(7)
    b, beta, n = 6, 1.3, 4096
    x = torch.rand(b, 8, 8, generator=g, dtype=torch.float64)
    with torch.no_grad():
        ref = orc.elbo(p, cfg, x, torch.zeros(b, cfg.z_dim, dtype=torch.float64), beta, kl="analytic")
        want = (ref["logqz"] - ref["logpz"]).item()
        assert abs(want - beta * ref["kl"].sum().item()) < 1e-12 * abs(want)
        draws = torch.empty(n, dtype=torch.float64)
        for i in range(n):
            out = orc.elbo(p, cfg, x, torch.randn(b, cfg.z_dim, generator=g, dtype=torch.float64), beta)
            draws[i] = out["logqz"] - out["logpz"]
    mean, sem = draws.mean().item(), draws.std(unbiased=True).item() / n ** 0.5
    assert sem > 0 and abs(mean - want) <= 5 * sem, (mean, want, sem)


def test_meanfield_oracle_inherits_adam_and_epochs():
    cfg = orc.Config(data_dim=(8, 8), latent_dim=2, invariances=["r"])
    p = {k: v.float() for k, v in _params(cfg).items()}
    o, s = orc.SVIOracle(p, cfg, kl="analytic"), orc.SVIOracle(p, cfg)
    g = torch.Generator().manual_seed(1)
    x, eps = torch.rand(4, 8, 8, generator=g), torch.randn(4, cfg.z_dim, generator=g)
    l0, l1 = o.step(x, eps), s.step(x, eps)
    assert l0 != l1 and o.last["ll"].item() == pytest.approx(s.last["ll"].item(), rel=1e-6)
    k = "encoder_z.fc11.weight"
    assert not torch.equal(o.p[k], p[k]) and float(o.p[k].grad.abs().sum()) == 0.0       # Adam stepped, grads zeroed
    loader = pv.utils.init_dataloader(x, batch_size=2)
    torch.manual_seed(0)
    assert math.isfinite(o.train_epoch(loader)) and math.isfinite(o.evaluate_epoch(loader))


# ------------------------------------------------------------------------------- trainer arguments
class _StandInEngine:
    """What SVItrainer needs from an engine before the first step (the existing engine= hook)."""
    device = torch.device("cpu")
    grads_live = False
    kl = "unset"

    def __init__(self):
        self.lr = self.betas = self.adam_eps = None
        self.reset = 0

    def reset_optimizer(self):
        self.reset += 1


@pytest.mark.parametrize("loss,kl", [(None, "sampled"), ("Trace_ELBO", "sampled"), ("TraceMeanField_ELBO", "analytic")])
def test_trainer_accepts_the_objective_strings_and_hands_kl_to_the_engine(loss, kl):
    model = pv.models.iVAE((8, 8), 2, ["r"], seed=1, device="cpu")
    eng = _StandInEngine()
    tr = pv.trainers.SVItrainer(model, loss=loss, seed=1, engine=eng)
    assert tr.engine is eng and eng.kl == kl and eng.reset == 1 and tr.svi is None


def test_trainer_rejects_unknown_objective_strings():
    model = pv.models.iVAE((8, 8), 2, ["r"], seed=1, device="cpu")
    for bad in ("TraceGraph_ELBO", "trace_elbo", "", "meanfield"):
        with pytest.raises(ValueError) as e:
            pv.trainers.SVItrainer(model, loss=bad, seed=1, engine=_StandInEngine())
        assert "'Trace_ELBO'" in str(e.value) and "'TraceMeanField_ELBO'" in str(e.value)


@pytest.mark.parametrize("enumerate_parallel", [False, True])
def test_trainer_rejects_the_meanfield_objective_for_jivae(enumerate_parallel):
    model = pv.models.jiVAE((8, 8), 2, 3, None, seed=1, device="cpu")
    with pytest.raises(ValueError, match="jiVAE"):
        pv.trainers.SVItrainer(model, loss="TraceMeanField_ELBO", enumerate_parallel=enumerate_parallel, seed=1,
                               engine=_StandInEngine())


def test_loss_objects_still_take_the_pyro_route():
    """Anything that is not one of the strings is a Pyro object: without pyro-ppl that is the TypeError it always was."""
    try:
        import pyro  # noqa: F401
        return          # (pyro-ppl is installed: the Pyro route itself is tests/test_gpu_pyro_programs.py's)
    except ImportError:
        pass
    model = pv.models.iVAE((8, 8), 2, ["r"], seed=1, device="cpu")
    with pytest.raises(TypeError, match="pyro-ppl"):
        pv.trainers.SVItrainer(model, loss=object(), seed=1)


def test_aux_trainer_has_no_loss_argument():
    import inspect
    assert "loss" not in inspect.signature(pv.trainers.auxSVItrainer.__init__).parameters


# ------------------------------------------------------------------------------- ABI
def test_abi_version_and_kl_mode_fields():
    """kl_mode sits where the header has it in both plans (a compiled probe, as test_plan_struct_matches_header_layout does for
    the fields it lists), takes the place of reserved0, and the enum's values are the binding's."""
    import subprocess
    import tempfile
    assert _abi.PV_ABI_VERSION == 17 and _abi.lib().pv_version() == 17
    assert _abi.KL == {"sampled": 0, "analytic": 1}
    names = [f[0] for f in _abi.pv_ivae_plan._fields_]
    assert "reserved0" not in names and names[-1] == "kl_mode" and names[-2] == "dec_kernel"
    probe = r'''
#include <stdio.h>
#include <stddef.h>
#include "pyroved_amd.h"
int main() {
  printf("%zu %zu %zu %zu %zu %d %d %d\n", offsetof(pv_ivae_plan, kl_mode), sizeof(pv_ivae_plan), offsetof(pv_ved_plan, kl_mode),
         offsetof(pv_ved_plan, params), sizeof(pv_ved_plan), (int)PV_KL_SAMPLED, (int)PV_KL_ANALYTIC, PV_ABI_VERSION);
  return 0; }'''
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "p.c"), "w").write(probe)
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), os.path.join(d, "p.c"), "-o", os.path.join(d, "p")])
        got = [int(v) for v in subprocess.check_output([os.path.join(d, "p")]).split()]
    P, V = _abi.pv_ivae_plan, _abi.pv_ved_plan
    assert got == [P.kl_mode.offset, C.sizeof(P), V.kl_mode.offset, V.params.offset, C.sizeof(V), 0, 1, 17]
    src = open(os.path.join(ROOT, "include", "pyroved_amd.h")).read()
    assert not re.search(r"\breserved0\s*;", src)


def _small_plan(kl_mode, discrete_dim=0):
    p = _abi.pv_ivae_plan()
    p.batch, p.n_pix, p.coord_dim, p.z_dim, p.latent_dim = 16, 784, 2, 5, 2
    p.has_r = p.has_t = 1
    p.lik, p.sigmoid_out, p.fused = _abi.LIK["bernoulli"], 1, 2

    def layer(i, o, act):
        l = _abi.pv_layer()
        l.in_dim, l.out_dim, l.act, l.b_off = i, o, _abi.ACT[act], 0
        return l
    p.n_enc = 2
    p.enc[0], p.enc[1] = layer(784, 128, "tanh"), layer(128, 128, "tanh")
    p.discrete_dim = discrete_dim
    p.head = layer(128, 10 + discrete_dim, None)
    p.fc_coord, p.fc_latent = layer(2, 128, "tanh"), layer(2 + discrete_dim, 128, None)
    p.n_dec = 2
    p.dec[0], p.dec[1] = layer(128, 128, "tanh"), layer(128, 128, "tanh")
    p.out = layer(128, 1, None)
    p.kl_mode = kl_mode
    return p


def test_library_validates_kl_mode_in_the_workspace_queries():
    """Host arithmetic only: kl_mode outside {0, 1} and PV_KL_ANALYTIC with a discrete latent are PV_EINVAL; both forms size
    the same workspace; the analytic form never hosts the guide in the decoder launch."""
    lib = _abi.lib()
    ws = [lib.pv_ivae_workspace_bytes(C.byref(_small_plan(m))) for m in (0, 1)]
    assert ws[0] > 0 and ws[0] == ws[1]
    for bad in (2, -1, 7):
        p = _small_plan(bad)
        assert lib.pv_ivae_workspace_bytes(C.byref(p)) == -1
        assert all(lib.pv_ivae_workspace_bytes_for(C.byref(p), w) == -1 for w in (1, 2, 3))
        # the step / loss calls refuse it before they touch a pointer
        assert lib.pv_ivae_loss_and_grads(C.byref(p), 1, None) == -1 and lib.pv_ivae_step(C.byref(p), None) == -1
    assert lib.pv_ivae_workspace_bytes(C.byref(_small_plan(0, discrete_dim=3))) > 0
    pj = _small_plan(1, discrete_dim=3)
    assert lib.pv_ivae_workspace_bytes(C.byref(pj)) == -1 and lib.pv_ivae_loss_and_grads(C.byref(pj), 1, None) == -1
    for fused in (2, 3):
        for b in (256, 304):
            p = _small_plan(1)
            p.batch, p.fused = b, fused
            assert lib.pv_ivae_guide_folds(C.byref(p)) == 0
    v = _abi.pv_ved_plan()
    v.kl_mode = 3
    assert lib.pv_ved_workspace_bytes(C.byref(v)) < 0 and lib.pv_ved_loss_and_grads(C.byref(v), 1, None) == -1


def test_engine_rejects_unknown_kl_names():
    from pyroved_amd.engine import _kl_name
    assert _kl_name("sampled") == "sampled" and _kl_name("analytic") == "analytic"
    with pytest.raises(ValueError):
        _kl_name("closed-form")
