"""
The bf16 throughput step (fused = 3, SVItrainer(precision="bf16")) against a reference that rounds where the kernel rounds
(oracle/bf16_plan.py): the oracle in float64 with the kernel's bf16 operands and per-workgroup bf16 records.  Against the
fp32 oracle the mode can only be held to 3e-2 (its own rounding is 2e-4 .. 1.5e-2), which lets a 1-2 % error through; against
the emulation the remaining distance is fp32 accumulation order, rare bf16 rounding flips and the hardware's 1-ulp exp2 / rcp,
and every gradient tensor is held to <= 1e-3.

Every case first asserts which kernel build it runs, then compares the loss, every parameter gradient and the encoder's
outputs (forward-only runs: loc) with the emulation on the same parameters and noise, and checks that the emulation explains
the error: a tensor more than 1e-3 from the float64 (unemulated) gradient lies at least 10x closer to the emulation.
"""
import ctypes as C
import dataclasses

import numpy as np
import pytest
import torch

from conftest import make_x

import pyroved_amd as pv
from pyroved_amd import _abi
from pyroved_amd.engine import IVAEEngine
from oracle import svi_oracle as orc
from oracle import bf16_plan as bp
from _bf16_judge import judge, SELF_CHECK, DECODE_BAR, LIK
from _device import cus, kernel_name
from _judge import rel_l2, near_zero, cpu_threads_16

pytestmark = pytest.mark.gpu


@dataclasses.dataclass
class Case:
    data_dim: tuple
    inv: list
    batch: int
    kernel: str                   # "w8" / "w4": the build the case must run (and the plan that restates it)
    fold: bool = False            # the guide folded into the decoder launch
    force_w8: bool = False
    xkind: str = "rand"
    xseed: int = 0
    eseed: int = 1
    K: int = 0                    # jiVAE classes
    model_kw: dict = dataclasses.field(default_factory=dict)
    beta: float = 1.0
    seed: int = 1


CASES = {
    # the headline: C2, 8-wave kernel with the guide folded in, 49 units per workgroup = 6 tiles + a column-parallel tail
    "c2_seed0": Case((28, 28), ["r", "t"], 256, "w8", fold=True),
    "c2_seed7": Case((28, 28), ["r", "t"], 256, "w8", fold=True, xseed=7, eseed=11),
    "c2_blobs": Case((28, 28), ["r", "t"], 256, "w8", fold=True, xkind="blobs", xseed=3, eseed=5),
    # C1: ranges of 24 / 25 units (a tail in half the workgroups), ranges crossing image boundaries
    "c1_r_b128": Case((28, 28), ["r"], 128, "w8"),
    # batch > grid: several images per workgroup, not folded
    "rt_b512": Case((28, 28), ["r", "t"], 512, "w8"),
    "rt_b1024": Case((28, 28), ["r", "t"], 1024, "w8"),
    # ranges that are whole tiles, no tail
    "16x16_rts_b256": Case((16, 16), ["r", "t", "s"], 256, "w8", fold=True),
    "16x16_rts_b512": Case((16, 16), ["r", "t", "s"], 512, "w8"),
    # the 8-wave kernel forced on a tiny problem: mostly idle waves, 1-D data
    "forced_1d16_t_b5": Case((16,), ["t"], 5, "w8", fold=True, force_w8=True),
    "forced_8x8_rts_b6": Case((8, 8), ["r", "t", "s"], 6, "w8", force_w8=True),
    # the 8-wave kernel at its size threshold: ranges of 6-7 units, one partial tile
    "r_b32_blobs": Case((28, 28), ["r"], 32, "w8", xkind="blobs"),
    # the 4-wave plain-bf16 build (no C scale, fp32 records)
    "w4_8x8_rts_b6": Case((8, 8), ["r", "t", "s"], 6, "w4"),
    "w4_rt_b16": Case((28, 28), ["r", "t"], 16, "w4"),
    # row weights, class conditioning, the likelihood branches
    "jivae_k10_r_b64": Case((28, 28), ["r"], 64, "w8", K=10),
    "cdim3_rt": Case((8, 8), ["r", "t"], 7, "w8", force_w8=True, model_kw=dict(c_dim=3), beta=1.7, seed=3),
    "gauss_rts": Case((8, 8), ["r", "t", "s"], 7, "w8", force_w8=True, model_kw=dict(sampler_d="gaussian"), beta=1.7, seed=3),
    "gauss_nosig_r": Case((8, 8), ["r"], 7, "w8", force_w8=True, model_kw=dict(sampler_d="gaussian", sigmoid_d=False),
                          beta=1.7, seed=3),
    "cbern_16x16_r": Case((16, 16), ["r"], 7, "w8", force_w8=True, model_kw=dict(sampler_d="continuous_bernoulli"),
                          beta=1.7, seed=3),
    "1d32_t_cdim2": Case((32,), ["t"], 7, "w8", force_w8=True, model_kw=dict(c_dim=2), beta=1.7, seed=3),
}

# Bars per case, from the measured residuals (MI355X): gradient rel L2 (worst tensor), loss relative.  Each bar is <= 4x the
# worst value measured (over the three draws for C2) and <= the ceilings of tests/_bf16_judge.py; the comment gives the measurement and the
# self-check's factor (how much closer the kernel lies to the emulation than to float64, worst tensor more than 1e-3 from it).
_C2 = (1.8e-4, 2.5e-7)                     # worst of the three draws: 4.66e-5 (seed7) / 6.49e-8 (seed7)
BARS = {
    "c2_seed0": _C2,                       # 4.34e-5 / 7.4e-11, factor 55.3
    "c2_seed7": _C2,                       # 4.66e-5 / 6.5e-8, factor 57.9
    "c2_blobs": _C2,                       # 9.21e-6 / 9.1e-9, factor 151.1
    "c1_r_b128": (9.2e-5, 2.1e-7),         # 2.30e-5 / 5.4e-8, factor 90.7
    "rt_b512": (1.0e-4, 8.5e-8),           # 2.68e-5 / 2.1e-8, factor 78.0
    "rt_b1024": (9.2e-5, 7.3e-7),          # 2.32e-5 / 1.8e-7, factor 89.6
    "16x16_rts_b256": (5.2e-4, 1.2e-7),    # 1.31e-4 / 3.2e-8, factor 35.5
    "16x16_rts_b512": (4.3e-4, 6.8e-8),    # 1.10e-4 / 1.7e-8, factor 74.2
    "forced_1d16_t_b5": (5.4e-4, 3.0e-7),  # 1.36e-4 / 7.7e-8, factor 21.4
    "forced_8x8_rts_b6": (8.5e-4, 4.5e-7), # 2.13e-4 / 1.2e-7, factor 23.1
    "r_b32_blobs": (2.8e-5, 1.7e-7),       # 7.23e-6 / 4.3e-8, factor 230.9
    "w4_8x8_rts_b6": (2.2e-4, 2.6e-7),     # 5.70e-5 / 6.6e-8, factor 67.6
    "w4_rt_b16": (3.7e-4, 2.9e-7),         # 9.32e-5 / 7.4e-8, factor 95.7
    "jivae_k10_r_b64": (1.0e-3, 8.7e-7),   # 2.56e-4 / 2.2e-7, factor 11.2
    "cdim3_rt": (1.0e-3, 2.4e-7),          # 2.82e-4 / 6.2e-8, factor 17.8
    "gauss_rts": (6.8e-4, 6.7e-8),         # 1.72e-4 / 1.7e-8, factor 22.4
    "gauss_nosig_r": (2.1e-4, 2.4e-6),     # 5.28e-5 / 6.1e-7, factor 45.8
    # loss above the 1e-5 ceiling: the ContinuousBernoulli ELBO is a remainder of B N terms of size ~0.7 whose sum nearly
    # cancels, and the kernel's log-normaliser (pv_cbern, fp32 transcendentals, left unemulated) errs per TERM; measured
    # 1.59e-5 of the remainder (the variants test in test_gpu_parity.py judges this loss on the terms' scale for that reason)
    "cbern_16x16_r": (1.0e-3, 6.3e-5),     # 4.28e-4 / 1.6e-5, factor 21.3
    "1d32_t_cdim2": (9.1e-4, 3.0e-7),      # 2.29e-4 / 7.5e-8, factor 11.1
}
# trained state: measured 5.42e-4 (fc_layers.0.weight) from the emulation with rounded records, loss 1.16e-7
TRAINED_BARS = (1.0e-3, 4.6e-7)
# record rounding alone in the trained state (emulation with rounded vs exact records): measured 1.64e-3 (W1) / 1.70e-3 (W2)
TRAINED_RECORDS_BAR = 6.5e-3


def _setup(case: Case):
    if case.force_w8:
        IVAEEngine.dec_kernel = 2
    try:
        kw = dict(case.model_kw)
        if case.K:
            model = pv.models.jiVAE(case.data_dim, 2, case.K, case.inv, seed=case.seed, device="cuda", **kw)
        else:
            model = pv.models.iVAE(case.data_dim, 2, case.inv, seed=case.seed, device="cuda", **kw)
        eng = model.engine(fused=3)
        b = case.batch
        x = make_x(case.xkind, b, case.data_dim, seed=case.xseed)
        eps = torch.randn(b, model.z_dim, generator=torch.Generator().manual_seed(case.eseed))
        y = None
        if kw.get("c_dim"):
            g = torch.Generator().manual_seed(11)
            y = torch.zeros(b, kw["c_dim"])
            y[torch.arange(b), torch.randint(0, kw["c_dim"], (b,), generator=g)] = 1.0
        # ---- which build runs ----
        n_pix = int(np.prod(case.data_dim))
        units = (max(case.K, 1) * b * n_pix) // 16
        assert eng.uses_fused(b)
        folds = bool(_abi.lib().pv_ivae_guide_folds(C.byref(eng._plan(b))))
        assert folds == case.fold, (folds, case.fold)
        lik = LIK[kw.get("sampler_d", "bernoulli")]
        if case.force_w8:
            # (the library's name lookup knows the size rule only: that the forced launch IS the 8-wave build is shown by the
            #  result, test_bf16_step_vs_emulated_reference: closer to the 8-wave restatement than to the 4-wave one)
            assert eng._plan(b).dec_kernel == 2
            assert "pv_sdec_w8_kernel" not in kernel_name(fused=3, units=units, lik=lik)       # unforced, this size takes the other build
        else:
            name = kernel_name(fused=3, units=units, lik=lik)
            want = "pv_sdec_w8_kernel<true, %d, 0>" % lik if case.kernel == "w8" else \
                "pv_sdec_fused_bf16_kernel<true, %d, 0>" % lik
            assert want in name, (name, want)
        return model, eng, x, eps, y
    finally:
        IVAEEngine.dec_kernel = 0


def _cfg(case: Case, plan=None):
    kw = case.model_kw
    return orc.Config(data_dim=case.data_dim, latent_dim=2, invariances=case.inv, discrete_dim=case.K, c_dim=kw.get("c_dim", 0),
                      sampler=kw.get("sampler_d", "bernoulli"), sigmoid_d=kw.get("sigmoid_d", True), bf16_plan=plan)


def _reference(case, params, x, eps, y, plan):
    o = orc.SVIOracle(params, _cfg(case, plan), dtype=torch.float64)
    out = o.loss_and_grads(x, eps, case.beta, y)
    return out, {k: v.grad.detach().clone() for k, v in o.p.items()}, o


@pytest.mark.parametrize("name", sorted(CASES))
def test_bf16_step_vs_emulated_reference(gpu_device, name):
    case = CASES[name]
    model, eng, x, eps, y = _setup(case)
    b = case.batch
    zl, zs = torch.empty(b, model.z_dim, device="cuda"), torch.empty(b, model.z_dim, device="cuda")
    if case.force_w8:
        IVAEEngine.dec_kernel = 2
    try:
        eng.loss_and_grads(x.cuda(), eps.cuda(), case.beta, None if y is None else y.cuda(), z_out=(zl, zs))
        torch.cuda.synchronize()
    finally:
        IVAEEngine.dec_kernel = 0
    params = {k: v.detach().cpu() for k, v in model.state_dict().items()}
    plan = bp.Bf16Plan(kernel=case.kernel, cus=cus())
    ref_out, ref_g, o = _reference(case, params, x, eps, y, plan)
    f64_out, f64_g, _ = _reference(case, params, x, eps, y, None)
    grad_bar, loss_bar = BARS[name]
    judge(name, eng, ref_out, ref_g, f64_out, f64_g, zl.cpu(), zs.cpu(), grad_bar, loss_bar, SELF_CHECK)
    if case.force_w8:
        # which build ran, from its arithmetic: the 8-wave kernel's images of C W and bf16-h derivatives, not the 4-wave
        # build's unscaled images and fp32-h derivatives
        _, w4_g, _ = _reference(case, params, x, eps, y, bp.Bf16Plan(kernel="w4", cus=cus()))
        for key in ("decoder.fc_layers.0.weight", "decoder.fc_layers.2.weight"):
            e8, e4 = rel_l2(eng.grad_of(key), ref_g[key]), rel_l2(eng.grad_of(key), w4_g[key])
            print("  %s: vs the 8-wave restatement %.3e, vs the 4-wave one %.3e" % (key, e8, e4))
            assert 3 * e8 < e4, (key, e8, e4)
    if name == "c2_seed0":
        # Adam on the emulated gradient: entries whose gradient is summation-noise-sized (|g| < 1e-5 max) may land on either
        # side (held to 2 lr), every other entry to 1e-4 relative L2 of the step
        p0 = {k: v.detach().clone() for k, v in model.state_dict().items()}
        eng.adam_step()
        torch.cuda.synchronize()
        o.opt = torch.optim.Adam(list(o.p.values()), lr=eng.lr, betas=tuple(eng.betas), eps=eng.adam_eps)
        o.opt.step()
        for k, p in model.state_dict().items():
            gr = ref_g[k].reshape(p.shape)
            ill = near_zero(gr)
            d = (p.detach().cpu().double() - o.p[k].detach())
            assert ill.double().mean() < 0.01 and (not ill.any() or d[ill].abs().max() <= 2 * eng.lr), k
            step = (o.p[k].detach() - p0[k].cpu().double())[~ill]
            err = d[~ill].norm() / step.norm().clamp_min(1e-300)
            assert err < 1e-4 or d[~ill].abs().max() <= 1e-6, (k, err.item())


@pytest.mark.parametrize("name", ["c2_seed0", "r_b32_blobs"])
def test_bf16_forward_only_vs_emulated_reference(gpu_device, name):
    """The forward-only launch of the same kernel (evaluate: want_grads=False): loss and loc against the emulation; and
    model.decode(), whose launch is the split-precision build (asserted), against the float64 oracle."""
    case = CASES[name]
    model, eng, x, eps, y = _setup(case)
    b = case.batch
    n_pix = int(np.prod(case.data_dim))
    loc = torch.empty(b, n_pix, device="cuda")
    eng.loss_and_grads(x.cuda(), eps.cuda(), case.beta, want_grads=False, loc_out=loc)
    torch.cuda.synchronize()
    params = {k: v.detach().cpu() for k, v in model.state_dict().items()}
    plan = bp.Bf16Plan(kernel=case.kernel, cus=cus())
    o = orc.SVIOracle(params, _cfg(case, plan), dtype=torch.float64)
    o64 = orc.SVIOracle(params, _cfg(case), dtype=torch.float64)
    with torch.no_grad():
        ref = o.loss_and_grads(x, eps, case.beta)
        r64 = o64.loss_and_grads(x, eps, case.beta)
    le = abs(eng.scalars[0].item() - ref["loss"].item()) / abs(ref["loss"].item())
    lo = rel_l2(loc, ref["loc"].reshape(b, -1))
    lo64 = rel_l2(loc, r64["loc"].reshape(b, -1))
    print("\n[bf16-emulated] forward %s: loss %.3e, loc %.3e (vs float64 %.3e)" % (name, le, lo, lo64))
    assert le < BARS[name][1] and lo < 4.5e-5       # measured loc 1.03e-5 / 1.10e-5 (ceiling LOC_CEIL)
    # model.decode(): pv_ivae_decode launches the split-precision (fp32-class) build whatever the training precision
    # (pv_plan.hip: decode_fused_run) — not the plain-bf16 kernel — so its reference is the plain float64 oracle
    dname = kernel_name(fused=2, units=b * n_pix // 16, grads=0, lik=LIK["gaussian"])
    assert "pv_sdec_w8_kernel" not in dname and "0>(PvFused, PvEncFold)" not in dname, dname
    z = torch.randn(b, 2, generator=torch.Generator().manual_seed(2))
    d = model.decode(z).reshape(b, -1)
    d64 = o64.decode(z).reshape(b, -1)
    de, de_em = rel_l2(d, d64), rel_l2(d, o.decode(z).reshape(b, -1))
    print("  decode (%s): vs float64 %.3e, vs the bf16 restatement %.3e" % (dname, de, de_em))
    assert de < DECODE_BAR


def test_bf16_trained_state_records(gpu_device):
    """Near convergence per-workgroup partials cancel and a record rounded relative to itself need not be small relative to
    the sum: C2 after 300 steps on one fixed batch, the step's gradient against the emulation with rounded
    records, against the absolute scale 2^-8 sqrt(sum_g |partial_g|^2), and its distance from float64 split into what the
    records and what the bf16 operands contribute."""
    case = CASES["c2_seed0"]
    model, eng, x, eps, y = _setup(case)
    b = case.batch
    xg = x.cuda()
    gen = torch.Generator().manual_seed(123)
    for _ in range(300):
        e = torch.randn(b, model.z_dim, generator=gen)
        eng.loss_and_grads(xg, e.cuda(), step=True)
    torch.cuda.synchronize()
    zl, zs = torch.empty(b, model.z_dim, device="cuda"), torch.empty(b, model.z_dim, device="cuda")
    eng.loss_and_grads(xg, eps.cuda(), z_out=(zl, zs))
    torch.cuda.synchronize()
    params = {k: v.detach().cpu() for k, v in model.state_dict().items()}
    plan = bp.Bf16Plan(kernel="w8", cus=cus())
    ref_out, ref_g, _ = _reference(case, params, x, eps, y, plan)
    parts = dict(plan.partials)
    _, nr_g, _ = _reference(case, params, x, eps, y, bp.Bf16Plan(kernel="w8", cus=cus(), round_records=False))
    f64_out, f64_g, _ = _reference(case, params, x, eps, y, None)
    rows = judge("c2_trained", eng, ref_out, ref_g, f64_out, f64_g, zl.cpu(), zs.cpu(), *TRAINED_BARS)
    for k, key in (("W1", "decoder.fc_layers.0.weight"), ("W2", "decoder.fc_layers.2.weight")):
        pt = parts[k]
        tot = pt.sum(0)
        scale = pt.pow(2).sum().sqrt().item()
        ratio = tot.norm().item() / scale
        dist_abs = (eng.grad_of(key).cpu().double() - ref_g[key]).norm().item()
        e64 = rel_l2(eng.grad_of(key), f64_g[key])
        e_rec = rel_l2(ref_g[key], nr_g[key])           # what the record rounding alone moves
        e_ops = rel_l2(nr_g[key], f64_g[key])           # the bf16 operands alone (records exact)
        print("  %s: |sum partials| / sqrt(sum |partial|^2) = %.4f; kernel - emulation = %.3e of that scale; vs float64 %.3e"
              % (key, ratio, dist_abs / scale, e64))
        print("  %s: attribution vs float64: records alone %.3e, operands alone %.3e" % (key, e_rec, e_ops))
        assert dist_abs <= 2.0 ** -8 * scale, key
        # Attribution of the distance from float64 (measured 3.6e-2 W1, 4.5e-2 W2 — above the 3e-2 the mode states at
        # initialisation): the bf16 OPERANDS carry it (emulation with exact records: 3.6e-2 / 4.5e-2), the packed records
        # move the gradient by 1.6e-3 / 1.7e-3 only.  fp32 records would not restore 3e-2; DESIGN.md 4.1 states the trained bound.
        assert e_rec < TRAINED_RECORDS_BAR, (key, e_rec)
        assert e_ops > 0.9 * e64 and e64 < 1.8e-1, (key, e_ops, e64)      # (1.8e-1: 4x the measured 4.5e-2)
