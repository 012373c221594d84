"""
_fast_weight_cases.py — the case table, the references and the bars of the tests of fast_weights=True: weighted steps
(pixel_weights= / image_weights=) on the weighted instances of the 4-wave bf16-class fused decoder kernel
(pv_sdec_fused_bf16_wt_kernel; PV_PLAN_FAST_WEIGHTS in the C ABI).

Two routes per case: "x3" (fused = 2, three bf16 products, fp32-class: the float64 WeightedOracle / ImageWeightedOracle and the
bars of tests/_judge.py) and "bf16" (fused = 3 / precision="bf16", plain bf16 operands: the same classes over a Config whose
bf16_plan restates the 4-wave build's roundings, judged by tests/_bf16_judge.py at the per-case bars below).

The shapes are the smallest at which each thing can go wrong on a 256-CU device (G = workgroups = min(units, 256), a unit = 16
rows); every case is one channel, hidden [128, 128], tanh:
  f01  8x8 rts, B = 6, shared disc                    24 units: grid = units < CUs, one unit per workgroup
  f02  (32,) t, B = 5, Gaussian, no sigmoid, ramp     one coordinate; fractional weights and exact zeros
  f03  6x8 rt, B = 171, per-image pdisc               3 units per sample on 513 units: samples straddle workgroups, the per-image
                                                      index wraps inside a workgroup
  f04  8x8 rts, B = 256 / 255, cont. Bernoulli, pramp batch == grid (the own-sample epilogue, part_rs) and one below
  f05  8x8 r, c_dim = 2, B = 352, Poisson, pramp      1408 units: 5 / 6 per workgroup, the weight prefetched across a tile
                                                      boundary; the weighted normaliser
  f06  (16,) t, B = 257, per-image pdisc              one unit per sample, two samples in one workgroup
  f07  28x28 rt, B = 6, Gaussian, per-image pdisc     one image over 42-43 workgroups (kmax = 44)
In every per-image case image 2 is masked out completely: it contributes its KL terms only.
"""
import dataclasses

import torch

from oracle import bf16_plan as bp
import _multichannel_cases as mc
import _pixel_weight_cases as pw
import _image_weight_cases as iwc
from _bf16_judge import GRAD_CEIL, LOSS_CEIL

CASES = {
    "f01_8x8_rts_b6_disc": dict(dims=(8, 8), inv=["r", "t", "s"], C=1, b=6, w="disc"),
    "f02_1d32_t_b5_gauss_nosig_ramp": dict(dims=(32,), inv=["t"], C=1, b=5, sampler="gaussian", sigmoid_d=False, w="ramp"),
    "f03_6x8_rt_b171_pdisc": dict(dims=(6, 8), inv=["r", "t"], C=1, b=171, w="pdisc", zero=(2,)),
    "f04_8x8_rts_b256_cbern_pramp": dict(dims=(8, 8), inv=["r", "t", "s"], C=1, b=256, sampler="continuous_bernoulli", w="pramp",
                                         zero=(2,)),
    "f04_8x8_rts_b255_cbern_pramp": dict(dims=(8, 8), inv=["r", "t", "s"], C=1, b=255, sampler="continuous_bernoulli", w="pramp",
                                         zero=(2,)),
    "f05_8x8_r_cdim2_b352_poisson_pramp": dict(dims=(8, 8), inv=["r"], C=1, b=352, c_dim=2, sampler="poisson_log", sigmoid_d=False,
                                               w="pramp", zero=(2,)),
    "f06_1d16_t_b257_pdisc": dict(dims=(16,), inv=["t"], C=1, b=257, w="pdisc", zero=(2,)),
    "f07_28x28_rt_b6_gauss_pdisc": dict(dims=(28, 28), inv=["r", "t"], C=1, b=6, sampler="gaussian", w="pdisc", zero=(2,)),
}
CASE1 = "f01_8x8_rts_b6_disc"
ANALYTIC = ("f01_8x8_rts_b6_disc", "f03_6x8_rt_b171_pdisc", "f05_8x8_r_cdim2_b352_poisson_pramp")
ROUTES = {"x3": 2, "bf16": 3}                       # route -> the engine's `fused`
PREC = {"x3": 1, "bf16": 0}                         # route -> the kernel's PREC template argument (FB_P_X3, FB_P_BF16)
LIK = {"bernoulli": 0, "gaussian": 1, "continuous_bernoulli": 2, "poisson_log": 3}

# plain-bf16 route: (gradient bar: worst tensor's relative L2 against the emulation; loss bar: relative) per case.  The rule is
# tests/test_gpu_bf16_emulated.py's: 4x the case's own measured worst value over the two steps and both KL forms, never above the
# ceilings of tests/_bf16_judge.py, a loss bar never below 2.4e-7 (two fp32 roundings of the loss).  The measured
# values (MI355X; gradient / loss, and where they arose) stand in the comment beside each bar.
BF16_BARS = {
    # (f01's loss bar also judges the trainer test's history on f01's data — two epochs of four Adam steps each, then evaluate: the
    #  mean loss per image after the parameters went their own way for up to eight steps — and its worst value arose there)
    "f01_8x8_rts_b6_disc": (1.5e-4, 7.1e-6),                      # 3.76e-5 (sampled and analytic, step 0) / 1.76e-6 (trainer, second
                                                                  # epoch; the step test's own worst: 2.98e-7, sampled, step 1)
    "f02_1d32_t_b5_gauss_nosig_ramp": (6.1e-5, 6.0e-7),           # 1.52e-5 (step 0) / 1.49e-7 (step 1)
    "f03_6x8_rt_b171_pdisc": (9.5e-5, 7.1e-7),                    # 2.37e-5 (analytic, step 1) / 1.78e-7 (analytic, step 1)
    "f04_8x8_rts_b256_cbern_pramp": (3.4e-5, 4.3e-6),             # 8.59e-6 (step 0) / 1.07e-6 (step 0)
    "f04_8x8_rts_b255_cbern_pramp": (3.1e-5, 5.0e-6),             # 7.77e-6 (step 0) / 1.24e-6 (step 0)
    "f05_8x8_r_cdim2_b352_poisson_pramp": (2.3e-4, 3.1e-7),       # 5.74e-5 (analytic, step 1) / 7.83e-8 (analytic, step 0)
    "f06_1d16_t_b257_pdisc": (7.5e-5, 9.9e-7),                    # 1.87e-5 (step 0) / 2.48e-7 (step 1)
    "f07_28x28_rt_b6_gauss_pdisc": (8.8e-5, 8.7e-7),              # 2.21e-5 (step 0) / 2.16e-7 (step 0)
}


def per_image(c):
    return c["w"].startswith("p")


def weights(c):
    """The case's weights as the engine takes them: (*dims) shared, (b, *dims) per image."""
    return iwc.weights(c)[..., 0].contiguous() if per_image(c) else pw.weights(c)


def engine_kw(c, route, **kw):
    """model.engine keywords of a case on a route (per-image cases bring their weights with every call)."""
    kw = dict(kw, fused=ROUTES[route], fast_weights=True)
    if per_image(c):
        kw["image_weights"] = True
    else:
        kw["pixel_weights"] = weights(c)
    return kw


def call_kw(c, device="cuda"):
    """loss_and_grads keywords of a case."""
    return dict(image_weights=weights(c).to(device)) if per_image(c) else {}


def config(c, route="x3", cus=256, exact=False):
    """The reference's Config: plain for the x3 route (float64 is the reference of an fp32-class path), with the 4-wave build's
    roundings restated for the bf16 route."""
    cfg = mc.case_config(c)
    if route == "bf16":
        cfg = dataclasses.replace(cfg, bf16_plan=bp.Bf16Plan(kernel="w4", cus=cus, exact=exact))
    return cfg


def oracle(c, params, route="x3", kl="sampled", cus=256, w=None, exact=False, lr=1e-3):
    """WeightedOracle / ImageWeightedOracle in float64 on the route's Config."""
    w = weights(c) if w is None else w
    cls = iwc.ImageWeightedOracle if per_image(c) else pw.WeightedOracle
    return cls(params, config(c, route, cus, exact), w, lr=lr, dtype=torch.float64, kl=kl)


case_data = pw.case_data


def kernel_name(c, route, grads=True):
    """The weighted 4-wave instance a case runs, as rocprofv3 prints it."""
    return "void pv_sdec_fused_bf16_wt_kernel<%s, %d, %d>(PvFused, PvEncFold, int)" % (
        "true" if grads else "false", LIK[c.get("sampler", "bernoulli")], PREC[route])
