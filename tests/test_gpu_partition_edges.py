"""
GPU tests (-m gpu) of the fused decoder kernels at the edges of their row partition, per sample.

Every fused decoder kernel splits its rows the same way (tests/_partition_cases.py restates it): units of 16 rows of one sample,
workgroup g of G = min(units, CUs) owns units [g units / G, (g + 1) units / G) and publishes its partial dL/d(hz[b]) — in some
builds the sample's row sums too — into slot g - gfirst(b) of sample b's kmax slots.  The bound has no slack, and each kernel
carries its own copy of the arithmetic; an off-by-one lands in the next sample's slots: silent corruption, not a fault.

The cases (tests/_partition_cases.CASES) sit where that arithmetic changes: one-unit samples on 257 / 600 / 255 units, three-unit
samples on 513 units, 43 workgroups per sample, every tail length of the 4- and 8-wave tiles, batch == grid and one below, both
sides of the size rules, and K B / P B decoder samples.  Each runs on every kernel family that accepts it (FAMILIES): the f32
kernel, the split-bf16 4-wave kernel, its fp16 builds H231 / H221, the plain-bf16 4- and 8-wave kernels, the multi-channel kernel
(C = 3; C = 6 on e04) and the weighted one (C = 1; C = 4 .. 7 on e04).  tests/test_partition_cases_cpu.py shows with the oracle
alone that no cell is blind to one unit of one sample going astray.

Per cell, one loss_and_grads from the seed-1 parameters: which build and path ran; the four scalars, z_loc / z_scale, loc_out,
every gradient tensor, each decoder.out row / bias entry (C > 1), each entry of row_elbo and each row of dy (one-channel iVAE
cells); a repeated call is bit-identical; want_grads=False gives the gradient call's scalars to 2e-6.

References and bars.  fp32-class families: the float64 oracle (WeightedOracle with weights) at the project's bars — loss / ll 2e-5,
the KL scalars 1e-4, z 1e-4 + 5e-6, loc_out 1e-4 + 2e-6, gradients 1e-4 relative L2 per tensor, per-sample rows 1e-4 per row.
jiVAE: conftest.jivae_grad_tol.  Particles: the same bars (tests/_judge.py: Z_ATOL 2e-6).  H231 / H221: h2_grad_tol(rows,
kind) per tensor and h2_grad_tol(N, kind) per per-sample row; their loc_out max abs error H2_LOC_ATOL (below, from measurement).  Plain bf16: the emulation
oracle/bf16_plan.Bf16Plan at bars set from measurement (_partition_cases.BF16_BARS; at most 4x the measured worst, never above the
ceilings 1e-3 for gradients and dy rows / 1e-5 for the loss and row_elbo entries), plus tests/_bf16_judge.py's self-check against float64.

What the dispatch assertions cover.  A forced build is asserted through plan.dec_kernel (the launcher's only input besides the size);
pv_debug_decoder_kernel_name knows the size rule alone and is used to assert that rule on both of its sides.  The multi-channel and
weighted families are asserted through the library's own predicates (uses_fused -> pv_ivae_uses_fused / pv_ivae_weighted_uses_fused),
plan.fused == 1 and the channel flag.  The guide's own launch on either side of PV_GUIDE_IMG_MAX_BATCH (e09 B = 384 / 385) has no hook:
that edge is covered by parity only.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from pyroved_amd import _abi
from pyroved_amd.engine import IVAEEngine
from oracle import bf16_plan as bp
import _partition_cases as pc
from _bf16_judge import SELF_CHECK, DECODE_BAR
from _device import cus, kernel_name, last_fold_build
from _judge import rel_l2, cpu_threads_16

pytestmark = pytest.mark.gpu

Z_RTOL, Z_ATOL, LOC_RTOL, LOC_ATOL = 1e-4, 5e-6, 1e-4, 2e-6
# loc_out of the fp16 builds, max abs error against float64.  The issue gives no bar; they stage every activation as ONE fp16 piece
# (relative rounding 2^-12 per entry), so the fp32-class 2e-6 cannot hold.  Set from measurement like BF16_LOC_BAR: 4x the worst
# of the 36 H231 / H221 cells, 3.56e-5 (e08).  (A row that reads another sample's hz is off by ~1e-1.)
H2_LOC_ATOL = 1.4e-4
BF16_LOC_BAR = 1.1e-5         # plain bf16, loc_out against the emulation, relative L2: measured worst 2.77e-6 over the 36 plain-bf16 cells (ceiling 1e-4,
                              # tests/_bf16_judge.py: LOC_CEIL)
BF16_Z_BAR = 1e-5             # ... z_loc / z_scale (that file's judge)
EVAL_RTOL = 2e-6


def excess(got, want, rtol, atol):
    """max over entries of |got - want| / (atol + rtol |want|): <= 1 is numpy.allclose"""
    got, want = got.double().cpu().reshape(-1), want.double().cpu().reshape(-1)
    return ((got - want).abs() / (atol + rtol * want.abs())).max().item()


def rows_rel(got, want):
    """relative L2 error of every row on its own: (worst, its index)"""
    got, want = got.double().cpu().reshape(want.shape[0], -1), want.double().cpu().reshape(want.shape[0], -1)
    e = (got - want).norm(dim=1) / want.norm(dim=1).clamp_min(1e-300)
    i = int(e.argmax())
    return e[i].item(), i


_EMULATED = {}


def emulated(name, kernel):
    """the bf16 restatement of the case on this device's grid (one evaluation per process)"""
    key = (name, kernel, cus())
    if key not in _EMULATED:
        _EMULATED[key] = pc.run_reference(name, "plain", plan=bp.Bf16Plan(kernel=kernel, cus=cus()))
    return _EMULATED[key]


# ------------------------------------------------------------------------------- which build and path
def check_dispatch(name, family, model, eng, part):
    c, fam = pc.CASES[name], pc.FAMILIES[family]
    B, variant, sel = c["B"], fam["variant"], fam["sel"]
    units, grid = part["units"], part["grid"]
    assert eng.uses_fused(B) is True, (name, family)
    p = eng._plan(B)
    want_fused = fam["engine"].get("fused", 1)
    assert p.fused == want_fused and p.dec_kernel == sel and p.n_pix == pc.n_pos(c) * pc.channels_of(variant), (name, family)
    assert bool(p.flags & _abi.PV_PLAN_FUSED_CHANNELS) == (pc.channels_of(variant) > 1)
    # the size rule, restated: what the library names for this many units when nothing is forced
    w8_by_size, h231_by_size = units >= 6 * grid, units >= 1024
    n3, n2, n1 = (kernel_name(fused=f, units=units) for f in (3, 2, 1))
    assert ("pv_sdec_w8_kernel<true, 0, 0>" in n3) == w8_by_size, (n3, units, grid)
    assert ("pv_sdec_fused_bf16_kernel<true, 0, 0>" in n3) == (not w8_by_size), n3
    assert ("pv_sdec_fused_bf16_kernel<true, 0, %d>" % (8 if h231_by_size else 1)) in n2, (n2, units)
    assert "pv_sdec_fused_kernel<true>" in n1
    # forward-only launches of the split-precision path: the 8-wave pv_sdec_w8x3 build by size
    assert ("pv_sdec_w8x3_kernel<false, 0, 8>" in kernel_name(fused=2, units=units, grads=0)) == w8_by_size
    # the guide rides in the decoder launch only on the 8-wave plain-bf16 kernel with one unconditioned image per workgroup
    # (the hook sees the plan, and the particle count travels beside the plan: for e11 it answers for the one-particle step of B
    #  images — asserted as such; the P-particle step itself never folds, pv_plan.hip: plan_guide_may_fold)
    hook = bool(_abi.lib().pv_ivae_guide_folds(C.byref(p)))
    one = pc.partition(pc.n_pos(c), B, cus())               # the one-particle / unenumerated plan's partition
    want_hook = family == "bf16w8" and c["kind"] != "jivae" and c["c_dim"] == 0 and one["grid"] == B
    assert hook == want_hook, (name, family, hook, want_hook)
    folds = hook and c["kind"] == "ivae"
    print("[partition-edges] %s %s: plan.fused %d dec_kernel %d, guide folded %s; by size: fused=3 -> %s, fused=2 -> %s"
          % (name, family, p.fused, p.dec_kernel, folds, "8-wave" if w8_by_size else "4-wave", "H231" if h231_by_size else "x3"))
    return folds


# ------------------------------------------------------------------------------- one cell
def run_cell(name, family):
    c, fam = pc.CASES[name], pc.FAMILIES[family]
    variant, sel = fam["variant"], fam["sel"]
    B, S, N, Cn = c["B"], pc.n_samples(c), pc.n_pos(c), pc.channels_of(variant)
    bf16 = family.startswith("bf16")
    part = pc.case_partition(c, cus())
    print("\n[partition-edges] %s %s on %d CUs: %s" % (name, family, cus(), pc.describe(part)))
    assert part["gfirst_ok"] and part["min_slot"] == 0 and part["max_slot"] <= part["kmax"] - 1
    if cus() == pc.CUS:
        for key, want in c["claims"].items():
            assert part[key] == want, (name, key, part[key], want)
    x, y, eps = pc.inputs(name, variant)
    xg, eg, yg = x.cuda(), eps.cuda(), None if y is None else y.cuda()
    res = []                                                 # (quantity, error, bar)
    IVAEEngine.dec_kernel = sel
    try:
        model = pc.make_model(name, variant, "cuda")
        for k, v in model.state_dict().items():              # the reference's parameters are this model's
            assert torch.equal(v.cpu(), pc.params(name, variant)[k]), k
        kw = dict(fam["engine"])
        if variant != "plain" and variant[0] == "w":
            kw["pixel_weights"] = pc.weights_of(name, variant)
        if c["P"] > 1:
            kw["particles"] = c["P"]
        eng = model.engine(**kw)
        folds = check_dispatch(name, family, model, eng, part)
        z_dim = model.z_dim
        zl, zs = torch.empty(B, z_dim, device="cuda"), torch.empty(B, z_dim, device="cuda")
        loc = torch.full((S, N * Cn), float("nan"), device="cuda")
        rows = pc.has_rows(name, family)
        row = torch.full((B,), float("nan"), device="cuda") if rows else None
        dy = torch.full((B, c["c_dim"]), float("nan"), device="cuda") if rows and c["c_dim"] else None
        extra = dict(row_elbo=row, dy=dy) if dy is not None else {}      # conditioned cells: the per-sample outputs ride in the one call
        eng.loss_and_grads(xg, eg, 1.0, yg, z_out=(zl, zs), loc_out=loc, **extra)
        torch.cuda.synchronize()
        if folds:
            assert last_fold_build() == 2, last_fold_build()           # the image-owning training build, generic tile loop (upb < 8)
        s = eng.scalars.cpu().double()
        keys = list(model.state_dict().keys())
        g = {k: eng.grad_of(k).detach().cpu().double().clone() for k in keys}
        assert all(torch.isfinite(v).all() for v in g.values()) and torch.isfinite(s).all()

        f64 = pc.reference(name, variant)
        ref = emulated(name, "w4" if family == "bf16w4" else "w8") if bf16 else f64
        gbar0, lbar = (pc.bf16_bars(name, family)[:2]) if bf16 else (None, pc.RTOL_ELBO)
        # ---- scalars
        for i, (q, bar, r) in enumerate((("loss", lbar, ref), ("ll", lbar, ref), ("logpz", pc.RTOL_KL, f64), ("logqz", pc.RTOL_KL, f64))):
            res.append((q, abs(s[i].item() - r[q]) / abs(r[q]), bar))
        res.append(("loss = -(ll + logpz - logqz)", abs(s[0] + (s[1] + s[2] - s[3])).item() / abs(s[0]).item(), 2e-6))
        # ---- z, loc_out
        z_atol = 2e-6 if c["kind"] == "particles" else Z_ATOL
        res.append(("z_loc (allclose excess)", excess(zl, f64["z_loc"], Z_RTOL, z_atol), 1.0))
        res.append(("z_scale (allclose excess)", excess(zs, f64["z_scale"], Z_RTOL, z_atol), 1.0))
        assert not torch.isnan(loc).any()
        if bf16:
            res.append(("z_loc", rel_l2(zl, ref["z_loc"]), BF16_Z_BAR))
            res.append(("z_scale", rel_l2(zs, ref["z_scale"]), BF16_Z_BAR))
            res.append(("loc_out", rel_l2(loc, ref["loc"]), BF16_LOC_BAR))
        elif family in ("h231", "h221"):
            res.append(("loc_out (max abs error)", (loc.cpu().double() - f64["loc"]).abs().max().item(), H2_LOC_ATOL))
        else:
            res.append(("loc_out (allclose excess)", excess(loc, f64["loc"], LOC_RTOL, LOC_ATOL), 1.0))
        # ---- gradients
        for k in keys:
            bar = pc.grad_bar(name, family, k)
            if bar is None:                                  # jiVAE's decoder.out.bias: one sum of K B N signed terms, absolute scale
                res.append((k + " (abs)", abs(g[k].item() - ref["grads"][k].item()), 1e-6 * S * N + 1e-5))
                continue
            e = rel_l2(g[k], ref["grads"][k])
            res.append((k, e, bar))
            if bf16:
                e64 = rel_l2(g[k], f64["grads"][k])
                if e64 > 1e-3:                                # the emulation must explain the error
                    res.append((k + " (self-check: 10x closer to the emulation than to float64)", SELF_CHECK * e / e64, 1.0))
        if Cn > 1:
            for ch in range(Cn):
                res.append(("decoder.out.weight[%d]" % ch, rel_l2(g["decoder.out.weight"][ch], ref["grads"]["decoder.out.weight"][ch]), pc.RTOL_GRAD))
                res.append(("decoder.out.bias[%d]" % ch, rel_l2(g["decoder.out.bias"][ch], ref["grads"]["decoder.out.bias"][ch]), pc.RTOL_GRAD))
        # ---- a repeated call is bit-identical: scalars, gradients and every output buffer (poisoned in between)
        outs = [t for t in (zl, zs, loc) + tuple(extra.values())]
        first = [t.clone() for t in outs]
        for t in outs:
            t.fill_(float("nan"))
        eng.loss_and_grads(xg, eg, 1.0, yg, z_out=(zl, zs), loc_out=loc, **extra)
        torch.cuda.synchronize()
        same = torch.equal(eng.scalars.cpu().double(), s) and all(torch.equal(eng.grad_of(k).cpu().double(), g[k]) for k in keys) \
            and all(torch.equal(a, b_) for a, b_ in zip(first, outs))
        res.append(("repeated call differs", 0.0 if same else 1.0, 0.5))
        # ---- per sample
        rbar, dbar = pc.row_bars(name, family)
        if rows and dy is None:                              # unconditioned: row_elbo in a call of its own (it changes the closing path)
            eng.loss_and_grads(xg, eg, 1.0, yg, row_elbo=row)
            torch.cuda.synchronize()
            row1 = row.clone()
            row.fill_(float("nan"))
            eng.loss_and_grads(xg, eg, 1.0, yg, row_elbo=row)
            torch.cuda.synchronize()
            res.append(("repeated row_elbo call differs", 0.0 if torch.equal(row1, row) else 1.0, 0.5))
        if rows:
            e = ((row.cpu().double() - ref["row_elbo"]).abs() / ref["row_elbo"].abs())
            res.append(("row_elbo entries (worst: sample %d)" % int(e.argmax()), e.max().item(), rbar))
        if dy is not None:
            e, i = rows_rel(dy, ref["dy"])
            res.append(("dy rows (worst: sample %d)" % i, e, dbar))
            ea = (dy.cpu().double() - ref["dy"]).norm(dim=1) / ref["dy"].norm(dim=1)
            print("[partition-edges] %s %s dy rows: median %.2e, 90 %% %.2e, worst %.2e" % (name, family, ea.median(), ea.quantile(0.9), ea.max()))
        # ---- forward-only
        eng.scalars.fill_(float("nan"))
        eng.loss_and_grads(xg, eg, 1.0, yg, want_grads=False)
        torch.cuda.synchronize()
        if folds:
            assert last_fold_build() == 1
        se = eng.scalars.cpu().double()
        res.append(("want_grads=False scalars", ((se - s).abs() / s.abs()).max().item(), EVAL_RTOL))
    finally:
        IVAEEngine.dec_kernel = 0
    for q, e, bar in res:
        print("[partition-edges] %s %s %-62s %.3e  (bar %.1e)%s" % (name, family, q, e, bar, "" if e < bar else "   <-- FAILS"))
    bad = [(q, e, bar) for q, e, bar in res if not e < bar]
    assert not bad, "%s %s: %s" % (name, family, "; ".join("%s %.3e (bar %.1e)" % t for t in bad))
    return res


@pytest.mark.parametrize("name,family", pc.cells(), ids=["%s-%s" % nf for nf in pc.cells()])
def test_partition_edge(gpu_device, name, family):
    run_cell(name, family)


def test_every_cell_is_run_or_refused_with_a_reason(gpu_device):
    """What _partition_cases.refusal says the engine refuses, the engine refuses."""
    for name, family, err in (("e10_jivae_k3_1d16_t_b86", "w1", "pixel_weights"), ("e11_p3_1d16_t_b86", "f32", "particles"),
                              ("e11_p3_1d16_t_b86", "mc3", "fused_channels"), ("e11_p3_1d16_t_b86", "w1", "pixel_weights")):
        assert pc.refusal(name, family)
        c, fam = pc.CASES[name], pc.FAMILIES[family]
        model = pc.make_model(name, "plain", "cuda")
        kw = dict(fam["engine"])
        if family == "w1":
            kw["pixel_weights"] = pc.weights_of(name, ("w", 1))
        if c["P"] > 1:
            kw["particles"] = c["P"]
        with pytest.raises(ValueError, match=err):
            model.engine(**kw)


# ------------------------------------------------------------------------------- forward-only decode
@pytest.mark.parametrize("mode", ["fp32-class", "bf16"])
@pytest.mark.parametrize("name,n", [("e01_1d16_t_b257", 257), ("e06_8x8_rts_cdim2_b600", 600)])
def test_decode_at_the_partition_edges(gpu_device, name, n, mode):
    """model.decode of 257 one-unit samples / 600 conditioned 8 x 8 samples in one launch (pv_ivae_decode: the split-precision
    forward-only builds whatever the training precision — 4 waves at 257 units, the 8-wave pv_sdec_w8x3 build at 2400) against
    SVIOracle.decode in float64, at the bars of the existing decode tests: 1e-4 + 2e-6, and DECODE_BAR (relative L2) in the bf16
    mode."""
    c = pc.CASES[name]
    model = pc.make_model(name, "plain", "cuda")
    model.engine(fused=3 if mode == "bf16" else 2)
    units = n * pc.n_pos(c) // pc.UNIT
    part = pc.partition(pc.n_pos(c), n, cus())
    print("\n[partition-edges] decode %s: %s" % (name, pc.describe(part)))
    dname = kernel_name(fused=2, units=units, grads=0, lik=1)
    assert ("pv_sdec_w8x3_kernel" in dname) == (units >= 6 * part["grid"]), dname
    g = torch.Generator().manual_seed(2)
    z = torch.randn(n, 2, generator=g)
    y = None
    if c["c_dim"]:
        y = torch.zeros(n, c["c_dim"])
        y[torch.arange(n), torch.randint(0, c["c_dim"], (n,), generator=g)] = 1.0
    o = pc.make_oracle(name, "plain")
    got = model.decode(z, y, batch_size=n).reshape(n, -1)
    want = o.decode(z, y).reshape(n, -1)
    e, (er, i) = rel_l2(got, want), rows_rel(got, want)
    print("[partition-edges] decode %s %s (%s): rel l2 %.3e, worst row %.3e (sample %d), max abs %.3e"
          % (name, mode, dname, e, er, i, (got.double() - want).abs().max().item()))
    np.testing.assert_allclose(got.numpy(), want.numpy(), rtol=1e-4, atol=2e-6)
    if mode == "bf16":
        assert e < DECODE_BAR
