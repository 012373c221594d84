"""
_partition_cases.py — the row partition every fused decoder kernel shares, restated in Python, and the case table the tests of
its edges run on (tests/test_partition_cases_cpu.py, tests/test_gpu_partition_edges.py).

The partition (pyroved_amd/csrc/pv_sdec_partition.h: sd_grid, sd_unit_bound, sd_gfirst, sd_slot, sd_kmax — the one text the kernels
and the host compile; tests/test_partition_cases_cpu.py holds this restatement against it through pv_debug_partition_table):
  * a unit is 16 rows of one decoder sample; a sample of N positions has upb = N / 16 units; S samples make units = S upb;
  * G = min(units, CUs) workgroups; workgroup g owns units [g units / G, (g + 1) units / G);
  * it publishes its partial dL/d(hz[b]) (in some builds the sample's row sums too) into slot g - gfirst(b) of sample b's
    kmax = upb G / units + 2 slots, gfirst(b) = ceil((b upb + 1) G / units) - 1 being the first workgroup that touches sample b.
S is the batch B — or K B for a jiVAE of K classes, P B for a P-particle ELBO.

Everything a case needs is made here once per process and shared: the seed-1 parameters, the inputs, the float64 reference.
"""
import functools

import numpy as np
import torch
import torch.distributions as td

from conftest import jivae_grad_tol
from _judge import h2_grad_tol
from oracle import svi_oracle as orc
import _multichannel_cases as mc
import _pixel_weight_cases as pw

UNIT = 16
CUS = 256                      # MI355X: the grid the table's claims are stated for


# ------------------------------------------------------------------------------- the partition, restated
def grid_of(units, cus=CUS):
    return max(1, min(int(units), int(cus)))


def kmax_of(upb, units, grid):
    return (upb * grid) // max(units, 1) + 2


def partition(N, S, cus=CUS):
    """Everything the kernels' arithmetic implies for S samples of N rows on `cus` compute units.  The workgroups' ranges come
    from the bounds themselves (a search over them: no formula shared with the kernels), `gfirst` from the kernels' formula."""
    assert N % UNIT == 0 and S >= 1
    upb = N // UNIT
    units = S * upb
    G = grid_of(units, cus)
    bounds = np.arange(G + 1, dtype=np.int64) * units // G
    per_wg = np.diff(bounds)
    assert per_wg.min() >= 1
    spw = (bounds[1:] - 1) // upb - bounds[:-1] // upb + 1                      # samples a workgroup touches
    b = np.arange(S, dtype=np.int64)
    first = np.searchsorted(bounds, b * upb, side="right") - 1                  # the workgroup that owns sample b's first unit
    last = np.searchsorted(bounds, (b + 1) * upb - 1, side="right") - 1         # ... its last unit
    gfirst = ((b * upb + 1) * G + units - 1) // units - 1                       # the kernels' formula
    kmax = kmax_of(upb, units, G)
    return dict(N=N, S=S, upb=upb, units=units, grid=G, kmax=kmax, bounds=bounds, first=first,
                units_per_wg=sorted(set(per_wg.tolist())), units_per_wg_counts={int(v): int((per_wg == v).sum()) for v in set(per_wg.tolist())},
                samples_per_wg=sorted(set(spw.tolist())), samples_per_wg_counts={int(v): int((spw == v).sum()) for v in set(spw.tolist())},
                wgs_per_sample=(int((last - first + 1).min()), int((last - first + 1).max())),
                gfirst_ok=bool((gfirst == first).all()), min_slot=int((first - gfirst).min()), max_slot=int((last - gfirst).max()),
                first_phases=len(set(((b * upb) - bounds[first]).tolist())))   # distinct offsets of a sample's start inside its workgroup


def describe(p):
    return ("N %d S %d: upb %d, %d units on %d workgroups (%s units each), samples per workgroup %s, workgroups per sample %d..%d, "
            "kmax %d, slots used %d..%d" % (p["N"], p["S"], p["upb"], p["units"], p["grid"], p["units_per_wg_counts"],
                                            p["samples_per_wg_counts"], p["wgs_per_sample"][0], p["wgs_per_sample"][1], p["kmax"],
                                            p["min_slot"], p["max_slot"]))


# ------------------------------------------------------------------------------- cases
# kind: "ivae" | "jivae" (K classes, S = K B) | "particles" (P particles, S = P B).  claims: what the case is in the table for,
# as values of partition(N, S, 256).  twin_of: the c_dim = 2 twin of an unconditioned case (it carries row_elbo and dy).
def _case(dims, inv, B, kind="ivae", c_dim=0, K=0, P=1, claims=None, twin_of=None):
    return dict(dims=tuple(dims), inv=list(inv), B=B, kind=kind, c_dim=c_dim, K=K, P=P, claims=claims or {}, twin_of=twin_of)


CASES = {
    # upb = 1; 257 units: one workgroup with two samples, 255 with one
    "e01_1d16_t_b257": _case((16,), "t", 257, claims=dict(upb=1, units=257, grid=256, samples_per_wg_counts={1: 255, 2: 1})),
    # 2-3 samples per workgroup, a flush per unit inside one tile
    "e02_1d16_t_b600": _case((16,), "t", 600, claims=dict(upb=1, units=600, samples_per_wg=[2, 3], units_per_wg=[2, 3])),
    # grid = units < CUs, two coordinates, upb = 1
    "e03_4x4_rts_b255": _case((4, 4), "rts", 255, claims=dict(upb=1, units=255, grid=255, units_per_wg=[1])),
    # upb = 3, 513 = 2 * 256 + 1 units: samples of three units on workgroups of two, so a sample starts at either phase of its
    # workgroup and straddles two of them (the one three-unit workgroup holds a whole sample)
    "e04_6x8_rt_b171": _case((6, 8), "rt", 171, claims=dict(upb=3, units=513, grid=256, units_per_wg_counts={2: 255, 3: 1},
                                                            first_phases=2, wgs_per_sample=(1, 2), kmax=3)),
    # 294 units: 42-43 workgroups per sample, kmax = 44, 1-2 units per workgroup
    "e05_28x28_rt_b6": _case((28, 28), "rt", 6, claims=dict(upb=49, units=294, grid=256, kmax=44, units_per_wg=[1, 2],
                                                            wgs_per_sample=(42, 43))),
    # 9 / 10 units per workgroup: an 8-unit tile plus a 1- or 2-unit tail (4-wave: 4 + 4 + 1 / 4 + 4 + 2); the size selects H231 and
    # the 8-wave builds on its own
    "e06_8x8_rts_cdim2_b600": _case((8, 8), "rts", 600, c_dim=2, claims=dict(upb=4, units=2400, grid=256, units_per_wg=[9, 10])),
    # 5 / 6 and 6 / 7 units per workgroup: every tail length of the 4-wave tile
    "e07_8x8_r_cdim2_b352": _case((8, 8), "r", 352, c_dim=2, claims=dict(upb=4, units=1408, units_per_wg=[5, 6])),
    "e07_8x8_r_cdim2_b416": _case((8, 8), "r", 416, c_dim=2, claims=dict(upb=4, units=1664, units_per_wg=[6, 7])),
    # batch == grid against one below it; 1024 units is exactly FB_H231_MIN_UNITS
    "e08_8x8_rts_b255": _case((8, 8), "rts", 255, claims=dict(upb=4, units=1020, grid=256, units_per_wg=[3, 4])),
    "e08_8x8_rts_b256": _case((8, 8), "rts", 256, claims=dict(upb=4, units=1024, grid=256, units_per_wg=[4], samples_per_wg=[1],
                                                              wgs_per_sample=(1, 1))),
    # batch == grid with a one-unit image; both sides of PV_GUIDE_IMG_MAX_BATCH (384)
    "e09_1d16_t_b256": _case((16,), "t", 256, claims=dict(upb=1, units=256, grid=256, units_per_wg=[1], samples_per_wg=[1])),
    "e09_1d16_t_b384": _case((16,), "t", 384, claims=dict(upb=1, units=384, grid=256, units_per_wg=[1, 2])),
    "e09_1d16_t_b385": _case((16,), "t", 385, claims=dict(upb=1, units=385, grid=256, units_per_wg=[1, 2])),
    # S = 258: observations addressed modulo B N across the seam
    "e10_jivae_k3_1d16_t_b86": _case((16,), "t", 86, kind="jivae", K=3, claims=dict(upb=1, units=258, grid=256,
                                                                                     samples_per_wg_counts={1: 254, 2: 2})),
    # the same for P B samples
    "e11_p3_1d16_t_b86": _case((16,), "t", 86, kind="particles", P=3, claims=dict(upb=1, units=258, grid=256,
                                                                                   samples_per_wg_counts={1: 254, 2: 2})),
    # c_dim = 2 twins: the per-sample outputs (row_elbo, dy) at the one-unit image, the straddling phases and kmax = 44
    "e01y_1d16_t_cdim2_b257": _case((16,), "t", 257, c_dim=2, twin_of="e01_1d16_t_b257"),
    "e04y_6x8_rt_cdim2_b171": _case((6, 8), "rt", 171, c_dim=2, twin_of="e04_6x8_rt_b171"),
    "e05y_28x28_rt_cdim2_b6": _case((28, 28), "rt", 6, c_dim=2, twin_of="e05_28x28_rt_b6"),
}
for _n, _c in CASES.items():
    if _c["twin_of"]:
        _c["claims"] = dict(CASES[_c["twin_of"]]["claims"])
E04 = "e04_6x8_rt_b171"

# family: how the engine is asked for it.  variant: which model / reference it needs ("plain", ("mc", C), ("w", C)).
FAMILIES = {
    "f32": dict(engine=dict(fused=1), sel=0, variant="plain"),
    "x3": dict(engine=dict(fused=2), sel=1, variant="plain"),                    # split bf16, 4 waves
    "h231": dict(engine=dict(fused=2), sel=28, variant="plain"),
    "h221": dict(engine=dict(fused=2), sel=21, variant="plain"),
    "bf16w4": dict(engine=dict(fused=3), sel=1, variant="plain"),                # plain bf16, 4 waves
    "bf16w8": dict(engine=dict(fused=3), sel=2, variant="plain"),                # plain bf16, 8 waves
    "mc3": dict(engine=dict(fused_channels=True), sel=0, variant=("mc", 3)),
    "mc6": dict(engine=dict(fused_channels=True), sel=0, variant=("mc", 6)),
    "w1": dict(engine=dict(), sel=0, variant=("w", 1)),
    "w4": dict(engine=dict(fused_channels=True), sel=0, variant=("w", 4)),
    "w5": dict(engine=dict(fused_channels=True), sel=0, variant=("w", 5)),
    "w6": dict(engine=dict(fused_channels=True), sel=0, variant=("w", 6)),
    "w7": dict(engine=dict(fused_channels=True), sel=0, variant=("w", 7)),
}
ONLY_E04 = ("mc6", "w4", "w5", "w6", "w7")


def refusal(name, family):
    """None when the case runs on the family, else the reason it does not."""
    c = CASES[name]
    var = FAMILIES[family]["variant"]
    if family in ONLY_E04 and name != E04:
        return "this channel count is run on e04 only (one launch per compiled instance)"
    if c["kind"] == "jivae" and var != "plain":
        return "fused_channels / pixel_weights are implemented for models.iVAE only (engine._check_fused_channels / _check_pixel_weights)"
    if c["kind"] == "particles":
        if var != "plain":
            return "fused_channels / pixel_weights run the one-particle ELBO only"
        if family == "f32":
            return "particles > 1 runs on fused = 0, 2 or 3, not on the f32-MFMA kernel (engine._check_particles)"
    return None


def cells():
    return [(n, f) for n in CASES for f in FAMILIES if refusal(n, f) is None]


def n_samples(c):
    return c["B"] * (c["K"] if c["kind"] == "jivae" else c["P"])


def n_pos(c):
    return int(np.prod(c["dims"]))


def case_partition(c, cus=CUS):
    return partition(n_pos(c), n_samples(c), cus)


# ------------------------------------------------------------------------------- models, inputs
def channels_of(variant):
    return 1 if variant == "plain" else variant[1]


def make_model(name, variant, device):
    import pyroved_amd as pv
    c = CASES[name]
    if c["kind"] == "jivae":
        return pv.models.jiVAE(c["dims"], 2, c["K"], c["inv"], seed=1, device=device)
    kw = dict(c_dim=c["c_dim"])
    if channels_of(variant) > 1:
        kw["channels"] = channels_of(variant)
    return pv.models.iVAE(c["dims"], 2, c["inv"], seed=1, device=device, **kw)


def make_config(name, variant):
    c = CASES[name]
    return orc.Config(data_dim=c["dims"], latent_dim=2, invariances=c["inv"], c_dim=c["c_dim"], discrete_dim=c["K"],
                      channels=channels_of(variant))


def weights_of(name, variant):
    """strictly positive weights (0.25 + 1.5 rand): a zero would take a position out of the objective on both sides"""
    c, C = CASES[name], channels_of(variant)
    w = pw.soft(c["dims"], C)
    return w[..., 0].contiguous() if C == 1 else w


DY_FLOOR = 1.0 / 3.0           # conditioned cases: every sample's dy row is at least this fraction of the median row norm


def _draw(name, variant, n):
    """n candidate samples: (x, y, eps)"""
    c, C = CASES[name], channels_of(variant)
    x = mc.images(torch.Generator().manual_seed(0), n, c["dims"], C)
    x = x if C > 1 else x[..., 0].contiguous()
    z_dim = make_config(name, variant).z_dim
    eps = torch.randn(c["P"] * n, z_dim, generator=torch.Generator().manual_seed(1))
    y = None
    if c["c_dim"]:
        y = torch.zeros(n, c["c_dim"])
        y[torch.arange(n), torch.arange(n) % c["c_dim"]] = 1.0
    return x, y, eps


@functools.lru_cache(maxsize=None)
def inputs(name, variant):
    """(x, y, eps): x (B, *dims[, C]) in (0, 1), y one-hot (B, c_dim) or None, eps (P B, z_dim) — float32, fixed seeds.
    x is _multichannel_cases.images (smooth bumps, 0.05 + amp exp(-d^2 / 0.18)), not uniform noise: at initialisation the decoder's
    mean is 0.5 everywhere, so against noise of mean 0.5 every bias gradient is a sum that cancels to its own rounding error and a
    relative bar measures nothing.
    Conditioned cases: dy[b] = d loss / d y[b] is the sum of an encoder and a decoder path that can cancel, and a relative error
    per row is only as good as the row is conditioned (a row 1 / 100 of the typical norm shows 100x the arithmetic's error).  The
    samples are therefore the first B of 2 B candidates whose float64 dy row has at least DY_FLOOR of the candidates' median norm —
    a sample's row depends on nothing but the sample, and the choice is made with the reference alone
    (tests/test_partition_cases_cpu.py asserts the outcome)."""
    c = CASES[name]
    B = c["B"]
    if not c["c_dim"]:
        return _draw(name, variant, B)
    x, y, eps = _draw(name, variant, 2 * B)
    cfg = make_config(name, variant)
    p = {k: v.double() for k, v in params(name, variant).items()}
    yl = y.double().requires_grad_(True)
    orc.elbo(p, cfg, x.double(), eps.double(), 1.0, yl, orc.generate_grid(cfg.data_dim, torch.float64))["loss"].backward()
    norm = yl.grad.norm(dim=1)
    keep = torch.nonzero(norm >= DY_FLOOR * norm.median()).flatten()[:B]
    assert keep.numel() == B, (name, keep.numel())
    return x[keep].contiguous(), y[keep].contiguous(), eps[keep].contiguous()


@functools.lru_cache(maxsize=None)
def params(name, variant):
    """the seed-1 parameters, from a CPU model (the GPU tests assert that their model holds the same values)"""
    return {k: v.detach().clone() for k, v in make_model(name, variant, "cpu").state_dict().items()}


# ------------------------------------------------------------------------------- the float64 reference
def make_oracle(name, variant, plan=None, state=None):
    c = CASES[name]
    cfg = make_config(name, variant)
    if plan is not None:
        import dataclasses
        cfg = dataclasses.replace(cfg, bf16_plan=plan)
    state = params(name, variant) if state is None else state
    if variant != "plain" and variant[0] == "w":
        return pw.WeightedOracle(state, cfg, weights_of(name, variant), dtype=torch.float64)
    return orc.SVIOracle(state, cfg, dtype=torch.float64, particles=c["P"])


def run_reference(name, variant, plan=None, state=None):
    """One loss_and_grads of the float64 oracle (y a float64 leaf), read-only afterwards: scalars, z_loc / z_scale, loc, every
    gradient, and where the model is an iVAE the per-sample row_elbo = ll_b + (log p(z_b) - log q(z_b)) and dy = d loss / d y."""
    c = CASES[name]
    x, y, eps = inputs(name, variant)
    o = make_oracle(name, variant, plan, state)
    yl = None if y is None else y.double().requires_grad_(True)
    out = o.loss_and_grads(x, eps, 1.0, yl)
    ref = dict(loss=out["loss"].item(), ll=out["ll"].item(), logpz=out["logpz"].item(), logqz=out["logqz"].item(),
               z_loc=out["z_loc"].detach(), z_scale=out["z_scale"].detach(), loc=out["loc"].detach().reshape(n_samples(c), -1),
               grads={k: v.grad.detach().clone() for k, v in o.p.items()}, row_elbo=None, dy=None, oracle=o)
    if c["kind"] == "ivae":
        z, zl, zs = out["z"].detach(), out["z_loc"].detach(), out["z_scale"].detach()
        kl = (td.Normal(torch.zeros_like(z), torch.ones_like(z)).log_prob(z) - td.Normal(zl, zs).log_prob(z)).sum(-1)
        ref["row_elbo"] = out["ll_per_sample"].detach() + kl
    if yl is not None:
        ref["dy"] = yl.grad.detach().clone()
    return ref


@functools.lru_cache(maxsize=None)
def reference(name, variant):
    return run_reference(name, variant)


# ------------------------------------------------------------------------------- one unit of one sample, taken out
def unit_term_grads(name, variant, s, u):
    """Gradient of what unit u (16 positions) of decoder sample s contributes to the loss — the difference between the objective
    and the objective without that unit: {parameter: gradient}, the term itself, and its gradient in y[b] (or None).  Computed
    on the sample's own image alone (nothing else in the batch enters the term)."""
    c, C = CASES[name], channels_of(variant)
    cfg = make_config(name, variant)
    x, y, eps = inputs(name, variant)
    B = c["B"]
    b, e = s % B, eps[s if c["kind"] == "particles" else s % B]
    p = {k: v.detach().double().requires_grad_(True) for k, v in params(name, variant).items()}
    grid = orc.generate_grid(cfg.data_dim, torch.float64)
    m = torch.zeros(n_pos(c), C, dtype=torch.float64)
    m[u * UNIT:(u + 1) * UNIT] = 1.0
    if variant != "plain" and variant[0] == "w":
        m = m * weights_of(name, variant).reshape(n_pos(c), C).double()
    m = m.reshape(-1)
    x1, e1 = x[b:b + 1].double(), e.reshape(1, -1).double()
    y1 = None if y is None else y[b:b + 1].double().requires_grad_(True)
    if c["kind"] == "jivae":
        K, k = c["K"], s // B
        z_loc, z_scale, alpha = orc.jencoder_forward(p, cfg, x1)
        z = z_loc + z_scale * e1
        loc, _ = orc.decode_from_latent(p, cfg, z.repeat(K, 1), torch.eye(K, dtype=torch.float64), grid)
        lp = orc.likelihood(cfg, loc.reshape(K, -1)).log_prob(x1.reshape(1, -1))
        term = -alpha[0, k] * (lp[k] * m).sum()
    else:
        z_loc, z_scale = orc._encode_any(p, cfg, x1, y1)
        z = z_loc + z_scale * e1
        loc, _ = orc.decode_from_latent(p, cfg, z, y1, grid)
        lp = orc.likelihood(cfg, loc.reshape(1, -1)).log_prob(x1.reshape(1, -1))
        term = -(lp[0] * m).sum() / c["P"]
    term.backward()
    g = {k: (torch.zeros_like(v) if v.grad is None else v.grad.detach()) for k, v in p.items()}
    return g, term.item(), (None if y1 is None else y1.grad.detach()[0])


# ------------------------------------------------------------------------------- bars
RTOL_ELBO, RTOL_KL, RTOL_GRAD, RTOL_ROW = 2e-5, 1e-4, 1e-4, 1e-4       # the project's fp32-class bars; per-sample rows: 1e-4 rel L2


# plain bf16 against the emulation (oracle/bf16_plan.py), per (case, family): (gradient bar, loss bar, row_elbo bar, dy bar).  Each is
# 4x the value measured for that cell on MI355X (256 CUs; in the comment: worst gradient tensor / the worse of loss and ll / worst
# row_elbo entry / worst dy row), and never above the ceilings of tests/_bf16_judge.py: 1e-3 for gradients and dy rows,
# 1e-5 for the loss and the row_elbo entries.  Where 4x would pass the ceiling the ceiling is the bar (two dy bars, 19 row_elbo bars).
# One deviation from "4x the cell's own value": the loss bar is never below BF16_LOSS_FLOOR = 2 fp32 eps — measured loss residuals go
# down to 1.4e-8, under fp32's own rounding of the scalar (6e-8), and 4x such a value would be a bar on the scalar's last bit.
# A cell without an entry has no bar: bf16_bars raises.
BF16_GRAD_CEIL, BF16_LOSS_CEIL = 1e-3, 1e-5
BF16_LOSS_FLOOR = 2.4e-7
BF16_BARS = {
    ("e01_1d16_t_b257", "bf16w4"): (2.8e-05, 4.3e-07, 1.0e-05, None),             # 7.15e-06 / 1.08e-07 / 5.64e-06 / -
    ("e01_1d16_t_b257", "bf16w8"): (7.7e-05, 4.5e-07, 1.0e-05, None),             # 1.93e-05 / 1.14e-07 / 4.51e-06 / -
    ("e02_1d16_t_b600", "bf16w4"): (2.0e-05, 2.4e-07, 1.0e-05, None),             # 5.25e-06 / 3.71e-08 / 5.64e-06 / -
    ("e02_1d16_t_b600", "bf16w8"): (4.8e-05, 2.4e-07, 1.0e-05, None),             # 1.22e-05 / 3.51e-08 / 7.62e-06 / -
    ("e03_4x4_rts_b255", "bf16w4"): (3.8e-05, 2.7e-07, 1.0e-05, None),            # 9.56e-06 / 6.86e-08 / 6.27e-06 / -
    ("e03_4x4_rts_b255", "bf16w8"): (7.1e-05, 3.4e-07, 1.0e-05, None),            # 1.78e-05 / 8.55e-08 / 5.29e-06 / -
    ("e04_6x8_rt_b171", "bf16w4"): (2.7e-05, 2.7e-07, 1.0e-05, None),             # 6.97e-06 / 6.95e-08 / 4.59e-06 / -
    ("e04_6x8_rt_b171", "bf16w8"): (6.3e-05, 2.4e-07, 9.3e-06, None),             # 1.57e-05 / 5.55e-08 / 2.35e-06 / -
    ("e05_28x28_rt_b6", "bf16w4"): (4.1e-05, 2.4e-07, 1.4e-06, None),             # 1.04e-05 / 1.75e-08 / 3.66e-07 / -
    ("e05_28x28_rt_b6", "bf16w8"): (1.3e-04, 4.0e-07, 8.0e-07, None),             # 3.31e-05 / 1.02e-07 / 2.00e-07 / -
    ("e06_8x8_rts_cdim2_b600", "bf16w4"): (1.6e-05, 2.4e-07, 1.0e-05, 6.2e-04),      # 4.10e-06 / 4.29e-08 / 2.98e-06 / 1.57e-04
    ("e06_8x8_rts_cdim2_b600", "bf16w8"): (3.0e-05, 2.4e-07, 1.0e-05, 1.0e-03),      # 7.69e-06 / 2.14e-08 / 2.78e-06 / 3.41e-04
    ("e07_8x8_r_cdim2_b352", "bf16w4"): (2.2e-05, 2.4e-07, 9.1e-06, 5.3e-04),        # 5.71e-06 / 1.44e-08 / 2.29e-06 / 1.34e-04
    ("e07_8x8_r_cdim2_b352", "bf16w8"): (3.2e-05, 2.4e-07, 1.0e-05, 8.3e-04),        # 8.07e-06 / 3.47e-08 / 3.41e-06 / 2.10e-04
    ("e07_8x8_r_cdim2_b416", "bf16w4"): (2.1e-05, 3.3e-07, 9.4e-06, 5.3e-04),        # 5.26e-06 / 8.48e-08 / 2.37e-06 / 1.34e-04
    ("e07_8x8_r_cdim2_b416", "bf16w8"): (2.8e-05, 7.9e-07, 1.0e-05, 8.9e-04),        # 7.24e-06 / 1.99e-07 / 3.41e-06 / 2.23e-04
    ("e08_8x8_rts_b255", "bf16w4"): (3.1e-05, 2.4e-07, 8.7e-06, None),            # 7.80e-06 / 4.27e-08 / 2.18e-06 / -
    ("e08_8x8_rts_b255", "bf16w8"): (4.2e-05, 3.1e-07, 9.9e-06, None),            # 1.06e-05 / 7.75e-08 / 2.49e-06 / -
    ("e08_8x8_rts_b256", "bf16w4"): (3.2e-05, 2.4e-07, 8.7e-06, None),            # 8.00e-06 / 3.42e-08 / 2.18e-06 / -
    ("e08_8x8_rts_b256", "bf16w8"): (4.7e-05, 3.5e-07, 9.9e-06, None),            # 1.20e-05 / 8.81e-08 / 2.49e-06 / -
    ("e09_1d16_t_b256", "bf16w4"): (2.9e-05, 3.4e-07, 1.0e-05, None),             # 7.28e-06 / 8.60e-08 / 5.64e-06 / -
    ("e09_1d16_t_b256", "bf16w8"): (7.7e-05, 5.5e-07, 1.0e-05, None),             # 1.93e-05 / 1.38e-07 / 4.51e-06 / -
    ("e09_1d16_t_b384", "bf16w4"): (2.1e-05, 2.4e-07, 1.0e-05, None),             # 5.43e-06 / 4.51e-08 / 5.64e-06 / -
    ("e09_1d16_t_b384", "bf16w8"): (5.6e-05, 3.0e-07, 1.0e-05, None),             # 1.40e-05 / 7.64e-08 / 4.51e-06 / -
    ("e09_1d16_t_b385", "bf16w4"): (2.3e-05, 2.6e-07, 1.0e-05, None),             # 5.95e-06 / 6.72e-08 / 5.64e-06 / -
    ("e09_1d16_t_b385", "bf16w8"): (5.8e-05, 2.4e-07, 1.0e-05, None),             # 1.45e-05 / 5.17e-08 / 4.51e-06 / -
    ("e10_jivae_k3_1d16_t_b86", "bf16w4"): (3.2e-05, 5.5e-07, None, None),     # 8.20e-06 / 1.38e-07 / - / -
    ("e10_jivae_k3_1d16_t_b86", "bf16w8"): (4.5e-05, 6.8e-07, None, None),     # 1.14e-05 / 1.72e-07 / - / -
    ("e11_p3_1d16_t_b86", "bf16w4"): (3.2e-05, 3.6e-07, None, None),           # 8.04e-06 / 9.17e-08 / - / -
    ("e11_p3_1d16_t_b86", "bf16w8"): (6.6e-05, 2.4e-07, None, None),           # 1.67e-05 / 5.31e-08 / - / -
    ("e01y_1d16_t_cdim2_b257", "bf16w4"): (2.3e-05, 2.4e-07, 1.0e-05, 8.2e-04),      # 5.77e-06 / 4.22e-08 / 5.63e-06 / 2.07e-04
    ("e01y_1d16_t_cdim2_b257", "bf16w8"): (5.2e-05, 2.5e-07, 1.0e-05, 1.0e-03),      # 1.32e-05 / 6.39e-08 / 3.23e-06 / 3.69e-04
    ("e04y_6x8_rt_cdim2_b171", "bf16w4"): (3.5e-05, 3.8e-07, 8.9e-06, 6.3e-04),      # 8.82e-06 / 9.60e-08 / 2.24e-06 / 1.59e-04
    ("e04y_6x8_rt_cdim2_b171", "bf16w8"): (4.0e-05, 2.4e-07, 5.8e-06, 3.2e-04),      # 1.02e-05 / 5.38e-08 / 1.46e-06 / 8.11e-05
    ("e05y_28x28_rt_cdim2_b6", "bf16w4"): (4.1e-05, 3.9e-07, 9.6e-07, 2.7e-05),      # 1.03e-05 / 9.77e-08 / 2.41e-07 / 6.75e-06
    ("e05y_28x28_rt_cdim2_b6", "bf16w8"): (6.2e-05, 6.0e-07, 9.5e-07, 8.3e-05),      # 1.57e-05 / 1.52e-07 / 2.39e-07 / 2.10e-05
}


def bf16_bars(name, family):
    return BF16_BARS[(name, family)]


def grad_bar(name, family, key):
    """The bar of one gradient tensor (relative L2), or None where the tensor is judged on an absolute scale (jiVAE's out.bias)."""
    c = CASES[name]
    rows = n_samples(c) * n_pos(c)
    sel = FAMILIES[family]["sel"]
    if family.startswith("bf16"):
        return bf16_bars(name, family)[0]
    bar = h2_grad_tol(rows, sel) if family in ("h231", "h221") else RTOL_GRAD
    if c["kind"] == "jivae":
        j = jivae_grad_tol(key)
        return None if j is None else max(j, bar)
    return bar


def row_bars(name, family):
    """(row_elbo entry bar, dy row bar)"""
    if family.startswith("bf16"):
        b = bf16_bars(name, family)
        return b[2], b[3]
    if family in ("h231", "h221"):
        t = h2_grad_tol(n_pos(CASES[name]), FAMILIES[family]["sel"])
        return t, t
    return RTOL_ROW, RTOL_ROW


def has_rows(name, family):
    """whether the cell carries per-sample quantities: row_elbo (every one-channel iVAE) and dy (c_dim > 0)"""
    c = CASES[name]
    return c["kind"] == "ivae" and FAMILIES[family]["variant"] == "plain"
