"""
GPU tests (-m gpu) of fused_any_size: a spatial model whose positions are no multiple of 16 on the tail form of the fused f32
decoder kernel — model.engine(fused_any_size=True) / SVItrainer(model, fused_any_size=True) -> plan.fused = 1 +
PV_PLAN_FUSED_TAIL -> pv_sdec_fused_mc_tail_kernel<GRADS, C, WEIGHTED> (pyroved_amd/csrc/pv_sdec_fused_mc.hip).

A sample occupies 16 ceil(N / 16) rows of the kernel's partition and observes the first N; the padding rows read nothing and
contribute exact zeros, so the bars are the project's own, unloosened (tests/_judge.py, tests/test_gpu_multichannel_fused.py):
loss and ll 2e-5, the KL scalars 1e-4, every gradient tensor 1e-4 relative L2 against the float64 oracle, the parameters after
Adam by the 5e-5 rule, loc_out and decode rtol 1e-4 atol 2e-6.  The shapes are the smallest at which the tail can go wrong:
  a  (5,) ['t'] B 6                 one partial unit per sample, N < 16, one coordinate
  b  (17,) ['t'] B 200              a full unit and a one-row tail; 400 units: workgroups of one and of two units on a 256-CU
                                    grid, sample boundaries inside workgroups, inactive waves
  c  (7, 9) ['r', 't', 's'] B 6     a 15-row tail, all four transform gradients; Bernoulli, Gaussian and Poisson (no sigmoid)
  d  (5, 5) x 3 channels B 6        fused_channels=True; every channel's output-layer row on its own
  e  (7, 9) + pixel_weights         a disc mask with zeros among the valid rows; once with c_dim = 2
  f  (7, 9) + image_weights         one image masked out completely
Every case: two steps with Adam between against the oracle; one step against the same model at fused=0; evaluate against the
gradient call; decode; a repeated call bit for bit — the repeat with x, the per-image weights and loc_out as views of exactly
B N C values inside NaN-filled tensors and the workspace, of exactly the queried size, filled with 0xFF bytes (NaN as fp32).
"""
import numpy as np
import pytest
import torch

import pyroved_amd as pv
from pyroved_amd import _abi
from oracle import svi_oracle as orc
import _multichannel_cases as mc
import _pixel_weight_cases as pw
import _image_weight_cases as iwc
import _ws_contract as wc
from _judge import RTOL_ELBO, RTOL_GRAD, LR, rel_l2, state, steps_vs_reference, cpu_threads_16
from test_gpu_multichannel_fused import check_channels

pytestmark = pytest.mark.gpu

UNIT = 16
CASES = {
    "a_1d5_t_b6": dict(dims=(5,), inv=["t"], C=1, b=6),
    "b_1d17_t_b200": dict(dims=(17,), inv=["t"], C=1, b=200),
    "c_7x9_rts_b6": dict(dims=(7, 9), inv=["r", "t", "s"], C=1, b=6),
    "c_7x9_rts_b6_gauss_nosig": dict(dims=(7, 9), inv=["r", "t", "s"], C=1, b=6, sampler="gaussian", sigmoid_d=False),
    "c_7x9_rts_b6_poisson": dict(dims=(7, 9), inv=["r", "t", "s"], C=1, b=6, sampler="poisson_log", sigmoid_d=False),
    "d_5x5_rt_c3_b6": dict(dims=(5, 5), inv=["r", "t"], C=3, b=6, engine=dict(fused_channels=True)),
    "e_7x9_rt_b6_disc": dict(dims=(7, 9), inv=["r", "t"], C=1, b=6, w="disc", weights="pixel"),
    "e_7x9_rt_cdim2_b6_disc": dict(dims=(7, 9), inv=["r", "t"], C=1, b=6, c_dim=2, w="disc", weights="pixel"),
    "f_7x9_rt_b6_pdisc": dict(dims=(7, 9), inv=["r", "t"], C=1, b=6, w="pdisc", zero=(3,), weights="image"),
}


def n_pos(c):
    return int(np.prod(c["dims"]))


class Case:
    """A case's model, engine keywords, data, weights and float64 reference."""

    def __init__(self, name):
        self.name, self.c = name, CASES[name]
        c = self.c
        self.b, self.n_obs = c["b"], n_pos(c) * c["C"]
        x, self.y, self.eps = mc.case_data(c)
        self.x = x[..., 0].contiguous() if c["C"] == 1 else x
        self.kw = dict(c.get("engine", {}))
        self.call_kw = {}
        self.w_img = None
        if c.get("weights") == "pixel":
            self.kw["pixel_weights"] = pw.weights(c)
            assert bool((self.kw["pixel_weights"] == 0).any()) and bool((self.kw["pixel_weights"] > 0).any())
        elif c.get("weights") == "image":
            self.kw["image_weights"] = True
            self.w_img = iwc.weights(c)[..., 0].contiguous()
            assert float(self.w_img[c["zero"][0]].abs().sum()) == 0.0
            self.call_kw["image_weights"] = self.w_img.cuda()

    def model(self):
        c = self.c
        return pv.models.iVAE(c["dims"], 2, c["inv"], seed=1, device="cuda", **mc.model_kwargs(c))

    def engine(self, **kw):
        model = self.model()
        own = {k: v for k, v in self.kw.items() if not (k == "fused_channels" and kw.get("fused") == 0)}      # (fused=0 refuses it)
        return model, model.engine(**{**own, **kw})

    def oracle(self, model):
        c, cfg = self.c, mc.case_config(self.c)
        if c.get("weights") == "pixel":
            return pw.WeightedOracle(state(model), cfg, pw.weights(c), lr=LR, dtype=torch.float64)
        if c.get("weights") == "image":
            return iwc.ImageWeightedOracle(state(model), cfg, iwc.weights(c), lr=LR, dtype=torch.float64)
        return orc.SVIOracle(state(model), cfg, lr=LR, dtype=torch.float64)

    def call(self, eng, k=0, x=None, **kw):
        yg = None if self.y is None else self.y.cuda()
        eng.loss_and_grads(self.x.cuda() if x is None else x, self.eps[k].cuda(), 1.0, yg, **{**self.call_kw, **kw})
        torch.cuda.synchronize()


def flagged(case):
    model, eng = case.engine(fused_any_size=True)
    assert eng._plan_fused() == 1 and eng._plan_flags() & _abi.PV_PLAN_FUSED_TAIL
    assert eng.uses_fused(case.b) is True and eng.supports_dp_step is False
    return model, eng


# ------------------------------------------------------------------------------- 1. two steps against the oracle
@pytest.mark.parametrize("name", sorted(CASES))
def test_steps_vs_reference(gpu_device, name):
    case = Case(name)
    model, eng = flagged(case)
    o = case.oracle(model)
    loc = torch.full((case.b, case.n_obs), float("nan"), device="cuda")
    steps_vs_reference(eng, model, o, case.x, case.y, case.eps, 1.0, "%s fused_any_size" % name, 0, 5e-6, atol=mc.loss_atol(case.c),
                       checks=[check_channels] if case.c["C"] > 1 else [], loc_out=loc, **case.call_kw)
    assert not torch.isnan(loc).any()


# ------------------------------------------------------------------------------- 2. against the layered kernels
@pytest.mark.parametrize("name", sorted(CASES))
def test_agrees_with_the_layered_kernels(gpu_device, name):
    case = Case(name)
    grads = []
    for kw in (dict(fused=0), dict(fused_any_size=True)):
        model, eng = case.engine(**kw)
        assert eng.uses_fused(case.b) is ("fused_any_size" in kw)
        case.call(eng)
        grads.append({k: eng.grad_of(k).clone() for k in model.state_dict()})
    for k in grads[0]:
        err = rel_l2(grads[1][k], grads[0][k])
        assert err < RTOL_GRAD, "%s %s: fused_any_size against layered, rel l2 %.3e" % (name, k, err)


# ------------------------------------------------------------------------------- 3. evaluate
@pytest.mark.parametrize("name", sorted(CASES))
def test_evaluate_gives_the_gradient_calls_scalars(gpu_device, name):
    """The same per-row values from the same forward arithmetic; the two closing launches sum them in different (blocked)
    orders: the bar and the reasoning of tests/test_gpu_multichannel_fused.py's test of the same name (at most 3400 rows of one
    sign here: log2(n) u = 12 * 6e-8 relative, 2e-6 leaves a factor of two)."""
    case = Case(name)
    model, eng = flagged(case)
    case.call(eng)
    with_grads = eng.scalars.clone()
    eng.scalars.fill_(float("nan"))
    case.call(eng, want_grads=False)
    print("%s evaluate: %s, gradient call: %s" % (name, eng.scalars.tolist(), with_grads.tolist()))
    np.testing.assert_allclose(eng.scalars.cpu().numpy(), with_grads.cpu().numpy(), rtol=2e-6)


# ------------------------------------------------------------------------------- 4. decode
@pytest.mark.parametrize("name", sorted(CASES))
def test_decode_with_a_transform_and_manifold(gpu_device, name):
    case = Case(name)
    c = case.c
    model, eng = flagged(case)
    o = orc.SVIOracle(state(model), mc.case_config(c), dtype=torch.float64)
    z = torch.randn(5, 2, generator=torch.Generator().manual_seed(2))
    y = None if case.y is None else case.y[:5]
    if len(c["dims"]) == 2:
        dec = model.decode(z, y, angle=0.3, shift=[0.1, -0.2], scale=1.2)
        want = o.decode(z, y, 0.3, [0.1, -0.2], 1.2, rate=True)
    else:
        dec = model.decode(z, y)
        want = o.decode(z, y, rate=True)
    shape = (5,) + tuple(c["dims"]) + ((c["C"],) if c["C"] > 1 else ())
    assert tuple(dec.shape) == shape and bool(torch.isfinite(dec).all())
    np.testing.assert_allclose(dec.numpy(), want.reshape(shape).numpy(), rtol=1e-4, atol=2e-6)
    if y is None:
        assert tuple(model.manifold2d(3, plot=False).shape) == (9,) + shape[1:]


# ------------------------------------------------------------------------------- 5. determinism, under the guards
@pytest.mark.parametrize("name", sorted(CASES))
def test_repeated_call_is_bit_identical_under_guards(gpu_device, name):
    """An ordinary call, then the same call with every caller-owned buffer the kernel indexes by observation as a view of exactly
    its B N C values with NaN behind it (x, per-image weights, loc_out), the shared weights likewise, and the workspace — of exactly
    the queried size, between two guard regions — holding 0xFF bytes: NaN wherever a float is read before it is written.  The
    same bits, all finite; the NaN behind loc_out and the workspace's guards untouched; no NaN left in loc_out."""
    case = Case(name)
    model, eng = flagged(case)
    n = case.b * case.n_obs
    loc0 = torch.full((case.b, case.n_obs), float("nan"), device="cuda")
    case.call(eng, loc_out=loc0)
    keys = sorted(model.state_dict())                   # (per tensor: the flat buffer's alignment padding is not under contract)

    def results(loc_):
        return [eng.grad_of(k).clone() for k in keys] + [eng.scalars.clone(), loc_.clone()]
    first = results(loc0)
    assert all(bool(torch.isfinite(t).all()) for t in first)

    need = int(wc.ivae_query(eng, case.b)())
    assert need == eng.ws.numel()
    view, guards = wc.guarded(need, "ones")
    wc.install(eng, view, need=need)
    buf = torch.full((n + wc.INPUT_GUARD,), float("nan"), device="cuda")
    loc = buf[:n].view(case.b, case.n_obs)
    kw = dict(loc_out=loc)
    if case.w_img is not None:
        kw["image_weights"] = wc.flush(case.w_img)
    if eng.pixel_weights is not None:
        eng.pixel_weights = wc.flush(eng.pixel_weights)
    eng.grad.fill_(float("nan"))
    case.call(eng, x=wc.flush(case.x), **kw)
    assert eng.ws is view
    guards()
    assert bool(torch.isnan(buf[n:]).all()), "loc_out: a write behind its B N C values"
    assert not bool(torch.isnan(loc).any()), "loc_out: an observation without a value"
    for what, a, b_ in zip(keys + ["scalars", "loc_out"], first, results(loc)):
        assert wc.same_bits(a, b_), "%s %s: differs under the guards (max %.3e)" % (name, what, (a - b_).abs().max().item())


# ------------------------------------------------------------------------------- 6. the partition of case b
def test_case_b_has_workgroups_that_start_and_end_on_a_tail_unit(gpu_device):
    """The kernel's partition restated (tests/_partition_cases.py): units of 16 rows, workgroup g of G = min(units, CUs) owns
    units [g units / G, (g + 1) units / G).  17 positions: two units per sample, the odd ones hold one valid row and 15 padding
    rows.  The case must put such a unit first in some workgroup, last in another, and have workgroups of one and of two units."""
    c = CASES["b_1d17_t_b200"]
    upb = (n_pos(c) + UNIT - 1) // UNIT
    units = c["b"] * upb
    G = min(units, torch.cuda.get_device_properties(0).multi_processor_count)
    ranges = [(g * units // G, (g + 1) * units // G) for g in range(G)]
    is_tail = lambda u: u % upb == upb - 1
    sizes = {hi - lo for lo, hi in ranges}
    print("units %d, grid %d, units per workgroup %s" % (units, G, sorted(sizes)))
    assert upb == 2 and units == 400
    assert any(is_tail(lo) for lo, hi in ranges), "no workgroup starts on a tail unit"
    assert any(is_tail(hi - 1) for lo, hi in ranges), "no workgroup ends on a tail unit"
    if G == 256:
        assert sizes == {1, 2}
        assert any(lo // upb != (hi - 1) // upb for lo, hi in ranges), "no sample boundary inside a workgroup"


# ------------------------------------------------------------------------------- 7. the workspace contract
def test_workspace_contract(gpu_device):
    """tests/_ws_contract.run_cell on the flagged 7 x 9 plan: the engine allocates what the query says, and on a workspace of
    exactly that size between guards, holding zeros, 0xFF bytes or noise, every result has the bits of the ordinary call."""
    case = Case("c_7x9_rts_b6")

    def make():
        model, eng = flagged(case)
        outs = dict(loc=torch.empty(case.b, case.n_obs, device="cuda"),
                    z_loc=torch.empty(case.b, model.z_dim, device="cuda"), z_scale=torch.empty(case.b, model.z_dim, device="cuda"))

        def call(inp):
            eng.loss_and_grads(inp["x"], inp["eps"], 1.0, z_out=(outs["z_loc"], outs["z_scale"]), loc_out=outs["loc"])
        return wc.engine_run(eng, dict(x=case.x.cuda(), eps=case.eps[0].cuda()), call, outs=outs,
                             workspaces={"ws": wc.ivae_query(eng, case.b)})
    need, secs = wc.run_cell("fused_any_size 7x9", make)
    print("workspace %s bytes, %.1f s" % (need, secs))


# ------------------------------------------------------------------------------- 8. trainer
def test_trainer_history(gpu_device):
    """SVItrainer(iVAE((7, 9), ...), fused_any_size=True): one epoch on the tail kernel; the loss history within the loss bar of
    the same trainer at fused=0."""
    c = CASES["c_7x9_rts_b6"]
    x = mc.case_data(dict(c, b=12))[0][..., 0].contiguous()
    hist = []
    for kw in (dict(fused_any_size=True), dict(fused=0)):
        loader = pv.utils.init_dataloader(x, batch_size=c["b"])
        model = pv.models.iVAE(c["dims"], 2, c["inv"], seed=1, device="cuda")
        tr = pv.trainers.SVItrainer(model, seed=1, **kw)
        assert tr.engine.uses_fused(c["b"]) is ("fused_any_size" in kw)
        tr.step(loader)
        torch.cuda.synchronize()
        hist.append(list(tr.loss_history["training_loss"]))
    print("trainer: fused_any_size %s, fused=0 %s" % tuple(hist))
    assert len(hist[0]) == 1 and np.isfinite(hist[0]).all()
    np.testing.assert_allclose(hist[0], hist[1], rtol=RTOL_ELBO)


# ------------------------------------------------------------------------------- 9. opt-in
def test_without_the_keyword_nothing_changes(gpu_device):
    """An engine built without the keyword on (7, 9) has the plan it had: the engine's `fused`, no new bit, the layered path,
    the layered workspace — for the default request, fused = 1 and fused = 0 alike, and the layered kernels' bits."""
    case = Case("c_7x9_rts_b6")
    out, need = [], []
    for kw in (dict(fused=0), dict(), dict(fused=1)):
        model, eng = case.engine(**kw)
        assert eng._plan_fused() == kw.get("fused", 2) and not eng._plan_flags() & _abi.PV_PLAN_FUSED_TAIL
        assert eng.uses_fused(case.b) is False
        case.call(eng)
        out.append(eng.grad.clone())
        need.append(int(eng.ws.numel()))
    assert torch.equal(out[0], out[1]) and torch.equal(out[0], out[2])
    assert need[0] == need[1] == need[2]
    _, eng = flagged(case)
    case.call(eng)
    assert int(eng.ws.numel()) != need[0]


# ------------------------------------------------------------------------------- 10. the engine's rule and the library's agree
SWEEP = {
    "7x9": (lambda: pv.models.iVAE((7, 9), 2, ["r", "t"], seed=1, device="cuda"), {}),
    "8x8": (lambda: pv.models.iVAE((8, 8), 2, ["r", "t"], seed=1, device="cuda"), {}),
    "1d17": (lambda: pv.models.iVAE((17,), 2, ["t"], seed=1, device="cuda"), {}),
    "1d32": (lambda: pv.models.iVAE((32,), 2, ["t"], seed=1, device="cuda"), {}),
    "7x9_cdim2": (lambda: pv.models.iVAE((7, 9), 2, ["r"], c_dim=2, seed=1, device="cuda"), {}),
    "7x9_72_40": (lambda: pv.models.iVAE((7, 9), 2, ["r"], hidden_dim_d=[72, 40], seed=1, device="cuda"), {}),
    "7x9_128_64": (lambda: pv.models.iVAE((7, 9), 2, ["r"], hidden_dim_d=[128, 64], seed=1, device="cuda"), {}),
    "7x9_three_layers": (lambda: pv.models.iVAE((7, 9), 2, ["r"], hidden_dim_d=[128, 128, 128], seed=1, device="cuda"), {}),
    "7x9_softplus": (lambda: pv.models.iVAE((7, 9), 2, ["r"], activation="softplus", seed=1, device="cuda"), {}),
    "7x9_gauss_nosig": (lambda: pv.models.iVAE((7, 9), 2, ["r"], sampler_d="gaussian", sigmoid_d=False, seed=1, device="cuda"), {}),
    "7x9_vanilla": (lambda: pv.models.iVAE((7, 9), 2, None, seed=1, device="cuda"), {}),
    "7x9_jivae": (lambda: pv.models.jiVAE((7, 9), 2, 3, ["r"], seed=1, device="cuda"), {}),
    "7x9_c3_no_channels_keyword": (lambda: pv.models.iVAE((7, 9), 2, ["r"], channels=3, seed=1, device="cuda"), {}),
    "7x9_c3": (lambda: pv.models.iVAE((7, 9), 2, ["r"], channels=3, seed=1, device="cuda"), dict(fused_channels=True)),
    "7x9_c7": (lambda: pv.models.iVAE((7, 9), 2, ["r"], channels=7, seed=1, device="cuda"), dict(fused_channels=True)),
    "7x9_c8": (lambda: pv.models.iVAE((7, 9), 2, ["r"], channels=8, seed=1, device="cuda"), dict(fused_channels=True)),
    "8x8_c3": (lambda: pv.models.iVAE((8, 8), 2, ["r"], channels=3, seed=1, device="cuda"), dict(fused_channels=True)),
    "7x9_c3_categorical": (lambda: pv.models.iVAE((7, 9), 2, ["r"], channels=3, sampler_d="categorical", sigmoid_d=False, seed=1,
                                                  device="cuda"), dict(fused_channels=True)),
}


@pytest.mark.parametrize("name", sorted(SWEEP))
def test_engine_rule_agrees_with_the_library(gpu_device, name):
    """IVAEEngine._any_size_on restates in Python where the library lets PV_PLAN_FUSED_TAIL take effect (pv_sdec_fused_tail); the
    engine needs the answer before it has a plan.  Over the architectures on either side of every condition the two must agree:
    the library's answer is read off the engine's own plan with fused = 1 and the bit forced on — the plan runs fused although
    its positions are no multiple of 16."""
    import ctypes as C
    make, kw = SWEEP[name]
    model = make()
    eng = model.engine(fused_any_size=True, **kw)
    p = _abi.pv_ivae_plan.from_buffer_copy(eng._plan(6))          # (a copy: the engine's own plan stays as it is)
    positions = int(np.prod(model.data_dim))
    p.fused = 1
    p.flags |= _abi.PV_PLAN_FUSED_TAIL
    lib_says = positions % UNIT != 0 and bool(_abi.lib().pv_ivae_uses_fused(C.byref(p)))
    print("%s: engine %s, library %s" % (name, eng._any_size_on(), lib_says))
    assert eng._any_size_on() is lib_says
    assert bool(eng._plan_flags() & _abi.PV_PLAN_FUSED_TAIL) is lib_says
