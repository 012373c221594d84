"""
The full-tile loop of the image-owning bf16 decoder launch (pv_sdec_fused_w8.hip, build <true, lik, 4>): fused = 3 with the guide
folded in, batch == number of CUs, an image of 8 n or 8 n + 1 units of 16 pixels (n >= 1), two coordinates, no per-sample
weights.  It runs the arithmetic of the generic loop (build <true, lik, 2>) in the same order, so everything it produces must be
the SAME BYTES as with engine.full_tile_loop = False (PV_PLAN_GENERIC_TILE_LOOP): the four loss scalars, the flat gradient, and
— through the one-call step — the parameters and both Adam moments.

The continuous Bernoulli and Poisson builds are held to the same byte identity on the 12 x 12 shape; the Gaussian likelihood and
cd == 1 must stay on the generic loop.

Which loop ran is read back from the library (pv_debug_w8_last_fold_build: the build the last hosting launch dispatched).

Tolerances: none of its own.  Cases 1-4 are bit-identity; case 4 is also held to the bars tests/test_gpu_own_image_sums.py keeps for
f_28x28_rt against the float64 oracle (tests/_own_image_cases.py: reused, and the oracle result is that module's cached one); case 7 (cd == 1, routed to the
generic loop) to the bf16 mode's bars of tests/test_gpu_parity.py (loss 1e-4, gradients 3e-2).
"""
import ctypes as C

import numpy as np
import pytest
import torch

from conftest import make_x

import pyroved_amd as pv
from pyroved_amd import _abi
from oracle import svi_oracle as orc
import _own_image_cases as own
from _device import cus, last_fold_build
from _judge import rel_l2

pytestmark = pytest.mark.gpu

# name: (data_dim, invariances, units of 16 pixels per image, build the default engine must dispatch)
CASES = {
    "c1_12x12_rts": ((12, 12), ["r", "t", "s"], 9, 4),     # one full tile + tail
    "c2_16x24_rt": ((16, 24), ["r", "t"], 24, 4),          # three full tiles, no tail: tile-to-tile pointer advance
    "c3_20x20_rts": ((20, 20), ["r", "t", "s"], 25, 4),    # three tiles + tail
    "c4_28x28_rt": ((28, 28), ["r", "t"], 49, 4),          # the headline shape, one draw
    "c5_8x8": ((8, 8), ["r", "t", "s"], 4, 2),             # partial tile: generic loop
    "c6_1d16_t": ((16,), ["t"], 1, 2),                     # tail only, cd == 1: generic loop
    "c7_1d144_t": ((144,), ["t"], 9, 2),                   # cd == 1 with a full tile: routed to the generic loop
}
FULL = ["c1_12x12_rts", "c2_16x24_rt", "c3_20x20_rts", "c4_28x28_rt"]
# the other likelihoods' builds on case 1's shape: (model keywords, build the default engine must dispatch).  The Gaussian
# likelihood keeps the generic loop (its full-tile build would spill a register its generic build does not)
LIKS = {
    "continuous_bernoulli": (dict(sampler_d="continuous_bernoulli"), 4),
    "poisson_log": (dict(sampler_d="poisson_log", sigmoid_d=False), 4),
    "gaussian": (dict(sampler_d="gaussian"), 2),
}


def _make(name, full=True, **kw):
    data_dim, inv, units, _ = CASES[name]
    assert int(np.prod(data_dim)) // 16 == units
    model = pv.models.iVAE(data_dim, 2, inv, seed=1, device="cuda", **kw)
    eng = model.engine(fused=3)
    eng.full_tile_loop = full
    if units < 6:
        eng.dec_kernel = 2          # below the 8-wave kernel's size threshold: forced, as tests/_own_image_cases.py does
    p = eng._plan(cus())
    assert bool(p.flags & _abi.PV_PLAN_GENERIC_TILE_LOOP) == (not full)
    assert int(_abi.lib().pv_ivae_guide_folds(C.byref(p))) == 1 and eng.uses_fused(cus()), name
    return model, eng


def _inputs(name, model, seed=5):
    x = make_x("rand", cus(), CASES[name][0], seed=3)
    eps = torch.randn(cus(), model.z_dim, generator=torch.Generator().manual_seed(seed))
    return x.cuda(), eps.cuda()


def _run(name, full, **kw):
    """loss_and_grads once: (scalars, flat gradient, build dispatched, engine, model)"""
    model, eng = _make(name, full, **kw)
    xg, eg = _inputs(name, model)
    eng.loss_and_grads(xg, eg, step=False)
    torch.cuda.synchronize()
    return eng.scalars.clone(), eng.grad.clone(), last_fold_build(), eng, model


def _same_bytes(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.view(torch.int32), b.view(torch.int32))


@pytest.mark.parametrize("name", sorted(CASES))
def test_loss_and_grads_same_bytes_with_either_loop(gpu_device, name):
    want = CASES[name][3]
    sc1, g1, b1, eng, model = _run(name, True)
    sc0, g0, b0, _, _ = _run(name, False)
    print("\n[full-tile-loop] %s: build %d (default) / %d (PV_PLAN_GENERIC_TILE_LOOP), loss %.6f / %.6f, max |dgrad| %.3e"
          % (name, b1, b0, sc1[0].item(), sc0[0].item(), (g1 - g0).abs().max().item()))
    assert b1 == want, (name, "default engine dispatched build", b1)
    assert b0 == 2, (name, "PV_PLAN_GENERIC_TILE_LOOP dispatched build", b0)
    assert torch.isfinite(sc1).all() and torch.isfinite(g1).all() and float(g1.abs().sum()) > 0.0
    assert _same_bytes(sc1, sc0), (name, sc1.tolist(), sc0.tolist())
    assert _same_bytes(g1, g0), (name, (g1 - g0).abs().max().item())
    # two runs of the default loop: the same bytes
    xg, eg = _inputs(name, model)
    eng.loss_and_grads(xg, eg, step=False)
    torch.cuda.synchronize()
    assert last_fold_build() == want
    assert _same_bytes(sc1, eng.scalars) and _same_bytes(g1, eng.grad), name


@pytest.mark.parametrize("lik", sorted(LIKS))
def test_other_likelihoods_same_bytes_with_either_loop(gpu_device, lik):
    kw, want = LIKS[lik]
    name = "c1_12x12_rts"
    sc1, g1, b1, _, _ = _run(name, True, **kw)
    sc0, g0, b0, _, _ = _run(name, False, **kw)
    print("\n[full-tile-loop] %s %s: build %d / %d, loss %.6f / %.6f" % (name, lik, b1, b0, sc1[0].item(), sc0[0].item()))
    assert b1 == want and b0 == 2, (lik, b1, b0)
    assert torch.isfinite(sc1).all() and torch.isfinite(g1).all() and float(g1.abs().sum()) > 0.0
    assert _same_bytes(sc1, sc0) and _same_bytes(g1, g0), (lik, sc1.tolist(), sc0.tolist(), (g1 - g0).abs().max().item())


@pytest.mark.parametrize("name", FULL)
def test_one_call_step_same_bytes_with_either_loop(gpu_device, name):
    (m1, e1), (m0, e0) = _make(name, True), _make(name, False)
    xg, _ = _inputs(name, m1)
    gen = torch.Generator().manual_seed(9)
    for k in range(2):
        eps = torch.randn(cus(), m1.z_dim, generator=gen).cuda()
        h1, h0 = torch.zeros(4, device="cuda"), torch.zeros(4, device="cuda")
        e1.loss_and_grads(xg, eps, scalars_out=h1, step=True)
        torch.cuda.synchronize()
        assert last_fold_build() == 4, (name, k)
        e0.loss_and_grads(xg, eps, scalars_out=h0, step=True)
        torch.cuda.synchronize()
        assert last_fold_build() == 2, (name, k)
        assert _same_bytes(h1, h0), (name, k, h1.tolist(), h0.tolist())
        for what, a, b_ in (("params", e1.flat, e0.flat), ("m", e1.m, e0.m), ("v", e1.v, e0.v)):
            assert _same_bytes(a, b_), (name, k, what, (a - b_).abs().max().item())
    assert float(e1.m.abs().sum()) > 0.0


def test_headline_shape_vs_float64_oracle(gpu_device):
    """case 4 on the full-tile loop against the float64 oracle, at tests/test_gpu_own_image_sums.py's bars for f_28x28_rt (the same
    model, data and noise: tests/_own_image_cases.py's inputs and its cached oracle result)"""
    name = "f_28x28_rt"
    model, eng = own.make(name)
    assert eng.full_tile_loop
    x, eps = own.inputs(name, model)
    ref_loss, ref_g = own.reference(name, model, x, eps)
    eng.loss_and_grads(x.cuda(), eps.cuda(), step=False)
    torch.cuda.synchronize()
    assert last_fold_build() == 4
    loss_bar, enc_bar, dec_bar, _ = own.BARS[name]
    le = abs(eng.scalars[0].item() - ref_loss) / abs(ref_loss)
    print("\n[full-tile-loop] %s: loss vs float64 %.3e (bar %.1e)" % (name, le, loss_bar))
    assert le < loss_bar, (le, loss_bar)
    for key in ref_g:
        d = rel_l2(eng.grad_of(key), ref_g[key])
        bar = enc_bar if own.is_enc(key) else dec_bar
        print("  %-42s vs float64 %.3e (bar %.1e)" % (key, d, bar))
        assert d < bar, (key, d, bar)


def test_cd1_with_full_tiles_vs_oracle(gpu_device):
    """case 7: one coordinate, nine units — runs on the generic loop and agrees with the fp32 oracle at the bf16 mode's bars"""
    name = "c7_1d144_t"
    data_dim, inv, _, _ = CASES[name]
    sc, _, build, eng, model = _run(name, True)
    assert build == 2
    x = make_x("rand", cus(), data_dim, seed=3)
    eps = torch.randn(cus(), model.z_dim, generator=torch.Generator().manual_seed(5))
    cfg = orc.Config(data_dim=data_dim, latent_dim=2, invariances=inv)
    o = orc.SVIOracle({k: v.detach().cpu() for k, v in model.state_dict().items()}, cfg)
    out = o.loss_and_grads(x, eps)
    ref_loss = out["loss"].item()
    le = abs(sc[0].item() - ref_loss) / abs(ref_loss)
    worst = max(rel_l2(eng.grad_of(k), v.grad) for k, v in o.p.items())
    print("\n[full-tile-loop] %s: loss vs oracle %.3e, worst gradient %.3e" % (name, le, worst))
    assert le < own.MODE_LOSS_BAR and worst < own.MODE_GRAD_BAR, (le, worst)
