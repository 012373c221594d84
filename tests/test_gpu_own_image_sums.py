"""
The image-owning build of the bf16 decoder launch (pv_sdec_fused_w8.hip, <true, lik, 2>: fused = 3 with the guide folded in, batch ==
number of CUs) keeps the image's five row sums {ll, d(phi), d(scale), d(tx), d(ty)} on chip: the log-likelihood in a running
register, the four transform-gradient sums from the column sums H_j, A_j, B_j of dpre0 the epilogue holds anyway — no per-row
outputs, no row-local coordinate backward.

Every case asserts which build runs, then compares the loss and every parameter gradient (the encoder-side ones are what these
sums feed: dL/d(head) never leaves the workspace, the head layer's bias gradient is its column sum and the weight gradient
dhead^T act) with the float64 oracle, and with the same engine with enc_fold = False — the per-row path in the per-sample launch.
Bars: the distance of the per-row form of this build (the commit before this file) to the float64 oracle was measured case by
case on an MI355X; every bar is <= 4x that and <= the mode's bars of tests/test_gpu_parity.py (loss 1e-4, gradients 3e-2).
"""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN, make_x

import pyroved_amd as pv
from pyroved_amd import _abi
from oracle import svi_oracle as orc

pytestmark = pytest.mark.gpu

MODE_LOSS_BAR, MODE_GRAD_BAR = 1e-4, 3e-2          # tests/test_gpu_parity.py: the bf16 mode against the fp32 oracle

# name: (data_dim, invariances, model / oracle keywords, units of 16 rows per workgroup)
CASES = {
    "a_1d16_t": ((16,), ["t"], {}, 1),                                       # tail only, coord_dim == 1 (only sum d0 live)
    "b_8x8_rts": ((8, 8), ["r", "t", "s"], {}, 4),                           # one partial tile, no tail, all four sums, sc != 1
    "c_12x12_rts": ((12, 12), ["r", "t", "s"], {}, 9),                       # one full tile + tail
    "d_12x12_r": ((12, 12), ["r"], {}, 9),                                   # phi only
    "e_12x12_rts_t2": ((12, 12), ["r", "t", "s"], dict(dx_prior=2.0, dy_prior=2.0), 9),   # |t| >~ sc |u|: the cancellation in A - t H
    "f_28x28_rt": ((28, 28), ["r", "t"], {}, 49),                            # the headline shape, one draw
}

# Bars per case: (loss, worst encoder-side gradient, worst decoder-side gradient) relative (L2 for tensors) to the float64 oracle, and
# the worst tensor's distance between the folded path and the enc_fold = False path.  Each is <= 4x what the per-row form of this
# build measured on an MI355X (comment: per-row form / the on-chip sums, same box and session) and <= the mode's bars.
BARS = {
    # loss 7.46e-6 / 7.46e-6, encoder 1.737e-4 / 1.737e-4, decoder 4.051e-3 / 4.051e-3, pair 8.90e-6 / 8.90e-6
    "a_1d16_t": (2.9e-5, 6.9e-4, 1.6e-2, 3.5e-5),
    # loss 9.58e-7 / 9.58e-7, encoder 1.150e-4 / 1.148e-4, decoder 2.970e-3 / 2.970e-3, pair 4.77e-5 / 4.68e-5
    "b_8x8_rts": (3.8e-6, 4.6e-4, 1.18e-2, 1.9e-4),
    # loss 1.145e-7 / 1.145e-7, encoder 2.002e-4 / 2.002e-4, decoder 3.413e-3 / 3.412e-3, pair 3.33e-5 / 3.71e-5
    "c_12x12_rts": (4.5e-7, 8.0e-4, 1.36e-2, 1.3e-4),
    # loss 7.05e-7 / 7.05e-7, encoder 6.706e-3 / 6.673e-3, decoder 4.707e-3 / 4.708e-3, pair 7.57e-5 / 8.41e-5
    "d_12x12_r": (2.8e-6, 2.68e-2, 1.88e-2, 3.0e-4),
    # loss 2.455e-6 / 2.530e-6 (enc_fold = False: 2.530e-6), encoder 1.179e-3 / 1.180e-3, decoder 2.897e-3 / 2.898e-3, pair 2.52e-5 / 2.55e-5
    "e_12x12_rts_t2": (9.8e-6, 4.7e-3, 1.15e-2, 1.0e-4),
    # loss 2.179e-6 / 2.179e-6, encoder 7.211e-3 / 7.213e-3, decoder 6.910e-3 / 6.910e-3, pair 2.30e-5 / 2.40e-5
    "f_28x28_rt": (8.7e-6, 2.88e-2, 2.76e-2, 9.2e-5),
}
assert all(b[0] <= MODE_LOSS_BAR and max(b[1:3]) <= MODE_GRAD_BAR for b in BARS.values())
# case e, encoder-side tensors: the per-row form's own distance to the float64 oracle; the on-chip sums must stay within 2x of it
# (the cancellation in A_j - tx H_j would show here first)
PARENT_E = {
    "encoder_z.fc_layers.0.weight": 6.061e-04,   # on-chip sums: 6.068e-04
    "encoder_z.fc_layers.0.bias": 6.131e-04,     # 6.138e-04
    "encoder_z.fc_layers.2.weight": 6.568e-04,   # 6.574e-04
    "encoder_z.fc_layers.2.bias": 6.603e-04,     # 6.609e-04
    "encoder_z.fc11.weight": 1.179e-03,          # 1.180e-03
    "encoder_z.fc11.bias": 1.159e-03,            # 1.160e-03
    "encoder_z.fc12.weight": 3.384e-04,          # 3.385e-04
    "encoder_z.fc12.bias": 3.400e-04,            # 3.401e-04
}


def rel_l2(a, b):
    a, b = a.double().flatten().cpu(), b.double().flatten().cpu()
    return ((a - b).norm() / b.norm().clamp_min(1e-300)).item()


def _batch():
    return torch.cuda.get_device_properties(0).multi_processor_count      # the fold needs batch == number of CUs


def _make(name, fold=True):
    data_dim, inv, kw, units = CASES[name]
    b = _batch()
    model = pv.models.iVAE(data_dim, 2, inv, seed=1, device="cuda", **kw)
    eng = model.engine(fused=3)
    eng.enc_fold = fold
    if units < 6:
        eng.dec_kernel = 2          # below the 8-wave kernel's size threshold (6 units per workgroup): forced, as test_gpu_bf16_emulated.py does
    p = eng._plan(b)
    folds = int(_abi.lib().pv_ivae_guide_folds(C.byref(p)))
    assert folds == (1 if fold else 0), (name, fold, folds)
    if fold:
        assert int(np.prod(data_dim)) // 16 == units and eng.uses_fused(b)
        if units < 6:
            assert p.dec_kernel == 2
        lib = _abi.lib()
        lib.pv_debug_decoder_kernel_name_fold.restype = C.c_char_p
        lib.pv_debug_decoder_kernel_name_fold.argtypes = [C.c_int, C.c_int]
        kname = lib.pv_debug_decoder_kernel_name_fold(1, 0).decode()
        assert "pv_sdec_w8_kernel<true, 0, 2>" in kname, kname
    return model, eng


def _inputs(name, model):
    data_dim = CASES[name][0]
    b = _batch()
    x = make_x("rand", b, data_dim, seed=3)
    eps = torch.randn(b, model.z_dim, generator=torch.Generator().manual_seed(5))
    return x, eps


_REF = {}


def _reference(name, model, x, eps):
    """float64 oracle on the model's initial parameters: computed once per case, shared, never modified"""
    if name not in _REF:
        data_dim, inv, kw, _ = CASES[name]
        n = torch.get_num_threads()
        torch.set_num_threads(16)
        try:
            cfg = orc.Config(data_dim=data_dim, latent_dim=2, invariances=inv, **kw)
            o = orc.SVIOracle({k: v.detach().cpu() for k, v in model.state_dict().items()}, cfg, dtype=torch.float64)
            out = o.loss_and_grads(x, eps)
            _REF[name] = (out["loss"].item(), {k: v.grad.detach().clone() for k, v in o.p.items()})
        finally:
            torch.set_num_threads(n)
    return _REF[name]


def _is_enc(key):
    return key.startswith("encoder_z.")


@pytest.mark.parametrize("name", sorted(CASES))
def test_on_chip_row_sums_vs_oracle_and_per_row_path(gpu_device, name):
    model, eng = _make(name)
    x, eps = _inputs(name, model)
    ref_loss, ref_g = _reference(name, model, x, eps)
    xg, eg = x.cuda(), eps.cuda()
    eng.loss_and_grads(xg, eg, step=False)
    torch.cuda.synchronize()
    grad0, sc0 = eng.grad.clone(), eng.scalars.clone()
    m2, e2 = _make(name, fold=False)
    e2.loss_and_grads(xg, eg, step=False)
    torch.cuda.synchronize()
    loss_bar, enc_bar, dec_bar, pair_bar = BARS[name]
    le = abs(sc0[0].item() - ref_loss) / abs(ref_loss)
    le2 = abs(e2.scalars[0].item() - ref_loss) / abs(ref_loss)
    rows = []
    for key in ref_g:
        g, g2 = eng.grad_of(key), e2.grad_of(key)
        rows.append((key, rel_l2(g, ref_g[key]), rel_l2(g2, ref_g[key]), rel_l2(g, g2)))
    print("\n[own-image-sums] %s: loss vs float64 %.3e (enc_fold=False %.3e)" % (name, le, le2))
    for key, a, c, d in rows:
        print("  %-42s vs float64 %.3e   enc_fold=False vs float64 %.3e   folded vs enc_fold=False %.3e" % (key, a, c, d))
    assert le < loss_bar and le2 < loss_bar, (name, le, le2, loss_bar)
    for key, a, c, d in rows:
        bar = enc_bar if _is_enc(key) else dec_bar
        assert a < bar, "%s: %s %.3e from float64 (bar %.1e)" % (name, key, a, bar)
        assert c < bar, "%s: %s (enc_fold=False) %.3e from float64 (bar %.1e)" % (name, key, c, bar)
        assert d < pair_bar, "%s: %s folded vs per-row path %.3e (bar %.1e)" % (name, key, d, pair_bar)
        if name in ("e_12x12_rts_t2",) and _is_enc(key):
            assert a <= 2.0 * PARENT_E[key], "%s: %s %.3e, the per-row form measured %.3e" % (name, key, a, PARENT_E[key])
    # bit-reproducible: the same call again, identical gradient buffer and scalars
    eng.loss_and_grads(xg, eg, step=False)
    torch.cuda.synchronize()
    assert torch.equal(grad0, eng.grad) and torch.equal(sc0, eng.scalars), name


@pytest.mark.parametrize("name", ["c_12x12_rts", "f_28x28_rt"])
def test_one_call_step_is_bit_identical_with_on_chip_sums(gpu_device, name):
    (m1, e1), (m2, e2) = _make(name), _make(name)
    x, _ = _inputs(name, m1)
    xg = x.cuda()
    gen = torch.Generator().manual_seed(9)
    for k in range(2):
        eps = torch.randn(_batch(), m1.z_dim, generator=gen).cuda()
        e1.loss_and_grads(xg, eps)
        s1 = e1.scalars.clone()
        e1.adam_step()
        hist = torch.zeros(4, device="cuda")
        e2.loss_and_grads(xg, eps, scalars_out=hist, step=True)
        torch.cuda.synchronize()
        assert torch.equal(s1, hist), (name, k)
        for what, a, b_ in (("params", e1.flat, e2.flat), ("m", e1.m, e2.m), ("v", e1.v, e2.v),
                            ("grad", e1.grad[:e1.n_flat], e2.grad[:e2.n_flat])):
            assert torch.equal(a, b_), (name, k, what, (a - b_).abs().max().item())
    assert float(e2.grad[:e2.n_flat].abs().sum()) == 0.0


def test_forward_only_launch_still_writes_rows(gpu_device):
    """want_grads=False with loc_out: the forward-only launch keeps its per-row outputs (evaluate and loc_out read them).  loc and
    the loss scalars against the values the commit before this file produced on an MI355X (tests/golden/own_sums_fwd_12x12_rts.npz)."""
    name = "c_12x12_rts"
    if _batch() != 256:
        pytest.skip("the recorded values are a batch of 256 (256 CUs)")
    model, eng = _make(name)
    x, eps = _inputs(name, model)
    loc = torch.empty(_batch(), 144, device="cuda")
    eng.loss_and_grads(x.cuda(), eps.cuda(), want_grads=False, loc_out=loc)
    torch.cuda.synchronize()
    gold = dict(np.load(os.path.join(GOLDEN, "own_sums_fwd_12x12_rts.npz"), allow_pickle=False))
    d_loc = float(np.abs(loc.cpu().numpy() - gold["loc"]).max())
    sc = eng.scalars.cpu().numpy()
    print("\n[own-image-sums] forward-only: max |loc - recorded| %.3e, scalars %s recorded %s" % (d_loc, sc, gold["scalars"]))
    assert np.array_equal(loc.cpu().numpy(), gold["loc"])
    assert np.array_equal(sc, gold["scalars"])
