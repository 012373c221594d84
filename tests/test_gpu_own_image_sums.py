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
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN

import _own_image_cases as own
from _device import cus
from _judge import rel_l2

pytestmark = pytest.mark.gpu

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


@pytest.mark.parametrize("name", sorted(own.CASES))
def test_on_chip_row_sums_vs_oracle_and_per_row_path(gpu_device, name):
    model, eng = own.make(name)
    x, eps = own.inputs(name, model)
    ref_loss, ref_g = own.reference(name, model, x, eps)
    xg, eg = x.cuda(), eps.cuda()
    eng.loss_and_grads(xg, eg, step=False)
    torch.cuda.synchronize()
    grad0, sc0 = eng.grad.clone(), eng.scalars.clone()
    m2, e2 = own.make(name, fold=False)
    e2.loss_and_grads(xg, eg, step=False)
    torch.cuda.synchronize()
    loss_bar, enc_bar, dec_bar, pair_bar = own.BARS[name]
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
        bar = enc_bar if own.is_enc(key) else dec_bar
        assert a < bar, "%s: %s %.3e from float64 (bar %.1e)" % (name, key, a, bar)
        assert c < bar, "%s: %s (enc_fold=False) %.3e from float64 (bar %.1e)" % (name, key, c, bar)
        assert d < pair_bar, "%s: %s folded vs per-row path %.3e (bar %.1e)" % (name, key, d, pair_bar)
        if name in ("e_12x12_rts_t2",) and own.is_enc(key):
            assert a <= 2.0 * PARENT_E[key], "%s: %s %.3e, the per-row form measured %.3e" % (name, key, a, PARENT_E[key])
    # bit-reproducible: the same call again, identical gradient buffer and scalars
    eng.loss_and_grads(xg, eg, step=False)
    torch.cuda.synchronize()
    assert torch.equal(grad0, eng.grad) and torch.equal(sc0, eng.scalars), name


@pytest.mark.parametrize("name", ["c_12x12_rts", "f_28x28_rt"])
def test_one_call_step_is_bit_identical_with_on_chip_sums(gpu_device, name):
    (m1, e1), (m2, e2) = own.make(name), own.make(name)
    x, _ = own.inputs(name, m1)
    xg = x.cuda()
    gen = torch.Generator().manual_seed(9)
    for k in range(2):
        eps = torch.randn(cus(), m1.z_dim, generator=gen).cuda()
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
    if cus() != 256:
        pytest.skip("the recorded values are a batch of 256 (256 CUs)")
    model, eng = own.make(name)
    x, eps = own.inputs(name, model)
    loc = torch.empty(cus(), 144, device="cuda")
    eng.loss_and_grads(x.cuda(), eps.cuda(), want_grads=False, loc_out=loc)
    torch.cuda.synchronize()
    gold = dict(np.load(os.path.join(GOLDEN, "own_sums_fwd_12x12_rts.npz"), allow_pickle=False))
    d_loc = float(np.abs(loc.cpu().numpy() - gold["loc"]).max())
    sc = eng.scalars.cpu().numpy()
    print("\n[own-image-sums] forward-only: max |loc - recorded| %.3e, scalars %s recorded %s" % (d_loc, sc, gold["scalars"]))
    assert np.array_equal(loc.cpu().numpy(), gold["loc"])
    assert np.array_equal(sc, gold["scalars"])
