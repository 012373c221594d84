"""
How the record blocks of the step's closing launch (pv_rec_wgrad_kernel; pv_sdec_fused.h: the reducing bodies) end: one LDS exchange,
every thread of the block finalising its share of the elements, Adam's operands requested behind the last batch of records.

The closing launch with Adam in its record blocks is taken by the one-call step (loss_and_grads(..., step=True)) at batch ==
number of CUs only, so every case runs at that batch.  Which launch closed the step is read back from the library
(pv_debug_rec_wgrad_launches: launches of pv_rec_wgrad_kernel so far, and those of them whose record blocks carried Adam).

Tolerances: none.  The reference is the two-call path — loss_and_grads() + adam_step(), whose separate Adam launch
(pv_adam_kernel) is a different kernel from the one under test — and the per-element arithmetic is the same in the same order:
parameters and both moments must be the SAME BYTES, and the one-call step must leave the gradient buffer all zeros.

Cases: 4 x 4 images (one unit of 16 pixels: the hosting launch's workgroups are tail only) and 12 x 12 (nine units: one full tile
plus the tail), invariances ['r', 't'], on fused = 3 (packed bf16 records: 64 matrix blocks, two elements per thread) and fused = 2
(fp32 lane-native records: 128 matrix blocks, one element per thread); in both formats the vectors' 641 floats take three blocks of
256 elements, the last one partial (129 elements: threads 129 .. 255 have no element, threads 33 .. 63 of slice 0 sum a chunk
no element of which exists).  The edge case adds what moves that edge: one coordinate ((16,) with ['t']: the record's second
coordinate column has no parameter, so 128 threads inside the vector blocks have no element either) and latent_dim = 3 (a head of
8 outputs, an fc_latent of 4 inputs: other tile counts behind the record blocks).
"""
import ctypes as C

import pytest
import torch

from conftest import make_x

import pyroved_amd as pv
from pyroved_amd import _abi
from _device import cus

pytestmark = pytest.mark.gpu

# name: (data_dim, invariances, latent_dim, fused)
CASES = {
    "4x4_rt_f3": ((4, 4), ["r", "t"], 2, 3),
    "4x4_rt_f2": ((4, 4), ["r", "t"], 2, 2),
    "12x12_rt_f3": ((12, 12), ["r", "t"], 2, 3),
    "12x12_rt_f2": ((12, 12), ["r", "t"], 2, 2),
    "edge_1d16_t_z3_f3": ((16,), ["t"], 3, 3),
}
EDGE = "edge_1d16_t_z3_f3"
STEPS = 3


def _launches():
    """(launches of pv_rec_wgrad_kernel so far, those with Adam in the record blocks)"""
    lib = _abi.lib()
    lib.pv_debug_rec_wgrad_launches.restype = C.c_uint64
    lib.pv_debug_rec_wgrad_launches.argtypes = []
    n = int(lib.pv_debug_rec_wgrad_launches())
    return n & 0xffffffff, n >> 32


def _make(name):
    data_dim, inv, latent, fused = CASES[name]
    model = pv.models.iVAE(data_dim, latent, inv, seed=1, device="cuda")
    eng = model.engine(fused=fused)
    units = 1
    for d in data_dim:
        units *= d
    if fused == 3 and units // 16 < 6:
        eng.dec_kernel = 2          # below the 8-wave kernel's size threshold: forced, as tests/_own_image_cases.py does
    assert eng.uses_fused(cus()), name
    return model, eng


def _inputs(name, model):
    x = make_x("rand", cus(), CASES[name][0], seed=3).cuda()
    gen = torch.Generator().manual_seed(9)
    eps = [torch.randn(cus(), model.z_dim, generator=gen).cuda() for _ in range(STEPS)]
    return x, eps


def _same_bytes(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.view(torch.int32), b.view(torch.int32))


def _one_call(name):
    """STEPS one-call steps from the initial state; asserts that each closed with pv_rec_wgrad_kernel, Adam in its record blocks"""
    model, eng = _make(name)
    x, eps = _inputs(name, model)
    hist = []
    for k in range(STEPS):
        n0, a0 = _launches()
        h = torch.zeros(4, device="cuda")
        eng.loss_and_grads(x, eps[k], scalars_out=h, step=True)
        torch.cuda.synchronize()
        n1, a1 = _launches()
        assert (n1 - n0, a1 - a0) == (1, 1), (name, k, "the one-call step did not close with pv_rec_wgrad_kernel + Adam", n1 - n0, a1 - a0)
        assert float(eng.grad[:eng.n_flat].abs().sum()) == 0.0, (name, k, "gradient slots not zeroed")
        hist.append(h)
    return model, eng, hist


_TWO = {}


def _two_call(name):
    """the reference: STEPS steps of loss_and_grads() + adam_step() from the same state — computed once per case, shared, not modified"""
    if name not in _TWO:
        model, eng = _make(name)
        x, eps = _inputs(name, model)
        hist = []
        for k in range(STEPS):
            _, a0 = _launches()
            eng.loss_and_grads(x, eps[k])
            hist.append(eng.scalars.clone())
            eng.adam_step()
            torch.cuda.synchronize()
            assert _launches()[1] == a0, (name, k, "the two-call path must not run Adam in the record blocks")
        _TWO[name] = (model, eng, hist)
    return _TWO[name]


@pytest.mark.parametrize("name", sorted(CASES))
def test_one_call_step_matches_separate_adam(gpu_device, name):
    """(a) three one-call steps against three steps of loss_and_grads + adam_step: parameters, exp_avg, exp_avg_sq byte for byte"""
    _, e2, h2 = _two_call(name)
    _, e1, h1 = _one_call(name)
    assert e1.adam_t == e2.adam_t == STEPS
    for k in range(STEPS):
        assert _same_bytes(h1[k], h2[k]), (name, k, h1[k].tolist(), h2[k].tolist())
    for what, a, b in (("params", e1.flat, e2.flat), ("exp_avg", e1.m, e2.m), ("exp_avg_sq", e1.v, e2.v)):
        diff = (a - b).abs().max().item()
        print("\n[record-finalise] %s %s: max |one-call - two-call| %.3e" % (name, what, diff))
        assert _same_bytes(a, b), (name, what, diff)
    assert float(e1.m.abs().sum()) > 0.0 and torch.isfinite(e1.flat).all()
    assert float(e1.grad[:e1.n_flat].abs().sum()) == 0.0


@pytest.mark.parametrize("name", ["12x12_rt_f3", "12x12_rt_f2"])
def test_one_call_step_twice_same_bytes(gpu_device, name):
    """(b) the steps run twice from the same state: the same bytes"""
    _, e1, h1 = _one_call(name)
    _, e2, h2 = _one_call(name)
    for k in range(STEPS):
        assert _same_bytes(h1[k], h2[k]), (name, k)
    for what, a, b in (("params", e1.flat, e2.flat), ("exp_avg", e1.m, e2.m), ("exp_avg_sq", e1.v, e2.v)):
        assert _same_bytes(a, b), (name, what, (a - b).abs().max().item())


def test_partial_vector_block_updates(gpu_device):
    """(c) the vectors' last block is partial and, with one coordinate, the record's second coordinate column has no parameter: the
    updates of the output bias, the coordinate layer's weight, the output weight and both hidden biases equal the two-call path's,
    tensor by tensor, and every one of them moved"""
    m2, e2, _ = _two_call(EDGE)
    m1, e1, _ = _one_call(EDGE)
    p0 = pv.models.iVAE(CASES[EDGE][0], CASES[EDGE][2], CASES[EDGE][1], seed=1, device="cpu").state_dict()
    s1, s2 = m1.state_dict(), m2.state_dict()
    keys = [k for k in s1 if k.startswith("decoder.") and s1[k].numel() < 128 * 128 and "fc_latent" not in k and k != "decoder.coord_latent.fc_coord.bias"]
    assert "decoder.out.bias" in keys and "decoder.out.weight" in keys and "decoder.coord_latent.fc_coord.weight" in keys
    assert sum(k.startswith("decoder.fc_layers") and k.endswith("bias") for k in keys) == 2, keys
    assert s1["decoder.coord_latent.fc_coord.weight"].shape == (128, 1)
    for k in keys:
        off, n = e1._layout[k], s1[k].numel()
        for what, a, b in (("param", e1.flat, e2.flat), ("exp_avg", e1.m, e2.m), ("exp_avg_sq", e1.v, e2.v)):
            assert _same_bytes(a[off:off + n], b[off:off + n]), (k, what)
        assert _same_bytes(s1[k].detach().contiguous(), s2[k].detach().contiguous()), k
        assert ((s1[k].detach().cpu() - p0[k]).abs() > 0).all(), (k, "an element was not updated")
