"""
_own_image_cases.py — the cases of the image-owning build of the bf16 decoder launch (tests/test_gpu_own_image_sums.py states the
method), their bars, and the engines, inputs and float64 reference both that file and tests/test_gpu_full_tile_loop.py run on.
"""
import ctypes as C

import numpy as np
import torch

from conftest import make_x

import pyroved_amd as pv
from pyroved_amd import _abi
from oracle import svi_oracle as orc
from _device import cus

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


def make(name, fold=True):
    data_dim, inv, kw, units = CASES[name]
    b = cus()                       # the fold needs batch == number of CUs
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


def inputs(name, model):
    data_dim = CASES[name][0]
    b = cus()
    x = make_x("rand", b, data_dim, seed=3)
    eps = torch.randn(b, model.z_dim, generator=torch.Generator().manual_seed(5))
    return x, eps


_REF = {}


def reference(name, model, x, eps):
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


def is_enc(key):
    return key.startswith("encoder_z.")
