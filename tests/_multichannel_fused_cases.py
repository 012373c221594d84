"""
_multichannel_fused_cases.py — the case table of tests/test_gpu_multichannel_fused.py: multi-channel models on the fused f32
decoder kernel (model.engine(fused_channels=True)).  The entries have the form of tests/_multichannel_cases.CASES, so that
module's model_kwargs / case_config / case_data (seed 0: the data first, then the eps draws) apply to them unchanged.  Every
case has hidden sizes [128, 128] and tanh — the decoder the kernel is written for — and a number of grid positions that is a
multiple of 16; each is the smallest shape that reaches a distinct part of the kernel (a unit = 16 rows = 16 positions of one
image; the kernel runs min(units, 256) workgroups of eight waves, one unit per wave and tile).
"""

CASES = {
    # 24 units, one per workgroup: a tile of one active wave, seven idle
    "f01_8x8_rts_c2_b6": dict(dims=(8, 8), inv=["r", "t", "s"], C=2, b=6),
    # one coordinate
    "f02_1d32_t_c4_b5_gauss_nosig": dict(dims=(32,), inv=["t"], C=4, b=5, sampler="gaussian", sigmoid_d=False),
    # counts: the normaliser pair, the rate in loc_out
    "f03_8x8_r_c3_b6_poisson": dict(dims=(8, 8), inv=["r"], C=3, b=6, sampler="poisson_log", sigmoid_d=False),
    # the concatenated latent input [z | y]
    "f04_8x8_rts_c2_cdim3_b6_cbern": dict(dims=(8, 8), inv=["r", "t", "s"], C=2, b=6, c_dim=3, sampler="continuous_bernoulli"),
    # 784 units on 256 workgroups: 3 - 4 units each, images split over workgroups (the dL/d(hz) slots of several workgroups per image)
    "f05_28x28_rt_c3_b16_gauss": dict(dims=(28, 28), inv=["r", "t"], C=3, b=16, sampler="gaussian"),
    # 2 560 units, 10 per workgroup: a full tile, then a 2-unit tile, an image boundary inside a workgroup; the widest C
    "f06_16x16_r_c8_b160": dict(dims=(16, 16), inv=["r"], C=8, b=160),
    # the odd instances
    "f07_8x8_r_c5_b4": dict(dims=(8, 8), inv=["r"], C=5, b=4),
    "f08_8x8_r_c7_b4": dict(dims=(8, 8), inv=["r"], C=7, b=4),
}
CASE1, CASE5, CASE6 = "f01_8x8_rts_c2_b6", "f05_28x28_rt_c3_b16_gauss", "f06_16x16_r_c8_b160"
