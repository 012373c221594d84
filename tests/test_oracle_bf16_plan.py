"""
The bf16 rounding plan of the oracle's spatial decoder (oracle/bf16_plan.py) on its own, CPU only: with the plan unset the
oracle is unchanged, with every rounding off the restated backward is autograd's, the bf16 helper is round-to-nearest-even,
the restated work partition is the kernel's, and the per-workgroup partials add up to the gradient.
"""
import dataclasses
import glob
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN, load_golden, make_x, meta_of, check_digest

import pyroved_amd as pv
from oracle import svi_oracle as orc
from oracle import bf16_plan as bp

STEP_CASES = sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(GOLDEN, "ivae_*.npz"))
                    if not p.endswith("_fwd.npz"))


def _case(name, dtype=torch.float32):
    gold = load_golden(name)
    meta = meta_of(gold)
    model = pv.models.iVAE(meta["data_dim"], meta["latent_dim"], meta["invariances"], seed=1, device="cpu")
    cfg = orc.Config(data_dim=meta["data_dim"], latent_dim=meta["latent_dim"], invariances=meta["invariances"])
    x = make_x(meta["xkind"], meta["batch"], meta["data_dim"])
    return model.state_dict(), cfg, x, torch.from_numpy(gold["s0.eps"]), meta["beta"]


def _loss_and_grads(params, cfg, x, eps, beta, dtype=torch.float32):
    o = orc.SVIOracle(params, cfg, dtype=dtype)
    out = o.loss_and_grads(x, eps, beta)
    return out["loss"].detach(), {k: v.grad for k, v in o.p.items()}


@pytest.fixture()
def threads8():
    n = torch.get_num_threads()
    torch.set_num_threads(8)
    try:
        yield
    finally:
        torch.set_num_threads(n)


@pytest.mark.parametrize("name", STEP_CASES)
def test_plan_unset_matches_the_reference(threads8, name):
    """Config.bf16_plan unset (the default) leaves the oracle as it is: the first step's loss and every gradient on what the
    reference's own code recorded (the tolerances of tests/test_oracle_golden.py), and a plan given and then removed
    (dataclasses.replace) computes the same bits as the default Config."""
    params, cfg, x, eps, beta = _case(name)
    gold = load_golden(name)
    l0, g0 = _loss_and_grads(params, cfg, x, eps, beta)
    np.testing.assert_allclose(l0.item(), float(gold["s0.loss"]), rtol=2e-6)
    for k, g in g0.items():
        check_digest(g, gold, "s0.grad." + k, rtol=2e-4, atol=1e-7, what=name)
    off = dataclasses.replace(dataclasses.replace(cfg, bf16_plan=bp.Bf16Plan()), bf16_plan=None)
    l1, g1 = _loss_and_grads(params, off, x, eps, beta)
    assert torch.equal(l0, l1) and all(torch.equal(g0[k], g1[k]) for k in g0)


@pytest.mark.parametrize("kernel", ["w8", "w4"])
@pytest.mark.parametrize("name", ["ivae_8x8_rts_b6", "ivae_1d16_t_b5", "ivae_28x28_r_b32_blobs"])
def test_restated_backward_is_autograd_without_rounding(name, kernel):
    """With every rounding off (exact=True) the plan's forward is the plain decoder and its explicit backward — scales carried
    and removed, signs, the per-workgroup partials and their sum — must equal float64 autograd of the plain oracle."""
    params, cfg, x, eps, beta = _case(name)
    l0, g0 = _loss_and_grads(params, cfg, x, eps, beta, torch.float64)
    plan = bp.Bf16Plan(kernel=kernel, exact=True, cus=7)
    l1, g1 = _loss_and_grads(params, dataclasses.replace(cfg, bf16_plan=plan), x, eps, beta, torch.float64)
    assert abs(l1.item() - l0.item()) <= 1e-12 * abs(l0.item())
    for k in g0:
        err = ((g1[k] - g0[k]).norm() / g0[k].norm()).item()
        assert err < 1e-11, (k, err)


def _bf16_int_reference(x: np.ndarray) -> np.ndarray:
    """Round-to-nearest-even fp32 -> bf16 on the bit pattern: add 0x7FFF + the kept part's lsb, truncate (finite inputs)."""
    u = x.astype(np.float32).view(np.uint32).astype(np.uint64)
    lsb = (u >> 16) & 1
    r = ((u + 0x7FFF + lsb) & 0xFFFF0000).astype(np.uint32)
    return r.view(np.float32)


def test_bf16_helper_is_round_to_nearest_even():
    ulp = 2.0 ** -7                                               # bf16 spacing in [1, 2)
    specials = [1.0 + ulp / 2, 1.0 + 3 * ulp / 2,                 # ties: to the even neighbour, down and up
                -(1.0 + ulp / 2), -(1.0 + 3 * ulp / 2),
                1.0 + ulp / 2 + 2.0 ** -23, 1.0 + ulp / 2 - 2.0 ** -23,
                0.0, -0.0,
                1e-40, -1e-40, 2.0 ** -149, 2.0 ** -126 * (1 - 2.0 ** -8),    # fp32 subnormals
                3.3895313892515355e38, -3.3895313892515355e38,    # the largest bf16
                3.3961e38, 3.4e38, -3.39e38]                      # near it: up to fp32 max
    g = torch.Generator().manual_seed(0)
    rnd = torch.randn(20000, generator=g) * torch.exp2(torch.randint(-60, 60, (20000,), generator=g).float())
    ties = (torch.randint(0, 1 << 16, (4000,), generator=g).to(torch.int32) << 16 | 0x8000).view(torch.float32)
    x = torch.cat([torch.tensor(specials, dtype=torch.float32), rnd, ties[torch.isfinite(ties)]])
    got = bp.bf16(x.double())
    ref = torch.from_numpy(_bf16_int_reference(x.numpy())).double()
    fin = torch.isfinite(ref)
    assert torch.equal(got[fin], ref[fin])
    assert torch.equal(torch.signbit(got[fin]), torch.signbit(ref[fin]))      # -0 stays -0
    assert torch.isinf(got[~fin]).all() and torch.equal(torch.signbit(got[~fin]), torch.signbit(ref[~fin]))
    # from the fp32 value, not from float64: a float64 just above an fp32 tie rounds to fp32 first (double rounding)
    t = torch.tensor([1.0 + 2.0 ** -8 + 2.0 ** -40], dtype=torch.float64)
    assert bp.bf16(t).item() == 1.0


@pytest.mark.parametrize("units,grid", [(12544, 256), (6272, 256), (25088, 256), (50176, 256), (1536, 256), (3072, 256),
                                        (392, 256), (12, 12), (5, 5), (1, 1), (1568, 256), (12544, 304), (999, 77)])
def test_partition_covers_units_and_flags_tails(units, grid):
    """u_lo = g units / G (`u_lo` in pv_sdec_w8_kernel, pv_sdec_fused_w8.hip): the ranges tile [0, units) in order without gaps or overlaps, and a range
    of 8 n + 1 units (and only such a range) ends with a column-parallel tail (`has_tail`, same kernel)."""
    parts = bp.partition(units, grid)
    assert len(parts) == grid and parts[0][0] == 0 and parts[-1][1] == units
    for (lo, hi, tail), nxt in zip(parts, parts[1:] + [(units, None, None)]):
        assert hi == nxt[0] and hi >= lo
        assert tail == ((hi - lo) % 8 == 1)
    n = [hi - lo for lo, hi, _ in parts]
    assert max(n) - min(n) <= 1
    if (units, grid) == (12544, 256):            # C2 batch 256: 49 units each, six 8-wave tiles + a tail everywhere
        assert set(n) == {49} and all(t for _, _, t in parts)
    if (units, grid) == (6272, 256):             # C1 batch 128: 24 / 25 units, the tail in half the workgroups
        assert set(n) == {24, 25} and sum(t for _, _, t in parts) == 128
    if (units, grid) == (1536, 256):             # 16x16 batch 256: whole tiles... of 6 units, no tail
        assert not any(t for _, _, t in parts)
    assert bp.grid_of(units, grid) == min(units, grid)


@pytest.mark.parametrize("name,cus", [("ivae_28x28_r_b32_blobs", 256), ("ivae_8x8_rts_b6", 3), ("ivae_1d16_t_b5", 2)])
def test_partials_add_up_to_the_gradient(name, cus):
    """Records unrounded: the sum of the explicit per-workgroup partials is autograd's gradient of the emulated ELBO to float64
    rounding; rounded, it differs from it by at most 2^-8 of sqrt(sum of the partials' squared norms)."""
    params, cfg, x, eps, beta = _case(name)
    plan = bp.Bf16Plan(kernel="w8", cus=cus, round_records=False)
    _, g = _loss_and_grads(params, dataclasses.replace(cfg, bf16_plan=plan), x, eps, beta, torch.float64)
    units = x.numel() // 16
    assert plan.partials["W1"].shape[0] == bp.grid_of(units, cus)
    for k, key in (("W1", "decoder.fc_layers.0.weight"), ("W2", "decoder.fc_layers.2.weight")):
        parts = plan.partials[k]
        s = sum(parts[i] for i in range(parts.shape[0]))
        assert ((s - g[key]).norm() / g[key].norm()).item() < 1e-13, k
        r = plan.__class__(kernel="w8", cus=cus).record_sum(parts, k)
        scale = parts.pow(2).sum().sqrt()
        assert (r - g[key]).norm() <= 2.0 ** -8 * scale, k
        assert not torch.equal(r, g[key])          # the records do round
