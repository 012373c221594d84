"""
Multi-channel models — iVAE(..., channels=C) — where no GPU is needed: the reference (oracle.svi_oracle, Config(channels=C))
against a restated C-output decoder at C = 1 and 3 and under a permutation of the channels, what the constructors build and refuse, plan validation and
workspace sizes through the library's queries (host arithmetic), and the condition the GPU step tests' parameter check rests on
(near-zero gradient entries below 1 % per tensor, with the reference alone).
"""
import ctypes as C
import os
import re

import pytest
import torch
import torch.nn.functional as F

from conftest import ROOT

import pyroved_amd as pv
from pyroved_amd import _abi
from pyroved_amd.engine import UnsupportedModel
from pyroved_amd.nets import fcEncoderNet, sDecoderNet, fcDecoderNet, convEncoderNet
from pyroved_amd.utils import set_deterministic_mode
from oracle import svi_oracle as orc
import _multichannel_cases as mc
from _judge import ILL_SHARE, near_zero_share, state
from _plan_kit import _plan, _vanilla_plan


# ------------------------------------------------------------------------------- the reference
def config(inv, C=1, **kw):
    return orc.Config(data_dim=(8, 8), latent_dim=2, invariances=inv, channels=C, **kw)


def restated_decoder(p, cfg, C):
    """The C-output decoder restated next to the oracle's, as a user-defined decoder over the parameter dict p: the
    single-channel trunk up to the last hidden layer, then the head — Linear(H, C) per (sample, position) row, or
    Linear(H, positions * C) for the vanilla decoder —, the sigmoid per value, rows flattened channel-last to (B, positions * C)."""
    act = orc._ACT[cfg.activation]

    def head(h, b):
        out = torch.sigmoid(F.linear(h, p["decoder.out.weight"], p["decoder.out.bias"]))
        assert out.shape[-1] == (C if cfg.coord > 0 else cfg.n_pix * C)
        return out.reshape(b, -1)

    def spatial(x_coord, z):
        b, n = x_coord.shape[:2]
        h_x = F.linear(x_coord.reshape(b * n, -1), p["decoder.coord_latent.fc_coord.weight"],
                       p["decoder.coord_latent.fc_coord.bias"]).reshape(b, n, -1)
        h = torch.tanh((h_x + F.linear(z, p["decoder.coord_latent.fc_latent.weight"]).unsqueeze(1)).reshape(b * n, -1))
        return head(orc._fc_stack(p, "decoder.fc_layers", cfg.n_hidden_d, act, h), b)

    def vanilla(z):
        return head(orc._fc_stack(p, "decoder.fc_layers", cfg.n_hidden_d, act, z), z.shape[0])
    return spatial if cfg.coord > 0 else vanilla


def test_reference_at_one_channel_is_the_plain_oracle():
    """8x8 rts, B = 6, float64: loss, the three terms and every gradient to 1e-12 — spatial and vanilla decoder.  The
    plain oracle on (B, 8, 8) against the C-output decoder restated above at C = 1 on (B, 8, 8, 1); and, the same way, the
    oracle's own three-channel decoder against that restatement at C = 3.  Then decode under a transform."""
    for inv in (["r", "t", "s"], None):
        for Cn in (1, 3):
            model = pv.models.iVAE((8, 8), 2, inv, channels=Cn, seed=1, device="cpu")
            cfg = config(inv, Cn)
            p = {k: v.double().requires_grad_(True) for k, v in state(model).items()}
            g = torch.Generator().manual_seed(0)
            x = mc.images(g, 6, (8, 8), Cn).double()
            assert x.shape == (6, 8, 8, Cn)
            eps = torch.randn(6, cfg.z_dim, generator=g).double()
            plain = orc.elbo(p, cfg, x[..., 0] if Cn == 1 else x, eps)
            assert plain["loc"].shape == ((6, 8, 8) if Cn == 1 else (6, 8, 8, Cn))
            rest = orc.elbo(p, config(inv, custom_decoder=restated_decoder(p, cfg, Cn)), x, eps)
            for k in ("loss", "ll", "logpz", "logqz"):
                torch.testing.assert_close(rest[k], plain[k], rtol=1e-12, atol=1e-12)
            grads = [torch.autograd.grad(o["loss"], list(p.values())) for o in (rest, plain)]
            for k, gr, gp in zip(p, *grads):
                torch.testing.assert_close(gr, gp, rtol=1e-12, atol=1e-12, msg=k)
            z = torch.randn(3, 2, generator=g).double()
            o = orc.SVIOracle(state(model), cfg, dtype=torch.float64)
            dec = o.decode(z, angle=0.3, shift=[0.1, -0.2], scale=1.2)
            assert dec.shape == ((3, 8, 8) if Cn == 1 else (3, 8, 8, Cn))
            if inv:
                t = lambda v: torch.tensor(v, dtype=torch.float64)
                xc = orc.transform_coordinates(o.grid.unsqueeze(0), t([0.3]), t([[0.1, -0.2]]), t([1.2]))
                want = restated_decoder(o.p, cfg, Cn)(xc.expand(3, -1, -1), z)
            else:
                want = restated_decoder(o.p, cfg, Cn)(z)
            torch.testing.assert_close(dec.reshape(3, -1), want.detach(), rtol=1e-12, atol=1e-12)


def test_channel_permutation_permutes_the_gradients():
    """Permuting the channels of x together with the rows of decoder.out.* and the matching encoder input columns leaves the
    loss unchanged and permutes the gradients — for the spatial and the vanilla decoder."""
    Cn, perm = 3, [2, 0, 1]
    for inv in (["r", "t", "s"], None):
        model = pv.models.iVAE((8, 8), 2, inv, channels=Cn, seed=1, device="cpu")
        g = torch.Generator().manual_seed(0)
        x = mc.images(g, 6, (8, 8), Cn)
        eps = torch.randn(6, model.z_dim, generator=g)
        sd = state(model)
        o = orc.SVIOracle(sd, config(inv, Cn), dtype=torch.float64)
        o.step(x, eps)
        P = 64
        # value (pos, c') of the permuted data is value (pos, perm[c']) of the original
        col = (torch.arange(P).reshape(P, 1) * Cn + torch.tensor(perm).reshape(1, Cn)).reshape(-1)
        sd2 = dict(sd)
        w0 = sd["encoder_z.fc_layers.0.weight"]
        sd2["encoder_z.fc_layers.0.weight"] = w0[:, col]
        rows = torch.tensor(perm) if inv else col
        sd2["decoder.out.weight"] = sd["decoder.out.weight"][rows]
        sd2["decoder.out.bias"] = sd["decoder.out.bias"][rows]
        o2 = orc.SVIOracle(sd2, config(inv, Cn), dtype=torch.float64)
        o2.step(x[..., perm], eps)
        torch.testing.assert_close(o2.last["loss"], o.last["loss"], rtol=1e-12, atol=1e-12)
        for k, gk in o.last_grads.items():
            want = gk
            if k == "encoder_z.fc_layers.0.weight":
                want = gk[:, col]
            elif k in ("decoder.out.weight", "decoder.out.bias"):
                want = gk[rows]
            torch.testing.assert_close(o2.last_grads[k], want, rtol=1e-10, atol=1e-12, msg=k)
        # ... and the channels do differ: without permuting the parameters the loss moves
        o3 = orc.SVIOracle(sd, config(inv, Cn), dtype=torch.float64)
        o3.step(x[..., perm], eps)
        assert abs(o3.last["loss"].item() - o.last["loss"].item()) > 1e-3 * abs(o.last["loss"].item())


def test_data_recipe():
    for c in mc.CASES.values():
        x, y, eps = mc.case_data(c)
        assert x.shape == (c["b"],) + tuple(c["dims"]) + (c["C"],)
        if c.get("sampler") == "poisson_log":
            assert (x >= 0).all() and (x == x.round()).all() and x.max() >= 4
        else:
            assert x.min() >= 0.05 and x.max() <= 0.95 + 1e-6
        flat = x.reshape(c["b"], -1, c["C"])
        for a in range(c["C"]):
            for b in range(a + 1, c["C"]):
                assert (flat[..., a] - flat[..., b]).abs().max() > 0.05, "channels %d and %d coincide" % (a, b)


# ------------------------------------------------------------------------------- construction
def test_state_dict_shapes_three_channels():
    m = pv.models.iVAE((8, 8), 2, ["r", "t", "s"], channels=3, seed=1, device="cpu")
    sd = m.state_dict()
    assert m.channels == 3 and m.data_dim == (8, 8)
    assert sd["decoder.out.weight"].shape == (3, 128) and sd["decoder.out.bias"].shape == (3,)
    assert sd["encoder_z.fc_layers.0.weight"].shape == (128, 192)
    assert m.decoder.reshape == (8, 8, 3) and m.grid.shape == (64, 2)
    one = pv.models.iVAE((8, 8), 2, ["r", "t", "s"], seed=1, device="cpu").state_dict()
    assert list(sd) == list(one)
    v = pv.models.iVAE((8, 8), 2, None, channels=3, c_dim=2, seed=1, device="cpu").state_dict()
    assert v["decoder.out.weight"].shape == (192, 128) and v["encoder_z.fc_layers.0.weight"].shape == (128, 194)
    s = pv.models.iVAE((16,), 2, ["t"], channels=4, seed=1, device="cpu")                # 1-D spectra take channels too
    assert s.state_dict()["decoder.out.weight"].shape == (4, 128) and s.decoder.reshape == (16, 4)
    assert s.state_dict()["encoder_z.fc_layers.0.weight"].shape == (128, 64)


def test_one_channel_builds_what_it_always_did():
    """Keys, shapes and initial weights for a given seed, bit for bit: against the default constructor call and against the
    construction sequence restated here (seed, encoder, decoder — with the nets called as they were before `channels`)."""
    for dims, inv in (((8, 8), ["r", "t", "s"]), ((8, 8), None), ((16,), ["t"])):
        a = pv.models.iVAE(dims, 2, inv, seed=3, device="cpu")
        b = pv.models.iVAE(dims, 2, inv, seed=3, channels=1, device="cpu")
        set_deterministic_mode(3)
        enc = fcEncoderNet(dims, 2 + a.coord, 0, None, "tanh", softplus_out=True)
        dec = (sDecoderNet if a.coord > 0 else fcDecoderNet)(dims, 2, 0, None, "tanh", sigmoid_out=True)
        want = {"encoder_z." + k: v for k, v in enc.state_dict().items()}
        want.update({"decoder." + k: v for k, v in dec.state_dict().items()})
        for m in (a, b):
            sd = m.state_dict()
            assert list(sd) == list(want) and m.channels == 1
            for k in want:
                assert sd[k].shape == want[k].shape and torch.equal(sd[k], want[k]), k
            assert m.decoder.reshape == dims
        if a.coord > 0:
            assert a.state_dict()["decoder.out.weight"].shape == (1, 128)


def test_refusals_name_channels():
    kw = dict(seed=1, device="cpu")
    with pytest.raises(ValueError, match="channels"):
        pv.models.jiVAE((8, 8), 2, 3, ["r"], channels=2, **kw)
    with pytest.raises(ValueError, match="channels"):
        pv.models.ssiVAE((8, 8), 2, 3, ["r"], channels=2, **kw)
    with pytest.raises(ValueError, match="channels"):
        pv.models.ss_reg_iVAE((8, 8), 2, 1, ["r"], channels=2, **kw)
    with pytest.raises(ValueError, match="channels"):
        pv.models.VED((32, 32), (32,), latent_dim=2, channels=2, **kw)
    for bad in (0, 9, -1, 2.0, True, "3"):
        with pytest.raises(ValueError, match="channels"):
            pv.models.iVAE((8, 8), 2, ["r"], channels=bad, **kw)
    m = pv.models.iVAE((8, 8), 2, ["r"], channels=2, **kw)
    with pytest.raises(ValueError, match="channels"):
        m.set_encoder(convEncoderNet((8, 8), 1, 3, hidden_dim=[(4,)]))
    with pytest.raises(ValueError, match="channels"):
        m.set_encoder(torch.nn.Linear(128, 6))
    with pytest.raises(ValueError, match="channels"):
        m.set_decoder(torch.nn.Linear(2, 128))
    x = torch.zeros(2, 8, 8, 2)
    with pytest.raises(ValueError, match="channels"):
        m.model(x)
    with pytest.raises(ValueError, match="channels"):
        m.guide(x)
    # a network swapped in behind the constructor's back is caught when the engine is made
    m.encoder_z = torch.nn.Linear(128, 6)
    with pytest.raises(UnsupportedModel, match="channels"):
        m.engine()
    # the single-channel models keep taking what they took
    pv.models.jiVAE((8, 8), 2, 3, ["r"], channels=1, **kw)
    one = pv.models.iVAE((8, 8), 2, ["r"], **kw)
    one.set_decoder(torch.nn.Linear(2, 64))


def test_bf16_precision_is_refused_before_anything_runs():
    m = pv.models.iVAE((8, 8), 2, ["r"], channels=2, seed=1, device="cpu")
    with pytest.raises(ValueError, match="channels"):
        pv.trainers.SVItrainer(m, precision="bf16")


# ------------------------------------------------------------------------------- plan validation (host arithmetic)
def test_header_constant():
    src = open(os.path.join(ROOT, "include", "pyroved_amd.h")).read()
    m = re.search(r"#define\s+PV_MAX_CHANNELS\s+(\d+)", src)
    assert m and int(m.group(1)) == 8 == _abi.PV_MAX_CHANNELS
    assert _abi.PV_ABI_VERSION == 17 and _abi.lib().pv_version() == 17 and C.sizeof(_abi.pv_ivae_plan) == 2824


def test_plan_validation_through_the_workspace_queries():
    lib = _abi.lib()
    EINVAL = -1
    prev = 0
    for ch in range(1, 9):
        for fused in (0, 1, 2, 3):                                  # a fused request falls back to the layered kernels
            p = _plan(fused, ch)
            assert lib.pv_ivae_workspace_bytes(C.byref(p)) > 0, (ch, fused)
            if ch > 1:
                assert lib.pv_ivae_uses_fused(C.byref(p)) == 0
                assert lib.pv_ivae_workspace_bytes_for(C.byref(p), 1) == lib.pv_ivae_workspace_bytes_for(C.byref(_plan(0, ch)), 1)
        step = lib.pv_ivae_workspace_bytes_for(C.byref(_plan(0, ch)), 1)
        assert step > prev                                          # (the encoder's input, x / loc and the partials grow with C)
        prev = step
        assert lib.pv_ivae_particles_workspace_bytes(C.byref(_plan(0, ch)), 3) > step
        assert lib.pv_ivae_renyi_workspace_bytes(C.byref(_plan(0, ch)), 3) > step
    assert lib.pv_ivae_workspace_bytes(C.byref(_plan(0, 9))) == EINVAL
    assert lib.pv_ivae_workspace_bytes(C.byref(_plan(0, 0))) == EINVAL
    p = _plan(0, 2)
    p.n_pix = 785                                                   # not a whole number of positions
    assert lib.pv_ivae_workspace_bytes(C.byref(p)) == EINVAL
    assert lib.pv_ivae_workspace_bytes(C.byref(_plan(0, 1, discrete_dim=3))) > 0
    assert lib.pv_ivae_workspace_bytes(C.byref(_plan(0, 2, discrete_dim=3))) == EINVAL
    keep = C.create_string_buffer(64)
    for field in ("row_w", "row_elbo", "dy"):
        for ch, ok in ((1, True), (2, False)):
            p = _plan(0, ch)
            if field == "dy":
                p.c_dim = 1
                p.fc_latent.in_dim = 3
                p.enc[0].in_dim += 1
            setattr(p, field, C.addressof(keep))
            assert (lib.pv_ivae_workspace_bytes(C.byref(p)) > 0) == ok, (field, ch)
    for ch, ok in ((1, True), (2, False)):
        p = _plan(0, ch)                                            # a conv encoder: Conv2d(1 -> 4, k 3) on 28 x 28
        p.n_pix, p.n_enc, p.n_enc_ops, p.enc_ndim = 784, 0, 1, 2
        p.enc_in_dim[0] = p.enc_in_dim[1] = 28
        op = _abi.pv_op()
        op.kind, op.cin, op.cout, op.ksize, op.act, op.w_off, op.b_off = _abi.OP["conv"], 1, 4, 3, _abi.ACT["lrelu"], 0, 36
        p.enc_ops[0] = op
        p.head.in_dim = 4 * 784
        if ch > 1:
            p.n_pix = 784 * ch
        assert (lib.pv_ivae_workspace_bytes(C.byref(p)) > 0) == ok, ("conv", ch)
        for field in ("ext_encoder", "ext_decoder"):
            p = _plan(0, ch)
            setattr(p, field, 1)
            assert (lib.pv_ivae_workspace_bytes(C.byref(p)) > 0) == ok, (field, ch)
    assert lib.pv_ivae_loss_and_grads(C.byref(_plan(0, 3)), 1, None) == EINVAL        # no buffers: refused before any pointer


def test_single_channel_workspace_sizes_are_the_parent_commits():
    """Bytes of pv_ivae_workspace_bytes_for(plan, what) for what = 0 .. 3 and of the 3-particle and Renyi step layouts.  The
    constants were taken from the parent commit's library (built from that commit's sources, queried with these same plans):
    with one channel every offset and the total stay what they were."""
    lib = _abi.lib()
    want = PARENT_WS
    for name, p in (("spatial_fused", _plan(2)), ("spatial_layered", _plan(0)), ("vanilla", _vanilla_plan(2))):
        got = [lib.pv_ivae_workspace_bytes_for(C.byref(p), w) for w in range(4)]
        got.append(lib.pv_ivae_particles_workspace_bytes(C.byref(p), 3))
        got.append(lib.pv_ivae_renyi_workspace_bytes(C.byref(p), 3))
        assert got == want[name], (name, got)


# [PV_WS_ALL, _STEP, _ENCODE, _DECODE, 3-particle step, 3-particle Renyi step], from the parent commit's library
PARENT_WS = {
    "spatial_fused": [37228288, 37228288, 107776, 140288, 39313920, 39314176],
    "spatial_layered": [41397248, 41397248, 107776, 41397248, 107202304, 107202560],
    "vanilla": [306688, 306688, 122368, 306688, 841984, 842240],
}


# ------------------------------------------------------------------------------- the GPU step cases' condition
def _near_zero_share(o, tag, worst):
    for key, g in o.last_grads.items():
        assert g.norm().item() > 0.0, "%s %s: zero gradient" % (tag, key)
        share = near_zero_share(g)
        worst[0] = max(worst[0], share)
        assert share < ILL_SHARE, "%s %s: %.2f %% near-zero gradient entries" % (tag, key, 100 * share)


def test_gpu_step_cases_keep_near_zero_gradient_entries_below_one_percent():
    """tests/_judge.py's check_params_after_adam holds entries with |g_ref| < 1e-5 max|g_ref| to 2 lr only, on
    the condition that they are fewer than 1 % of a tensor and that no tensor's gradient vanishes: confirmed here with the
    float64 reference alone, at every case of tests/_multichannel_cases.py over its two steps (each from float32-rounded parameters, as there).
    Measured worst share: 0.78 % (one entry of a 128-entry bias).  (An lrelu decoder breaches the cap with 7 %: no case uses one.)"""
    torch.set_num_threads(min(8, torch.get_num_threads()))
    worst = [0.0]
    for name, c in sorted(mc.CASES.items()):
        model = pv.models.iVAE(c["dims"], 2, c["inv"], seed=1, device="cpu", **mc.model_kwargs(c))
        x, y, eps = mc.case_data(c)
        o = orc.SVIOracle(state(model), mc.case_config(c), dtype=torch.float64)
        for k in range(2):
            o.step(x, eps[k], 1.0, y)
            _near_zero_share(o, "%s step %d" % (name, k), worst)
            mc.round_to_float32(o)
    print("worst near-zero share, one-particle cases: %.3f %%" % (100 * worst[0]))
    # the other objectives on case 1's shape
    c = mc.CASES["c01_8x8_rts_c2_b6"]
    model = pv.models.iVAE(c["dims"], 2, c["inv"], seed=1, device="cpu", **mc.model_kwargs(c))
    x, y, eps3 = mc.case_data(c, particles=3)
    _, _, eps1 = mc.case_data(c)
    for tag, kw, eps in (("analytic", dict(kl="analytic"), eps1), ("particles3", dict(particles=3), eps3),
                         ("renyi3", dict(particles=3, renyi=0.0), eps3)):
        o = orc.SVIOracle(state(model), mc.case_config(c), dtype=torch.float64, **kw)
        for k in range(2):
            o.step(x, eps[k], 1.0, y)
            _near_zero_share(o, "%s step %d" % (tag, k), worst)
            mc.round_to_float32(o)
    print("worst near-zero share overall: %.3f %%" % (100 * worst[0]))


def test_encode_layout_of_a_wide_decoder():
    """The encode-only layout gives the decoder zero rows; sizing the split-K scratch of a zero-row problem whose contraction
    is 256 .. 1024 long (the GPU tests' 512-wide decoder) used to divide by its tile count.  One channel and eight."""
    lib = _abi.lib()
    for ch in (1, 8):
        p = _plan(0, ch)
        p.batch = 2
        p.n_pix = 16 * ch
        p.enc[0].in_dim = 16 * ch
        for l in (p.fc_coord, p.fc_latent, p.dec[0], p.dec[1]):
            l.out_dim = 512
        p.dec[0].in_dim = p.dec[1].in_dim = p.out.in_dim = 512
        enc = lib.pv_ivae_workspace_bytes_for(C.byref(p), 2)
        assert 0 < enc < lib.pv_ivae_workspace_bytes_for(C.byref(p), 1)
