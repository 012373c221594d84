"""
The workspace contract without a GPU (tests/_ws_contract.py has the GPU half's method):
  * the kit tests itself, in the spirit of tests/test_judge_cpu.py: its guards see one byte, its 0xFF fill is NaN in both float
    formats, its comparison is bitwise, its install refuses a short view, and run_cell finds a planted read of unwritten bytes;
  * PV_EWS: every entry point that takes a plan with ws_bytes refuses a workspace one byte short of its query with -2 — before
    anything touches HIP, which is why this runs here: every pointer of the plan is a small HOST buffer that nothing may
    dereference, and there is no device to launch on;
  * the workspace queries answer with a null `ws` (carve with a null base IS the size query).
"""
import ctypes as C

import pytest
import torch

import pyroved_amd as pv
from pyroved_amd import _abi, ops
from pyroved_amd._convplan import conv_ops, fill_ops
import _plan_kit as pk
import _ws_contract as wc

PV_EINVAL, PV_EWS = -1, -2


# ------------------------------------------------------------------------------- the kit
@pytest.mark.parametrize("fill", wc.FILLS)
def test_guard_check_sees_one_byte_at_either_inner_edge(fill):
    need, guard = 1000, 4096
    for at in (guard - 1, guard + need):                 # the last byte in front of the workspace, the first one behind it
        view, check = wc.guarded(need, fill, guard=guard, device="cpu")
        assert view.numel() == need and view.data_ptr() == check.ptr
        check()
        view.fill_(7)                                    # the workspace itself is the call's to write
        check()
        check.base[at] ^= 0x10
        with pytest.raises(AssertionError, match="guard bytes changed"):
            check()
        assert check.damage() == [("front", -1, 1)] if at < guard else check.damage() == [("back", need, 1)]


def test_guards_differ_per_fill_and_from_the_fill():
    seen = set()
    for fill in wc.FILLS:
        view, check = wc.guarded(256, fill, guard=4096, device="cpu")
        front, back = check.saved
        assert not torch.equal(front[:256], view) and not torch.equal(back[:256], view)
        seen.add(bytes(front[:16].tolist()))
    assert len(seen) == 3
    a, _ = wc.guarded(4096, "noise", guard=4096, device="cpu")
    b, _ = wc.guarded(4096, "noise", guard=4096, device="cpu")
    assert torch.equal(a, b) and len(set(a.tolist())) > 200            # seeded, and noise


def test_ones_fill_is_nan_in_fp32_and_bf16_and_all_bits_as_a_word():
    view, _ = wc.guarded(1024, "ones", guard=4096, device="cpu")
    assert torch.isnan(view.view(torch.float32)).all() and torch.isnan(view.view(torch.bfloat16)).all()
    assert (view.view(torch.int32) == -1).all() and (view == 255).all()
    z, _ = wc.guarded(1024, "zeros", guard=4096, device="cpu")
    assert (z == 0).all()


def test_same_bits_is_bitwise():
    a = torch.tensor([1.0, -0.0, float("nan"), 3.5])
    assert wc.same_bits(a, a.clone())
    b = a.clone()
    b.view(torch.int32)[3] ^= 1                          # one mantissa bit
    assert not wc.same_bits(a, b) and torch.allclose(a, b, equal_nan=True)
    c = a.clone()
    c.view(torch.int32)[2] ^= 0x1234                     # another NaN payload: equal_nan would pass it
    assert torch.isnan(c[2]) and not wc.same_bits(a, c)
    assert not wc.same_bits(torch.tensor([0.0]), torch.tensor([-0.0]))
    assert not wc.same_bits(a, a[:3]) and wc.same_bits(a[:0], a[:0])


def test_install_refuses_a_short_view():
    class E:
        ws = None
    view, _ = wc.guarded(512, "zeros", guard=4096, device="cpu")
    assert wc.install(E, view, "ws", 512) is view and E.ws is view
    with pytest.raises(ValueError, match="need 513"):
        wc.install(E, view, "ws", 513)
    with pytest.raises(ValueError):
        wc.install(E, view.view(torch.float32), "ws", 16)


def test_flush_puts_nan_behind_the_input():
    t = torch.arange(15.0).reshape(5, 3)
    f = wc.flush(t, device="cpu")
    assert torch.equal(f, t) and f.data_ptr() % 16 == 0
    behind = torch.as_strided(f, (wc.INPUT_GUARD,), (1,), f.storage_offset() + f.numel())
    assert torch.isnan(behind).all()
    assert wc.flush(None) is None


class _Owner:
    ws = None


def _planted(reads_unwritten, step_over=False):
    """a stand-in call sequence in plain torch: writes 4 workspace words and reads them back — and, planted, reads 4 it never wrote"""
    own = _Owner()
    own.ws = torch.zeros(1024, dtype=torch.uint8)
    out = dict(y=torch.empty(4))

    def call(inp):
        wsf = own.ws.view(torch.float32)
        wsf[:4].copy_(inp["x"])
        extra = (wsf.view(torch.int32)[200:204] & 1).float() if reads_unwritten else 0.0
        out["y"].copy_(wsf[:4] * 2.0 + extra)
    return lambda: wc.Run(own, {"ws": lambda: 1024}, dict(x=torch.arange(4.0)), call, outs=out)


def test_run_cell_passes_a_clean_sequence_and_finds_a_planted_read():
    need, _ = wc.run_cell("clean", _planted(False), device="cpu")
    assert need == {"ws": 1024}
    with pytest.raises(AssertionError, match="a read of bytes the call never wrote"):
        wc.run_cell("planted-read", _planted(True), device="cpu")


def test_run_cell_blames_the_family_not_a_fill_when_two_ordinary_calls_differ():
    own = _Owner()
    own.ws = torch.zeros(64, dtype=torch.uint8)
    out, n = dict(y=torch.empty(1)), [0]

    def call(inp):
        n[0] += 1
        out["y"].fill_(float(n[0]))
    with pytest.raises(AssertionError, match="NON-DETERMINISTIC"):
        wc.run_cell("drifting", lambda: wc.Run(own, {"ws": lambda: 64}, {}, call, outs=out), device="cpu")


def test_run_cell_refuses_an_engine_that_over_allocates():
    own = _Owner()
    own.ws = torch.zeros(128, dtype=torch.uint8)
    with pytest.raises(AssertionError, match="the workspace query says 64"):
        wc.run_cell("fat", lambda: wc.Run(own, {"ws": lambda: 64}, {}, lambda inp: None), device="cpu")


# ------------------------------------------------------------------------------- PV_EWS
_HOST = (C.c_char * 256)()                               # every pointer of every plan below: host memory nothing may touch
HOST = C.addressof(_HOST)
_IVAE_PTRS = ("params", "grads", "adam_m", "adam_v", "x", "eps", "grid", "ws", "scalars")


def ivae_plan(fused=2, **kw):
    p = pk._small_plan(fused=fused)
    for f in _IVAE_PTRS:
        setattr(p, f, HOST)
    p.n_params, p.adam_step, p.lr, p.adam_beta1, p.adam_beta2, p.adam_eps = 1 << 20, 1, 1e-3, 0.9, 0.999, 1e-8
    p.beta = 1.0
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def _vanilla(fused=0):
    p = pk._vanilla_plan(fused)
    for f in _IVAE_PTRS:
        setattr(p, f, HOST)
    p.n_params, p.adam_step, p.beta = 1 << 20, 1, 1.0
    return p


def _ivae_entry_points():
    """(id, plan factory, query(lib, plan) -> need, call(lib, plan) -> code)"""
    P, A = 3, C.c_float(0.0)
    ref = C.byref
    step_q = lambda L, p: L.pv_ivae_workspace_bytes_for(ref(p), 1)
    part_q = lambda L, p: L.pv_ivae_particles_workspace_bytes(ref(p), P)
    ren_q = lambda L, p: L.pv_ivae_renyi_workspace_bytes(ref(p), P)
    w_q = lambda L, p: L.pv_ivae_weighted_workspace_bytes(ref(p))
    guide = lambda f: ivae_plan(f, ext_decoder=1, ext_z=HOST, ext_dz=HOST, ext_ll=HOST)
    fast = lambda f: ivae_plan(f, flags=_abi.PV_PLAN_FAST_WEIGHTS)
    out = []
    for f in (0, 1, 2, 3):
        t = "fused%d" % f
        out += [("loss_and_grads-" + t, lambda f=f: ivae_plan(f), step_q, lambda L, p: L.pv_ivae_loss_and_grads(ref(p), 1, None)),
                ("loss_only-" + t, lambda f=f: ivae_plan(f), step_q, lambda L, p: L.pv_ivae_loss_and_grads(ref(p), 0, None)),
                ("step-" + t, lambda f=f: ivae_plan(f), step_q, lambda L, p: L.pv_ivae_step(ref(p), None)),
                ("encode-" + t, lambda f=f: ivae_plan(f), lambda L, p: L.pv_ivae_workspace_bytes_for(ref(p), 2),
                 lambda L, p: L.pv_ivae_encode(ref(p), HOST, HOST, None)),
                ("decode-" + t, lambda f=f: ivae_plan(f), lambda L, p: L.pv_ivae_workspace_bytes_for(ref(p), 3),
                 lambda L, p: L.pv_ivae_decode(ref(p), HOST, 0.0, 0.0, 0.0, 1.0, HOST, None))]
    for f in (0, 2, 3):
        t = "fused%d" % f
        out += [("particles_loss_and_grads-" + t, lambda f=f: ivae_plan(f), part_q,
                 lambda L, p: L.pv_ivae_particles_loss_and_grads(ref(p), P, 1, None)),
                ("particles_step-" + t, lambda f=f: ivae_plan(f), part_q, lambda L, p: L.pv_ivae_particles_step(ref(p), P, None)),
                ("renyi_loss_and_grads-" + t, lambda f=f: ivae_plan(f), ren_q,
                 lambda L, p: L.pv_ivae_renyi_loss_and_grads(ref(p), P, A, 1, HOST, None)),
                ("renyi_step-" + t, lambda f=f: ivae_plan(f), ren_q, lambda L, p: L.pv_ivae_renyi_step(ref(p), P, A, HOST, None))]
    for t, mk in (("fused0", lambda: ivae_plan(0)), ("fused1", lambda: ivae_plan(1)), ("fused2", lambda: ivae_plan(2)),
                  ("fast2", lambda: fast(2)), ("fast3", lambda: fast(3))):
        out += [("weighted_loss_and_grads-" + t, mk, w_q, lambda L, p: L.pv_ivae_weighted_loss_and_grads(ref(p), HOST, 1, None)),
                ("weighted_step-" + t, mk, w_q, lambda L, p: L.pv_ivae_weighted_step(ref(p), HOST, None)),
                ("weighted_images_loss_and_grads-" + t, mk, w_q,
                 lambda L, p: L.pv_ivae_weighted_images_loss_and_grads(ref(p), HOST, 1, None)),
                ("weighted_images_step-" + t, mk, w_q, lambda L, p: L.pv_ivae_weighted_images_step(ref(p), HOST, None))]
    out += [("guide", lambda: guide(2), step_q, lambda L, p: L.pv_ivae_guide(ref(p), None)),
            ("guide_backward", lambda: guide(2), step_q, lambda L, p: L.pv_ivae_guide_backward(ref(p), 1, None)),
            ("guide_backward_loss_only", lambda: guide(2), step_q, lambda L, p: L.pv_ivae_guide_backward(ref(p), 0, None)),
            ("encode-ext_decoder", lambda: guide(2), lambda L, p: L.pv_ivae_workspace_bytes_for(ref(p), 2),
             lambda L, p: L.pv_ivae_encode(ref(p), HOST, HOST, None)),
            ("loss_and_grads-vanilla", _vanilla, step_q, lambda L, p: L.pv_ivae_loss_and_grads(ref(p), 1, None)),
            ("step-vanilla", _vanilla, step_q, lambda L, p: L.pv_ivae_step(ref(p), None)),
            ("decode-vanilla", _vanilla, lambda L, p: L.pv_ivae_workspace_bytes_for(ref(p), 3),
             lambda L, p: L.pv_ivae_decode(ref(p), HOST, 0.0, 0.0, 0.0, 1.0, HOST, None)),
            ("loss_and_grads-jivae", lambda: _with_ptrs(pk._small_plan(discrete_dim=3, fused=2)), step_q,
             lambda L, p: L.pv_ivae_loss_and_grads(ref(p), 1, None)),
            ("loss_and_grads-poisson", lambda: ivae_plan(2, lik=_abi.LIK["poisson_log"], sigmoid_out=0), step_q,
             lambda L, p: L.pv_ivae_loss_and_grads(ref(p), 1, None))]
    return out


def _with_ptrs(p):
    for f in _IVAE_PTRS:
        setattr(p, f, HOST)
    p.n_params, p.adam_step, p.beta, p.beta_disc = 1 << 20, 1, 1.0, 1.0
    return p


_IVAE = _ivae_entry_points()


def _short_by_one(lib, p, query, call, what):
    need = int(query(lib, p))
    assert need > 0, "%s: the workspace query refuses the plan (%d)" % (what, need)
    p.ws_bytes = need - 1
    assert call(lib, p) == PV_EWS, "%s: a workspace of %d bytes (one short of the query) is not PV_EWS" % (what, need - 1)
    p.ws, p.ws_bytes = None, need                        # and the size query does not need the pointer
    assert int(query(lib, p)) == need
    return need


@pytest.mark.parametrize("ep", _IVAE, ids=[e[0] for e in _IVAE])
def test_ivae_entry_points_refuse_a_short_workspace(ep):
    name, mk, query, call = ep
    _short_by_one(_abi.lib(), mk(), query, call, name)


def test_short_workspace_is_judged_before_the_pointers_are_used():
    """PV_EWS comes from arithmetic on the plan alone: the same answer with ws_bytes = 0 and with 1 byte short, and PV_EINVAL —
    not a fault — for a null workspace pointer"""
    lib = _abi.lib()
    p = ivae_plan(2)
    need = lib.pv_ivae_workspace_bytes_for(C.byref(p), 1)
    for nbytes in (0, 1, need // 2, need - 1):
        p.ws_bytes = nbytes
        assert lib.pv_ivae_loss_and_grads(C.byref(p), 1, None) == PV_EWS
        assert lib.pv_ivae_step(C.byref(p), None) == PV_EWS
    p.ws, p.ws_bytes = None, need
    assert lib.pv_ivae_loss_and_grads(C.byref(p), 1, None) == PV_EINVAL


# ---- pv_ved_*: the plan of a small VED read off the modules as engine_ved.VEDEngine._static_plan reads it, offsets of our own
def _layout_of(named):
    layout, off = {}, 0
    for k, t in named:
        layout[k] = off
        off += (t.numel() + 63) // 64 * 64
    return layout, off


def _layer(layout, prefix, lin, act):
    l = _abi.pv_layer()
    l.in_dim, l.out_dim, l.act = lin.in_features, lin.out_features, _abi.ACT[act]
    l.w_off = layout[prefix + ".weight"]
    l.b_off = layout[prefix + ".bias"] if lin.bias is not None else -1
    return l


def ved_plan(batchnorm=False, batch=4):
    kw = dict(hidden_dim_e=[(8,), (16, 16)], hidden_dim_d=[(16, 16), (8,)])       # (the ved_1d32_to_1d32_small fixtures' networks)
    model = pv.models.VED((32,), (32,), latent_dim=2, seed=1, device="cpu", batchnorm=batchnorm, **kw)
    enc, dec = model.encoder_z, model.decoder
    named = list(model.named_parameters()) + [(k, b) for k, b in model.named_buffers()
                                              if k.endswith((".running_mean", ".running_var"))]
    layout, total = _layout_of(named)
    p = _abi.pv_ved_plan()
    p.batch, p.ndim_in, p.ndim_out = batch, len(enc.input_dim), len(dec.output_dim)
    for i, d in enumerate(enc.input_dim):
        p.in_dim[i] = d
    for i, d in enumerate(dec.output_dim):
        p.out_dim[i] = d
    p.in_ch, p.out_ch, p.z_dim, p.beta = enc.input_channels, dec.output_channels, model.z_dim, 1.0
    p.lik, p.sigmoid_out, p.decoder_sig = _abi.LIK[model.sampler_d.name], int(dec.sigmoid_out), model.sampler_d.decoder_sig
    p.n_enc_ops = fill_ops(p.enc, conv_ops(enc.feature_extractor.layers, enc.feature_extractor.activation,
                                           "encoder_z.feature_extractor.layers"), layout)
    p.n_dec_ops = fill_ops(p.dec, conv_ops(dec.upsampler.layers, dec.upsampler.activation, "decoder.upsampler.layers"), layout)
    p.head = _layer(layout, "encoder_z.features2latent.fc_latent", enc.features2latent.fc_latent, None)
    p.l2f = _layer(layout, "decoder.latent2features.fc", dec.latent2features.fc, None)
    shape0 = [int(v) for v in dec.latent2features.reshape_]
    p.dec_c0 = shape0[0]
    for i, d in enumerate(shape0[1:]):
        p.dec_dim0[i] = d
    p.conv_bf16, p.n_params = 4, total
    for f in ("params", "grads", "adam_m", "adam_v", "x", "y", "eps", "ws", "scalars"):
        setattr(p, f, HOST)
    return p


@pytest.mark.parametrize("batchnorm", [False, True], ids=["plain", "batchnorm"])
@pytest.mark.parametrize("conv_bf16", [0, 3, 4])
def test_ved_entry_points_refuse_a_short_workspace(conv_bf16, batchnorm):
    lib = _abi.lib()
    ref = C.byref
    q = lambda L, p: L.pv_ved_workspace_bytes(ref(p))
    for what, call in (("pv_ved_loss_and_grads", lambda L, p: L.pv_ved_loss_and_grads(ref(p), 1, None)),
                       ("pv_ved_loss_and_grads (no gradients)", lambda L, p: L.pv_ved_loss_and_grads(ref(p), 0, None)),
                       ("pv_ved_encode", lambda L, p: L.pv_ved_encode(ref(p), HOST, HOST, None)),
                       ("pv_ved_decode", lambda L, p: L.pv_ved_decode(ref(p), HOST, HOST, None))):
        p = ved_plan(batchnorm)
        p.conv_bf16 = conv_bf16
        _short_by_one(lib, p, q, call, what)


# ---- pv_mlp_*: the label network of the semi-supervised models
def mlp_plan(out_kind):
    q = _abi.pv_mlp_plan()
    q.batch, q.in_dim, q.n_layers, q.out_kind = 6, 64, 2, _abi.MLP_OUT[out_kind]

    def layer(i, o, act, w_off):
        l = _abi.pv_layer()
        l.in_dim, l.out_dim, l.act, l.w_off, l.b_off = i, o, _abi.ACT[act], w_off, w_off + i * o
        return l
    q.layers[0], q.layers[1] = layer(64, 128, "tanh", 0), layer(128, 128, "tanh", 16384)
    q.out = layer(128, 3, None, 40960)
    for f in ("params", "grads", "x", "ws"):
        setattr(q, f, HOST)
    return q


@pytest.mark.parametrize("out_kind", ["linear", "softmax"])
def test_mlp_entry_points_refuse_a_short_workspace(out_kind):
    lib = _abi.lib()
    q = lambda L, p: L.pv_mlp_workspace_bytes(C.byref(p))
    _short_by_one(lib, mlp_plan(out_kind), q, lambda L, p: L.pv_mlp_forward(C.byref(p), HOST, None), "pv_mlp_forward")
    _short_by_one(lib, mlp_plan(out_kind), q, lambda L, p: L.pv_mlp_backward(C.byref(p), HOST, HOST, None), "pv_mlp_backward")


# ---- pv_convnet_*: a stand-alone stack through ops._stack_plan, as nets.conv's forward builds it
@pytest.mark.parametrize("kind", ["fe2d_bn", "fe1d_dx", "up1d"])
def test_convnet_entry_points_refuse_a_short_workspace(kind):
    from pyroved_amd.nets.conv import FeatureExtractor, Upsampler
    torch.manual_seed(3)
    if kind == "fe2d_bn":
        net, x = FeatureExtractor(2, 1, [(8,), (16,)], batchnorm=True, activation="lrelu"), torch.zeros(5, 1, 8, 8)
    elif kind == "fe1d_dx":
        net, x = FeatureExtractor(1, 2, [(16,), (32, 32)], batchnorm=False, activation="lrelu"), torch.zeros(4, 2, 40).requires_grad_()
    else:
        net, x = Upsampler(1, 32, [(32, 32), (16,)], 1, batchnorm=False, activation="lrelu", upsampling_mode="nearest"), \
            torch.zeros(3, 32, 8).requires_grad_()
    lib = _abi.lib()
    q = lambda L, p: L.pv_convnet_workspace_bytes(C.byref(p))

    def plan():
        p, need = ops._stack_plan(net, x, conv_ops(net.layers, net.activation, "L"))
        assert need > 0
        p.params = p.grads = p.ws = HOST
        return p
    _short_by_one(lib, plan(), q, lambda L, p: L.pv_convnet_forward(C.byref(p), HOST, HOST, None), "pv_convnet_forward")
    _short_by_one(lib, plan(), q, lambda L, p: L.pv_convnet_backward(C.byref(p), HOST, HOST, None, None), "pv_convnet_backward")


# ------------------------------------------------------------------------------- the size queries need no workspace
def test_workspace_queries_answer_with_a_null_workspace():
    lib = _abi.lib()
    for fused in (0, 1, 2, 3):
        p = pk._small_plan(fused=fused)                  # every pointer null, ws_bytes 0
        assert p.ws is None and p.ws_bytes == 0
        sizes = [lib.pv_ivae_workspace_bytes_for(C.byref(p), w) for w in (0, 1, 2, 3)]
        assert min(sizes) > 0 and sizes[0] == max(sizes) == lib.pv_ivae_workspace_bytes(C.byref(p))
        assert all(s % 256 == 0 for s in sizes), sizes   # every region is padded to 256 bytes
        assert lib.pv_ivae_particles_workspace_bytes(C.byref(p), 1) == sizes[1]
        if fused != 1:
            assert lib.pv_ivae_particles_workspace_bytes(C.byref(p), 3) > sizes[1]
            assert lib.pv_ivae_renyi_workspace_bytes(C.byref(p), 3) > lib.pv_ivae_particles_workspace_bytes(C.byref(p), 3)
        if fused != 3:
            assert lib.pv_ivae_weighted_workspace_bytes(C.byref(p)) > 0
    v = ved_plan()
    v.ws, v.ws_bytes = None, 0
    assert lib.pv_ved_workspace_bytes(C.byref(v)) > 0
    m = mlp_plan("softmax")
    m.ws, m.ws_bytes = None, 0
    assert lib.pv_mlp_workspace_bytes(C.byref(m)) > 0
