"""
GPU tests (-m gpu) of the workspace contract of include/pyroved_amd.h: the size a workspace query returns is enough, and the
workspace may hold anything when a call starts (tests/_ws_contract.py has the method; tests/test_workspace_contract_cpu.py the
refusal of a smaller one).

One pytest id per cell.  A cell is one call sequence of one engine on one case of the existing case kits:
  the fused decoder families of tests/_partition_cases.py at the edges of the row partition (kmax = 44 with almost every slot
    unused, batch == grid and one above it, samples that straddle workgroups, row_elbo / dy in the call, jiVAE, particles) — the
    fp32-class ones also judged against the float64 reference on the noise-fill run, at that kit's bars, so that two runs that are
    wrong in the same way cannot pass;
  the Renyi bound, the analytic KL, Poisson, image_weights and fast_weights on the smallest case of their kits;
  the layered path (a spatial tanh model, a GELU model, a vanilla decoder), the conv encoder, its batch-norm form, VED at both
    precisions, VED with batch norm;
  the semi-supervised engines (row_w + row_elbo, dy, and the label MLP's own workspace), a user-defined encoder, a user-defined
    decoder (the guide pair: poisoned before pv_ivae_guide only);
  encode, decode (257 one-unit samples on the fused forward-only kernel, and layered), want_grads=False;
  the one-call step (gradients zero afterwards; parameters, m and v in the snapshot);
  pv_linear_fwd / _bwd and pv_convnet_forward / _backward straight through the C ABI.
Cells the engines refuse are listed with the reason and the refusal is asserted (test_every_cell_is_run_or_refused_with_a_reason).
"""
import ctypes as C
import os

import pytest
import torch

from conftest import load_golden, make_x, ssmeta_of, ss_build

import pyroved_amd as pv
from pyroved_amd import _abi, ops
from _golden_models import convenc_model, ved_case, vedbn_oracle
from _judge import rel_l2
from _variant_cases import variant_case
import _fast_weight_cases as fw
import _image_weight_cases as iwc
import _partition_cases as pc
import _poisson_data as pd
import _renyi_cases as rc
import _ws_contract as wc

pytestmark = pytest.mark.gpu

REPORT = []                                             # (cell, {workspace: bytes}, seconds): printed per cell, kept for the profile


def _report(name, need, secs):
    REPORT.append((name, need, secs))
    print("[ws-contract] %-44s need %s  %.2f s" % (name, " ".join("%s=%d" % kv for kv in need.items()), secs))
    out = os.environ.get("PV_WS_CONTRACT_REPORT")       # (a file the per-cell figures of profiles/workspace_contract.txt come from)
    if out:
        with open(out, "a") as f:
            f.write("%-44s %-28s %.2f\n" % (name, " ".join("%s=%d" % kv for kv in need.items()), secs))


def cuda(t):
    return None if t is None else t.cuda()


# ------------------------------------------------------------------------------- the fused decoder families
PARTITION_CELLS = [
    ("e05_28x28_rt_b6", ("f32", "x3", "h231", "bf16w4", "bf16w8")),
    ("e09_1d16_t_b256", ("x3", "h231", "bf16w4", "bf16w8")),
    ("e01_1d16_t_b257", ("f32", "x3", "bf16w8")),
    ("e04_6x8_rt_b171", ("x3", "h221", "mc3", "w1", "w4")),
    ("e06_8x8_rts_cdim2_b600", ("h231", "bf16w8")),
    ("e10_jivae_k3_1d16_t_b86", ("f32", "x3")),
    ("e11_p3_1d16_t_b86", ("x3", "bf16w4")),
]
FP32_CLASS = ("f32", "x3", "h231", "h221", "mc3", "w1", "w4")


def partition_engine(name, family):
    c, fam = pc.CASES[name], pc.FAMILIES[family]
    variant = fam["variant"]
    model = pc.make_model(name, variant, "cuda")
    kw = dict(fam["engine"])
    if variant != "plain" and variant[0] == "w":
        kw["pixel_weights"] = pc.weights_of(name, variant)
    if c["P"] > 1:
        kw["particles"] = c["P"]
    eng = model.engine(**kw)
    eng.dec_kernel = fam["sel"]
    return model, eng


def partition_judge(name, family, eng):
    """the noise-fill run against the float64 reference at the kit's own bars (fp32-class families)"""
    c, variant = pc.CASES[name], pc.FAMILIES[family]["variant"]
    S, N = pc.n_samples(c), pc.n_pos(c)

    def judge(snap):
        ref = pc.reference(name, variant)
        s = snap["scalars"].cpu().double()
        bad = []
        for i, q in enumerate(("loss", "ll")):
            e = abs(s[i].item() - ref[q]) / abs(ref[q])
            if not e < pc.RTOL_ELBO:
                bad.append((q, e, pc.RTOL_ELBO))
        for k, want in ref["grads"].items():
            got = snap["grad." + k].cpu().double()
            bar = pc.grad_bar(name, family, k)
            if bar is None:
                e, bar = abs(got.item() - want.item()), 1e-6 * S * N + 1e-5
            else:
                e = rel_l2(got, want)
            if not e < bar:
                bad.append((k, e, bar))
        assert not bad, "%s-%s, noise fill, against the float64 reference: %s" % (
            name, family, "; ".join("%s %.3e (bar %.1e)" % t for t in bad))
    return judge


def partition_cell(name, family, step=False, want_grads=True):
    def make():
        c, variant = pc.CASES[name], pc.FAMILIES[family]["variant"]
        B, S, N, Cn = c["B"], pc.n_samples(c), pc.n_pos(c), pc.channels_of(variant)
        model, eng = partition_engine(name, family)
        x, y, eps = pc.inputs(name, variant)
        outs = {}
        if not step:
            outs = dict(z_loc=torch.empty(B, model.z_dim, device="cuda"), z_scale=torch.empty(B, model.z_dim, device="cuda"),
                        loc=torch.empty(S, N * Cn, device="cuda"))
            if want_grads and pc.has_rows(name, family) and c["c_dim"]:
                outs.update(row_elbo=torch.empty(B, device="cuda"), dy=torch.empty(B, c["c_dim"], device="cuda"))

        def call(inp):
            kw = {}
            if not step:
                kw = dict(z_out=(outs["z_loc"], outs["z_scale"]), loc_out=outs["loc"])
                kw.update({k: outs[k] for k in ("row_elbo", "dy") if k in outs})
            if "pixel_weights" in inp:
                eng.pixel_weights = inp["pixel_weights"]
            eng.loss_and_grads(inp["x"], inp["eps"], 1.0, inp["y"], want_grads=want_grads, step=step, **kw)

        judge = partition_judge(name, family, eng) if (family in FP32_CLASS and want_grads and not step) else None
        inputs = dict(x=cuda(x), eps=cuda(eps), y=cuda(y))
        if eng.pixel_weights is not None:
            inputs["pixel_weights"] = eng.pixel_weights
        return wc.engine_run(eng, inputs, call, outs=outs,
                             workspaces={"ws": wc.ivae_query(eng, B)}, want_grads=want_grads, step=step, judge=judge)
    return make


# ------------------------------------------------------------------------------- objectives and likelihoods
def renyi_cell():
    cfg, params, x, y, eps, b, P, beta, model = rc.case_inputs("8x8_rts_b6_p3", "cuda")
    eng = model.engine(fused=2, particles=P, renyi=0.0)
    outs = dict(weights=torch.empty(P * b, device="cuda"), loc=torch.empty(P * b, cfg.n_pix, device="cuda"))

    def call(inp):
        eng.loss_and_grads(inp["x"], inp["eps"], beta, inp["y"], weights_out=outs["weights"], loc_out=outs["loc"])
    return wc.engine_run(eng, dict(x=cuda(x), eps=cuda(eps[0]), y=cuda(y)), call, outs=outs, workspaces={"ws": wc.ivae_query(eng, b, beta=beta)})


def analytic_cell():
    """the smallest partition case with the closed-form KL (tests/test_gpu_meanfield.py's keyword)"""
    name = "e09_1d16_t_b256"
    model = pc.make_model(name, "plain", "cuda")
    eng = model.engine(fused=2, kl="analytic")
    x, y, eps = pc.inputs(name, "plain")
    B = pc.CASES[name]["B"]
    outs = dict(z_loc=torch.empty(B, model.z_dim, device="cuda"), z_scale=torch.empty(B, model.z_dim, device="cuda"))

    def call(inp):
        eng.loss_and_grads(inp["x"], inp["eps"], 1.0, z_out=(outs["z_loc"], outs["z_scale"]))
    return wc.engine_run(eng, dict(x=cuda(x), eps=cuda(eps)), call, outs=outs, workspaces={"ws": wc.ivae_query(eng, B)})


def poisson_cell(fused):
    def make():
        model, cfg, x, y, eps, b = pd.step_case("8x8_rts_b6", "cuda")
        eng = model.engine(fused=fused)
        outs = dict(loc=torch.empty(b, cfg.n_pix, device="cuda"))

        def call(inp):
            eng.loss_and_grads(inp["x"], inp["eps"], 1.0, loc_out=outs["loc"])
        return wc.engine_run(eng, dict(x=cuda(x), eps=cuda(eps[0])), call, outs=outs, workspaces={"ws": wc.ivae_query(eng, b)})
    return make


def image_weights_cell():
    c = iwc.CASES[iwc.CASE1]
    x, y, eps = iwc.case_data(c)
    model = pv.models.iVAE(c["dims"], 2, c["inv"], seed=1, device="cuda")
    eng = model.engine(image_weights=True)
    w = iwc.weights(c)[..., 0].contiguous()

    def call(inp):
        eng.loss_and_grads(inp["x"], inp["eps"], 1.0, image_weights=inp["image_weights"])
    return wc.engine_run(eng, dict(x=cuda(x), eps=cuda(eps[0]), image_weights=cuda(w)), call, workspaces={"ws": wc.ivae_query(eng, c["b"])})


def fast_weights_cell(route):
    def make():
        c = fw.CASES[fw.CASE1]
        x, y, eps = fw.case_data(c)
        model = pv.models.iVAE(c["dims"], 2, c["inv"], seed=1, device="cuda")
        eng = model.engine(**fw.engine_kw(c, route))
        assert eng._fast_weights_on()

        def call(inp):
            eng.pixel_weights = inp["pixel_weights"]     # (the shared weights are an input like x: flushed in the fill runs)
            eng.loss_and_grads(inp["x"], inp["eps"], 1.0)
        return wc.engine_run(eng, dict(x=cuda(x), eps=cuda(eps[0]), pixel_weights=eng.pixel_weights), call,
                             workspaces={"ws": wc.ivae_query(eng, c["b"])})
    return make


# ------------------------------------------------------------------------------- the layered path
def variant_cell(vname, fused=0):
    def make():
        model, cfg, o, x, y, g = variant_case(vname)
        eng = model.engine(fused=fused)
        b = x.shape[0]
        eps = torch.randn(b, cfg.z_dim, generator=g)
        if y is not None:
            x = x.flatten(1)
        outs = dict(z_loc=torch.empty(b, cfg.z_dim, device="cuda"), z_scale=torch.empty(b, cfg.z_dim, device="cuda"),
                    loc=torch.empty(b, cfg.n_pix, device="cuda"))

        def call(inp):
            eng.loss_and_grads(inp["x"], inp["eps"], 1.0, inp["y"], z_out=(outs["z_loc"], outs["z_scale"]), loc_out=outs["loc"])
        return wc.engine_run(eng, dict(x=cuda(x), eps=cuda(eps), y=cuda(y)), call, outs=outs, workspaces={"ws": wc.ivae_query(eng, b)})
    return make


# ------------------------------------------------------------------------------- convolutional networks
CONVENC = "ivaeconv_1d16_t_b5"
VED, VEDBN = "ved_1d32_to_1d32_small_b4", "vedbn_1d32_to_1d32_small_b4_relu"


def convenc_cell(fused, step=False):
    def make():
        gold = load_golden(CONVENC)
        meta, model, cfg = convenc_model(gold, "cuda")
        eng = model.engine(fused=fused)
        x = make_x(meta["xkind"], meta["batch"], meta["data_dim"])
        eps = torch.from_numpy(gold["s0.eps"])

        def call(inp):
            eng.loss_and_grads(inp["x"], inp["eps"], meta["beta"], step=step)
        return wc.engine_run(eng, dict(x=cuda(x), eps=cuda(eps)), call, workspaces={"ws": wc.ivae_query(eng, meta["batch"], beta=meta["beta"])},
                             step=step)
    return make


def convenc_bn_cell():
    """tests/test_gpu_parity.py: test_convenc_batchnorm_vs_oracle's model and data"""
    dd, inv, hid, b = (16, 16), ["r", "t"], [(8,), (16, 16)], 6
    model = pv.models.iVAE(dd, 2, inv, seed=1, device="cuda")
    model.set_encoder(pv.nets.convEncoderNet(dd, latent_dim=model.z_dim, hidden_dim=hid, batchnorm=True))
    eng = model.engine(fused=2)
    g = torch.Generator().manual_seed(3)
    x = torch.rand(b, *dd, generator=g)
    eps = torch.randn(b, model.z_dim, generator=g)

    def call(inp):
        eng.loss_and_grads(inp["x"], inp["eps"], 1.0)
    return wc.engine_run(eng, dict(x=cuda(x), eps=cuda(eps)), call, workspaces={"ws": wc.ivae_query(eng, b)})


def ved_cell(name, fused=2, bn=False):
    def make():
        gold = load_golden(name)
        if bn:
            c, model, cfg = vedbn_oracle(gold, "cuda")
        else:
            c = ved_case(gold)
            model = pv.models.VED(c["input_dim"], c["output_dim"], latent_dim=c["latent_dim"], seed=1, device="cuda", **c["kw"])
        eng = model.engine(fused=fused)
        x, y, eps = torch.from_numpy(gold["x"]), torch.from_numpy(gold["y"]), torch.from_numpy(gold["s0.eps"])
        b = x.shape[0]
        outs = dict(z_loc=torch.empty(b, model.z_dim, device="cuda"), z_scale=torch.empty(b, model.z_dim, device="cuda"),
                    loc=torch.empty(eng._out_shape(b), device="cuda"))

        def call(inp):
            eng.loss_and_grads(inp["x"], inp["eps"], c["beta"], inp["y"], z_out=(outs["z_loc"], outs["z_scale"]), loc_out=outs["loc"])
        return wc.engine_run(eng, dict(x=cuda(x), eps=cuda(eps), y=cuda(y)), call, outs=outs, workspaces={"ws": wc.ved_query(eng, b)})
    return make


# ------------------------------------------------------------------------------- other engines and call sequences
def ss_cell(name):
    """the unlabeled ELBO step of a semi-supervised fixture: classification enumerates the label (row_w, row_elbo on K B rows),
    regression samples it (dy); both run the label MLP forward and backward on its own workspace (ws_y)"""
    def make():
        gold = load_golden(name)
        meta = ssmeta_of(gold)
        model = ss_build(meta, "cuda")
        eng = model.engine(lr=5e-4, fused=2)
        b = meta["batch_u"]
        xu = torch.from_numpy(gold["xu"])[:b].reshape(b, -1)
        pre = next("c%d" % i for i in range(meta["calls"]) if str(gold["c%d.kind" % i]) == "u")
        eps = torch.from_numpy(gold[pre + ".eps"])
        eps_y = torch.from_numpy(gold[pre + ".eps_y"]) if (pre + ".eps_y") in gold else None
        rows = b * (meta["dim"] if meta["task"] == "classification" else 1)
        outs = dict(loss=torch.empty(1, device="cuda"))

        def call(inp):
            outs["loss"].copy_(eng.elbo_loss_and_grads(inp["x"], inp["eps"], None, inp["eps_y"], meta["beta"]).reshape(1))
        return wc.engine_run(eng, dict(x=cuda(xu), eps=cuda(eps), eps_y=cuda(eps_y)), call, outs=outs,
                             workspaces={"ws": wc.ivae_query(eng, rows, beta=meta["beta"]), "ws_y": wc.mlp_query(eng, b)})
    return make


class _UserEncoder(torch.nn.Module):
    def __init__(self, n_pix, z_dim):
        super().__init__()
        self.fc = torch.nn.Linear(n_pix, 24)
        self.mu, self.sig = torch.nn.Linear(24, z_dim), torch.nn.Linear(24, z_dim)

    def forward(self, x):
        h = torch.tanh(self.fc(x.flatten(1)))
        return self.mu(h), torch.nn.functional.softplus(self.sig(h)) + 1e-3


class _UserDecoder(torch.nn.Module):
    def __init__(self, data_dim, latent_dim):
        super().__init__()
        self.data_dim = data_dim
        self.fx, self.fz, self.o = torch.nn.Linear(2, 24), torch.nn.Linear(latent_dim, 24), torch.nn.Linear(24, 1)

    def forward(self, xc, z):
        h = torch.tanh(self.fx(xc) + self.fz(z).unsqueeze(1))
        return torch.sigmoid(self.o(h)).reshape(-1, *self.data_dim)


def _user_data(model, b=6, data_dim=(8, 8)):
    g = torch.Generator().manual_seed(2)
    return torch.rand(b, *data_dim, generator=g), torch.randn(b, model.z_dim, generator=g)


def user_encoder_cell():
    torch.manual_seed(5)
    model = pv.models.iVAE((8, 8), 2, ["r", "t", "s"], seed=1, device="cuda")
    user = _UserEncoder(64, model.z_dim)
    model.set_encoder(user)
    eng = model.engine(fused=2)
    x, eps = _user_data(model)

    def call(inp):
        eng.loss_and_grads(inp["x"], inp["eps"], 1.3)
    return wc.engine_run(eng, dict(x=cuda(x), eps=cuda(eps)), call, workspaces={"ws": wc.ivae_query(eng, 6, beta=1.3)},
                         extra_grads=lambda: {"user." + k: p.grad for k, p in user.named_parameters()})


def user_decoder_cell():
    """pv_ivae_guide -> the user's decoder in torch -> pv_ivae_guide_backward, inside one engine call: the workspace is poisoned
    before the guide only, as the header's pair demands"""
    torch.manual_seed(7)
    model = pv.models.iVAE((8, 8), 2, ["r", "t", "s"], seed=1, device="cuda")
    user = _UserDecoder((8, 8), 2)
    model.set_decoder(user)
    eng = model.engine()
    x, eps = _user_data(model)
    outs = dict(z_loc=torch.empty(6, model.z_dim, device="cuda"), z_scale=torch.empty(6, model.z_dim, device="cuda"))

    def call(inp):
        eng.loss_and_grads(inp["x"], inp["eps"], 1.3, z_out=(outs["z_loc"], outs["z_scale"]))
    return wc.engine_run(eng, dict(x=cuda(x), eps=cuda(eps)), call, outs=outs, workspaces={"ws": wc.ivae_query(eng, 6, beta=1.3)},
                         extra_grads=lambda: {"user." + k: p.grad for k, p in user.named_parameters()})


# ------------------------------------------------------------------------------- inference
def encode_cell():
    name = "e04_6x8_rt_b171"
    model = pc.make_model(name, "plain", "cuda")
    eng = model.engine(fused=2)
    x, _, _ = pc.inputs(name, "plain")
    B = x.shape[0]
    outs = dict(z_loc=torch.empty(B, model.z_dim, device="cuda"), z_scale=torch.empty(B, model.z_dim, device="cuda"))

    def call(inp):
        zl, zs = eng.encode(inp["x"])
        outs["z_loc"].copy_(zl)
        outs["z_scale"].copy_(zs)
    return wc.engine_run(eng, dict(x=cuda(x)), call, outs=outs, workspaces={"ws": wc.ivae_query(eng, B, what=2)},
                         want_grads=False, scalars=False)


def decode_cell(fused):
    """257 one-unit samples: fused = 2 runs the forward-only fused kernel (the `xdummy` fill), fused = 0 the layered kernels"""
    def make():
        name, n = "e01_1d16_t_b257", 257
        model = pc.make_model(name, "plain", "cuda")
        eng = model.engine(fused=fused)
        z = torch.randn(n, 2, generator=torch.Generator().manual_seed(2))
        outs = dict(loc=torch.empty(n, pc.n_pos(pc.CASES[name]), device="cuda"))

        def call(inp):
            outs["loc"].copy_(eng.decode(inp["z"], shift=(0.1, 0.0)).reshape(n, -1))
        return wc.engine_run(eng, dict(z=cuda(z)), call, outs=outs, workspaces={"ws": wc.ivae_query(eng, n, what=3)},
                             want_grads=False, scalars=False)
    return make


# ------------------------------------------------------------------------------- straight through the C ABI
class _Owner:
    """stands in for an engine: the attribute the kit installs the workspace on"""
    ws = None


def linear_cell(m, k, n, act="tanh"):
    """pv_linear_fwd / pv_linear_bwd as tests/test_gpu_parity.py: test_linear_fwd_bwd_blocks drives them"""
    def make():
        L = _abi.lib()
        g = torch.Generator().manual_seed(m * 7 + k)
        x, w = torch.randn(m, k, generator=g), torch.randn(n, k, generator=g) / k ** 0.5
        b, dy = torch.randn(n, generator=g), torch.randn(m, n, generator=g)
        own = _Owner()
        need = int(L.pv_linear_workspace_bytes(m, k, n))
        own.ws = torch.empty(need, dtype=torch.uint8, device="cuda")
        outs = dict(y=torch.empty(m, n, device="cuda"), dx=torch.empty(m, k, device="cuda"), dw=torch.empty(n, k, device="cuda"),
                    db=torch.empty(n, device="cuda"))

        def call(inp):
            ws = own.ws
            wsp = C.c_void_p(ws.data_ptr() if ws.numel() else (ws._base.data_ptr() + ws.storage_offset() if ws._base is not None else 0))
            st = _abi.current_stream()
            _abi.check(L.pv_linear_fwd(_abi.ptr(inp["x"]), k, _abi.ptr(inp["w"]), _abi.ptr(inp["b"]), _abi.ptr(outs["y"]), None, n,
                                       m, k, n, _abi.ACT[act], wsp, ws.numel(), st), "pv_linear_fwd")
            _abi.check(L.pv_linear_bwd(_abi.ptr(inp["dy"]), n, _abi.ptr(inp["x"]), k, _abi.ptr(inp["w"]), _abi.ptr(outs["dx"]), k,
                                       None, None, 0, 0, _abi.ptr(outs["dw"]), _abi.ptr(outs["db"]), m, k, n, wsp, ws.numel(), st),
                       "pv_linear_bwd")
        return wc.Run(own, {"ws": lambda: L.pv_linear_workspace_bytes(m, k, n)}, dict(x=cuda(x), w=cuda(w), b=cuda(b), dy=cuda(dy)),
                      call, outs=outs, writes_ws=max(m, k, n) > 128)      # (5, 3, 7): no split contraction, the scratch stays unused)
    return make


def convnet_cell():
    """pv_convnet_forward -> pv_convnet_backward on the smallest standalone stack of tests/test_gpu_conv_kernels.py (its case
    fe2d_bn, restated: a batch-norm FeatureExtractor on (5, 1, 8, 8), no input gradient — so with max-pool winner bytes), through
    ops._stack_plan.  The pair keeps the workspace: poisoned before the forward only."""
    from pyroved_amd.nets.conv import FeatureExtractor
    from pyroved_amd._convplan import conv_ops
    spec, shape = dict(ndim=2, in_ch=1, filters=[(8,), (16,)], bn=True, act="lrelu"), (5, 1, 8, 8)
    torch.manual_seed(3)
    net = FeatureExtractor(spec["ndim"], spec["in_ch"], spec["filters"], batchnorm=spec["bn"], activation=spec["act"]).cuda()
    x = torch.randn(*shape, generator=torch.Generator().manual_seed(1))
    ops_list = conv_ops(net.layers, net.activation, "L")
    named = ops._stack_tensors(ops_list)
    layout, off = {}, 0
    for key, t, _ in named:
        layout[key] = off
        off += (t.numel() + 63) // 64 * 64
    flat0 = torch.zeros(off, device="cuda")
    for key, t, _ in named:
        flat0[layout[key]:layout[key] + t.numel()].copy_(t.detach().reshape(-1))
    flat, grads = flat0.clone(), torch.zeros(off, device="cuda")
    L = _abi.lib()
    plan, need = ops._stack_plan(net, x.cuda(), ops_list, layout)
    assert need > 0 and plan.need_dx == 0
    shp = (C.c_int32 * 3)()
    _abi.check(L.pv_convnet_out_shape(C.byref(plan), shp), "pv_convnet_out_shape")
    out_shape = (shape[0], shp[0]) + tuple(shp[1:1 + spec["ndim"]])
    dout = torch.randn(*out_shape, generator=torch.Generator().manual_seed(2))
    own = _Owner()
    own.ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    outs = dict(out=torch.empty(out_shape, device="cuda"))

    def call(inp):
        plan.params, plan.grads = flat.data_ptr(), grads.data_ptr()
        plan.ws, plan.ws_bytes = own.ws.data_ptr(), own.ws.numel()
        st = _abi.current_stream()
        _abi.check(L.pv_convnet_forward(C.byref(plan), _abi.ptr(inp["x"]), _abi.ptr(outs["out"]), st), "pv_convnet_forward")
        _abi.check(L.pv_convnet_backward(C.byref(plan), _abi.ptr(inp["x"]), _abi.ptr(inp["dout"]), None, st), "pv_convnet_backward")

    def grad_views():
        return {key: grads[layout[key]:layout[key] + t.numel()] for key, t, is_param in named if is_param}

    def stats():
        return {key: flat[layout[key]:layout[key] + t.numel()] for key, t, is_param in named if not is_param}
    return wc.Run(own, {"ws": lambda: L.pv_convnet_workspace_bytes(C.byref(plan))}, dict(x=cuda(x), dout=cuda(dout)), call, outs=outs,
                  grads=grad_views, state=stats, poison=lambda: grads.fill_(float("nan")), restore=lambda: flat.copy_(flat0))


# ------------------------------------------------------------------------------- the table
CELLS = {}
for _name, _fams in PARTITION_CELLS:
    for _f in _fams:
        CELLS["%s-%s" % (_name, _f)] = partition_cell(_name, _f)
CELLS.update({
    "renyi_8x8_rts_b6_p3": renyi_cell,
    "analytic_kl_e09_1d16_t_b256": analytic_cell,
    "poisson_8x8_rts_b6-fused0": poisson_cell(0),
    "poisson_8x8_rts_b6-fused2": poisson_cell(2),
    "image_weights_i01": image_weights_cell,
    "fast_weights_f01-x3": fast_weights_cell("x3"),
    "fast_weights_f01-bf16": fast_weights_cell("bf16"),
    "layered_gauss_rts": variant_cell("gauss_rts"),
    "layered_gelu_r": variant_cell("gelu_r"),
    "layered_lrelu_none": variant_cell("lrelu_none"),
    "convenc_1d16_t_b5-fused0": convenc_cell(0),
    "convenc_1d16_t_b5-fused2": convenc_cell(2),
    "convenc_batchnorm_16x16_rt_b6": convenc_bn_cell,
    "ved_1d32_b4-fp32": ved_cell(VED, 2),
    "ved_1d32_b4-bf16": ved_cell(VED, 3),
    "vedbn_1d32_b4_relu": ved_cell(VEDBN, 2, bn=True),
    "sscls_1d16_t_k2": ss_cell("sscls_1d16_t_k2"),
    "ssreg_8x8_rt_c2": ss_cell("ssreg_8x8_rt_c2"),
    "user_encoder_8x8_rts_b6": user_encoder_cell,
    "user_decoder_8x8_rts_b6": user_decoder_cell,
    "encode_e04_6x8_rt_b171": encode_cell,
    "decode_1d16_t_n257-fused2": decode_cell(2),
    "decode_1d16_t_n257-fused0": decode_cell(0),
    "eval_e09_1d16_t_b256-x3": partition_cell("e09_1d16_t_b256", "x3", want_grads=False),
    "step_e09_1d16_t_b256-x3": partition_cell("e09_1d16_t_b256", "x3", step=True),
    "step_e09_1d16_t_b256-bf16w8": partition_cell("e09_1d16_t_b256", "bf16w8", step=True),
    "step_e05_28x28_rt_b6-x3": partition_cell("e05_28x28_rt_b6", "x3", step=True),
    "step_convenc_1d16_t_b5-fused2": convenc_cell(2, step=True),
    "linear_5x3x7": linear_cell(5, 3, 7),
    "linear_200x784x128": linear_cell(200, 784, 128),
    "convnet_fe2d_bn_5x1x8x8": convnet_cell,
})

# cells of the plan that no engine runs: (id, what is asked, the exception, the words of the reason)
REFUSED = [
    # the one-call step of VED exists only as the data-parallel pv_ved_dp_step (out of scope here): VEDEngine has no single-process form
    ("step_ved_1d32_b4", "VED one-call step", ValueError, "data-parallel step"),
    # a family the partition kit refuses for the case (tests/_partition_cases.refusal)
    ("e11_p3_1d16_t_b86-f32", "particles on the f32 kernel", ValueError, "particles"),
    ("e10_jivae_k3_1d16_t_b86-w1", "pixel_weights on a jiVAE", ValueError, "pixel_weights"),
    # the one-call step with a user-defined module
    ("step_user_encoder", "one-call step with a user-defined encoder", ValueError, "step=True needs every parameter"),
]


_GPU_ERROR = []                                         # a cell that ended in anything but an assertion: nothing more runs on the device


@pytest.mark.parametrize("cell", list(CELLS), ids=list(CELLS))
def test_workspace_contract(gpu_device, cell):
    if _GPU_ERROR:
        pytest.fail("not run: the cell %s ended in an error (%s); no further call goes to the device in this process" % _GPU_ERROR[0])
    try:
        wc.run_cell(cell, CELLS[cell], report=_report)
    except AssertionError:
        raise
    except Exception as e:
        _GPU_ERROR.append((cell, "%s: %s" % (type(e).__name__, str(e)[:200])))
        raise


def test_every_cell_is_run_or_refused_with_a_reason(gpu_device):
    """What the table lists as refused, the engines refuse, in these words."""
    ran = set(CELLS)
    for cid, what, exc, words in REFUSED:
        assert cid not in ran, cid
        if cid == "step_ved_1d32_b4":
            run = ved_cell(VED, 2)()
            assert run.eng.supports_step is False
            inp = run.inputs
            with pytest.raises(exc, match=words):
                run.eng.loss_and_grads(inp["x"], inp["eps"], 1.0, inp["y"], step=True)
        elif cid == "step_user_encoder":
            run = user_encoder_cell()
            with pytest.raises(exc, match=words):
                run.eng.loss_and_grads(run.inputs["x"], run.inputs["eps"], 1.0, step=True)
        else:
            name, family = cid.rsplit("-", 1)
            assert pc.refusal(name, family)
            with pytest.raises(exc, match=words):
                partition_engine(name, family)
    # every cell of the plan is in exactly one of the two lists
    for name, fams in PARTITION_CELLS:
        for f in fams:
            assert ("%s-%s" % (name, f) in ran) != bool(pc.refusal(name, f)), (name, f)
