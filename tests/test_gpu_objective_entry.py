"""
GPU tests (-m gpu) of the step's objective as one descriptor: pv_ivae_objective_loss_and_grads / pv_ivae_objective_step against
the entry point each descriptor stands for (pv_ivae_* / pv_ivae_particles_* / pv_ivae_renyi_* / pv_ivae_weighted_* /
pv_ivae_weighted_images_*).  Both spellings reach the same launches, so what can break is argument forwarding, not arithmetic:
every cell runs the same inputs through the old function and through the unified one with the equivalent descriptor — raw
library calls on the plan the engine builds, with the pointers set the way IVAEEngine.loss_and_grads sets them, from the same
parameters, moments and adam_step — and every result must have the same bits: the four scalars, the flat gradient, after a step
the parameters and both moments, z_loc / z_scale, loc and the Renyi weights.  The unified route runs twice (bit-reproducible).
The shapes are the smallest that reach each forwarding path: (8, 8) images, batch 6 — 24 units of 16 rows, fewer than the
workgroups the fused kernels could start; one more cell at batch == number of CUs, the only shape at which the bf16 throughput
step folds its guide into the decoder launch (pv_ivae_guide_folds) and closes with Adam in its last gradient launch.
The arithmetic behind the unified calls is judged by the oracle suites, which reach every objective through them.
"""
import ctypes as C

import pytest
import torch

import pyroved_amd as pv
from pyroved_amd import _abi
import _multichannel_cases as mc
import _pixel_weight_cases as pw
import _image_weight_cases as iwc

pytestmark = pytest.mark.gpu

BETA, ALPHA, POISON = 1.3, 0.5, -7.5
ELBO, RENYI = _abi.PV_BOUND_ELBO, _abi.PV_BOUND_RENYI
NONE, SHARED, PER_IMAGE = _abi.PV_OBS_W_NONE, _abi.PV_OBS_W_SHARED, _abi.PV_OBS_W_PER_IMAGE
CALLS = ("loss", "grads", "step")

RTS = dict(dims=(8, 8), inv=["r", "t", "s"], C=1, b=6)
POISSON = dict(dims=(8, 8), inv=["r"], C=1, b=6, sampler="poisson_log", sigmoid_d=False)
VANILLA = dict(dims=(8, 8), inv=None, C=1, b=6)
# name -> (engine keywords, particles, alpha or None, obs_w_kind)
DESCRIPTORS = {
    "plain": (dict(), 1, None, NONE),
    "particles3": (dict(particles=3), 3, None, NONE),
    "renyi3": (dict(particles=3, renyi=ALPHA), 3, ALPHA, NONE),
    "renyi1": (dict(particles=1, renyi=ALPHA), 1, ALPHA, NONE),
    "shared": (dict(pixel_weights=pw.disc((8, 8), 1)[..., 0]), 1, None, SHARED),
    "per_image": (dict(image_weights=True), 1, None, PER_IMAGE),
}


def image_weights(b):
    """a disc per image, image 2 masked out completely"""
    w = iwc.pdisc(b, (8, 8), 1)
    w[2] = 0.0
    return w.reshape(b, -1)


class Routes:
    """One engine, one set of inputs, and the two spellings of each of the three calls."""

    def __init__(self, c, desc, **engine_kw):
        kw, self.P, self.alpha, self.kind = DESCRIPTORS[desc]
        model = pv.models.iVAE(c["dims"], 2, c["inv"], seed=1, device="cuda", **mc.model_kwargs(c))
        self.eng = eng = model.engine(**dict(kw, **engine_kw))
        self.b = b = c["b"]
        x, _, eps = mc.case_data(c, self.P)
        self.x = x.reshape(b, -1).cuda().contiguous()
        self.eps = eps[0].cuda().contiguous()
        n_pix, z = self.x.shape[1], model.z_dim
        self.w = eng.pixel_weights if self.kind == SHARED else image_weights(b).cuda().contiguous() if self.kind == PER_IMAGE else None
        self.outs = dict(z_loc=torch.empty(b, z, device="cuda"), z_scale=torch.empty(b, z, device="cuda"),
                         loc=torch.empty(self.P * b, n_pix, device="cuda"))
        if self.alpha is not None:
            self.outs["weights"] = torch.empty(self.P * b, device="cuda")
        self.saved = (eng.flat.clone(), eng.m.clone(), eng.v.clone())

    def plan(self, step):
        """eng._plan's plan with the pointers IVAEEngine.loss_and_grads sets"""
        eng, o = self.eng, self.outs
        p = eng._plan(self.b, BETA)
        p.x, p.eps = self.x.data_ptr(), self.eps.data_ptr()
        p.z_loc, p.z_scale, p.loc = o["z_loc"].data_ptr(), o["z_scale"].data_ptr(), o["loc"].data_ptr()
        if step:
            p.lr, p.adam_beta1, p.adam_beta2, p.adam_eps = eng.lr, eng.betas[0], eng.betas[1], eng.adam_eps
            p.adam_step = eng.adam_t + 1
        return p

    def old(self, p, call):
        L, r, s, g = _abi.lib(), C.byref(p), _abi.current_stream(), int(call == "grads")
        wout, w = _abi.ptr(self.outs.get("weights")), _abi.ptr(self.w)
        if self.alpha is not None:
            return ("pv_ivae_renyi_step", L.pv_ivae_renyi_step(r, self.P, self.alpha, wout, s)) if call == "step" else \
                   ("pv_ivae_renyi_loss_and_grads", L.pv_ivae_renyi_loss_and_grads(r, self.P, self.alpha, g, wout, s))
        if self.P > 1:
            return ("pv_ivae_particles_step", L.pv_ivae_particles_step(r, self.P, s)) if call == "step" else \
                   ("pv_ivae_particles_loss_and_grads", L.pv_ivae_particles_loss_and_grads(r, self.P, g, s))
        if self.kind == SHARED:
            return ("pv_ivae_weighted_step", L.pv_ivae_weighted_step(r, w, s)) if call == "step" else \
                   ("pv_ivae_weighted_loss_and_grads", L.pv_ivae_weighted_loss_and_grads(r, w, g, s))
        if self.kind == PER_IMAGE:
            return ("pv_ivae_weighted_images_step", L.pv_ivae_weighted_images_step(r, w, s)) if call == "step" else \
                   ("pv_ivae_weighted_images_loss_and_grads", L.pv_ivae_weighted_images_loss_and_grads(r, w, g, s))
        return ("pv_ivae_step", L.pv_ivae_step(r, s)) if call == "step" else ("pv_ivae_loss_and_grads", L.pv_ivae_loss_and_grads(r, g, s))

    def objective(self):
        o = _abi.pv_ivae_objective()
        o.num_particles, o.bound, o.alpha = self.P, (ELBO if self.alpha is None else RENYI), (self.alpha or 0.0)
        o.obs_w_kind = self.kind
        o.obs_w = self.w.data_ptr() if self.w is not None else None
        o.weights_out = self.outs["weights"].data_ptr() if "weights" in self.outs else None
        return o

    def new(self, p, call):
        L, r, s, o = _abi.lib(), C.byref(p), _abi.current_stream(), self.objective()
        if call == "step":
            return "pv_ivae_objective_step", L.pv_ivae_objective_step(r, C.byref(o), s)
        return "pv_ivae_objective_loss_and_grads", L.pv_ivae_objective_loss_and_grads(r, C.byref(o), int(call == "grads"), s)

    def run(self, route, call):
        """One call from the saved parameters and moments, every output and the gradient buffer (scalars included) poisoned first."""
        eng = self.eng
        for buf, was in zip((eng.flat, eng.m, eng.v), self.saved):
            buf.copy_(was)
        eng.grad.fill_(POISON)
        for t in self.outs.values():
            t.fill_(POISON)
        torch.cuda.synchronize()
        name, code = route(self.plan(call == "step"), call)
        _abi.check(code, name)
        torch.cuda.synchronize()
        snap = dict(scalars=eng.scalars.clone(), grad=eng.grad[:eng.n_flat].clone(), **{k: v.clone() for k, v in self.outs.items()})
        if call == "step":
            snap.update(params=eng.flat.clone(), m=eng.m.clone(), v=eng.v.clone())
        return snap


def check_cell(c, desc, **engine_kw):
    r = Routes(c, desc, **engine_kw)
    tag = "%s %s %s" % (c["inv"], desc, engine_kw)
    for call in CALLS:
        old, new, again = r.run(r.old, call), r.run(r.new, call), r.run(r.new, call)
        for k in old:
            assert torch.equal(old[k], new[k]), "%s, %s: %s differs between the old and the unified entry point" % (tag, call, k)
            assert torch.equal(new[k], again[k]), "%s, %s: %s differs between two unified calls" % (tag, call, k)
        # the comparison is not one of untouched buffers
        for k in ("scalars", "z_loc", "z_scale", "loc"):
            assert bool(torch.isfinite(new[k]).all()) and not bool((new[k] == POISON).any()), (tag, call, k)
        if call == "grads":
            for key in r.eng._views:                         # (per tensor: the flat buffer's alignment padding is nobody's to write)
                g = r.eng.grad_of(key)                       # (the last unified call's, whose bits are `new`'s)
                assert bool(torch.isfinite(g).all()) and not bool((g == POISON).any()) and float(g.abs().max()) > 0.0, (tag, key)
        if call == "step":                                   # both routes leave the gradients zeroed and the parameters moved
            for key, v in r.eng._views.items():             # (per tensor, as above)
                at = r.eng._layout[key]
                for snap in (old, new):
                    assert float(snap["grad"][at:at + v.numel()].abs().max()) == 0.0, (tag, "zero_grads", key)
            assert not torch.equal(new["params"], r.saved[0]) and bool(torch.isfinite(new["params"]).all())
        if r.alpha is not None:
            w = new["weights"].reshape(r.P, r.b)
            if r.P == 1:
                assert bool((w == 1.0).all()), (tag, call, "one particle: every weight is 1")
            else:
                assert bool((w > 0).all()) and float((w.sum(0) - 1.0).abs().max()) < 1e-5, (tag, call)
    return r


# ------------------------------------------------------------------------------- A. plain, particles, the Renyi bound
@pytest.mark.parametrize("desc", ["plain", "particles3", "renyi3", "renyi1"])
@pytest.mark.parametrize("fused", [0, 2, 3])
def test_plain_particles_and_renyi(gpu_device, fused, desc):
    check_cell(RTS, desc, fused=fused)


def test_folded_guide_step_with_the_plain_descriptor(gpu_device):
    """batch == number of CUs on the bf16 throughput path: the guide rides in the decoder launch and the step closes with Adam in
    its last gradient launch — the unified step must take that route as pv_ivae_step does (the same bits, zeroed gradients)."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    r = check_cell(dict(dims=(16, 16), inv=["r", "t", "s"], C=1, b=cus), "plain", fused=3)
    assert _abi.lib().pv_ivae_guide_folds(C.byref(r.plan(True))) == 1


# ------------------------------------------------------------------------------- B. weights, shared and per image
@pytest.mark.parametrize("desc", ["shared", "per_image"])
@pytest.mark.parametrize("fused", [0, 1, 2])
def test_weights(gpu_device, fused, desc):
    r = check_cell(RTS, desc, fused=fused)
    assert r.eng.uses_fused(r.b) is (fused != 0)


@pytest.mark.parametrize("desc", ["shared", "per_image"])
@pytest.mark.parametrize("fused", [2, 3])
def test_weights_on_the_bf16_class_kernels(gpu_device, fused, desc):
    r = check_cell(RTS, desc, fused=fused, fast_weights=True)
    assert r.plan(False).flags & _abi.PV_PLAN_FAST_WEIGHTS and r.plan(False).fused == fused


@pytest.mark.parametrize("desc", ["shared", "per_image"])
@pytest.mark.parametrize("fused", [0, 2])
def test_weights_reach_the_poisson_normaliser(gpu_device, fused, desc):
    """Poisson counts: the weighted normaliser launch gets the same weights from both spellings — and they do arrive: with the
    plain descriptor on the same plan scalars[1] is another number."""
    r = check_cell(POISSON, desc, fused=fused)
    weighted = r.run(r.new, "loss")["scalars"]
    r.kind, r.w = NONE, None
    plain = r.run(r.new, "loss")["scalars"]
    assert abs(float(plain[1]) - float(weighted[1])) > 1e-3 * abs(float(plain[1]))


# ------------------------------------------------------------------------------- C. vanilla decoder
@pytest.mark.parametrize("desc", ["plain", "particles3", "shared"])
def test_vanilla_decoder(gpu_device, desc):
    check_cell(VANILLA, desc, fused=0)


# ------------------------------------------------------------------------------- D. refusals
def test_mixed_descriptor_is_refused_by_the_library_and_by_the_engine(gpu_device):
    """Weights together with three particles: the library answers PV_EINVAL (PvError through _abi.check) on a plan that is
    otherwise complete; the engine never gets that far — it raises its own ValueError when it is configured."""
    r = Routes(RTS, "shared", fused=0)
    o = r.objective()
    o.num_particles = 3
    for name, code in (("pv_ivae_objective_loss_and_grads",
                        _abi.lib().pv_ivae_objective_loss_and_grads(C.byref(r.plan(False)), C.byref(o), 1, _abi.current_stream())),
                       ("pv_ivae_objective_step", _abi.lib().pv_ivae_objective_step(C.byref(r.plan(True)), C.byref(o), _abi.current_stream()))):
        with pytest.raises(_abi.PvError, match="%s failed with PV_EINVAL" % name):
            _abi.check(code, name)
    assert _abi.lib().pv_ivae_objective_workspace_bytes(C.byref(r.plan(False)), C.byref(o)) == -1
    model = pv.models.iVAE((8, 8), 2, ["r", "t", "s"], seed=1, device="cuda")
    with pytest.raises(ValueError, match="one-particle ELBO only"):
        model.engine(fused=0, particles=3, image_weights=True)
