"""
engine.py — host-side driver of the HIP SVI step for models.iVAE.

Owns the device memory layout the C ABI works on:
  * ONE flat fp32 parameter buffer; every nn.Parameter of the model's encoder_z
    and decoder is re-pointed to a view of it (state_dict keys and values are
    unchanged, save/load keep working), laid out so that fc11/fc12 are adjacent
    (the kernels treat them as one Linear of width 2*z_dim);
  * flat gradient buffer with 4 trailing slots for the ELBO scalars, so that the
    data-parallel path needs exactly one all-reduce (grads + loss);
  * flat Adam moment buffers and the workspace.
and fills a `pv_ivae_plan` (include/pyroved_amd.h) per call.

Replaces, for the product, what Pyro's SVI/Trace_ELBO/PyroOptim objects hold in
the reference (pyroved/trainers/svi.py:79-91).
"""
import ctypes as C
import math
from typing import Dict, List, Optional

import torch
import torch.nn as nn

from . import _abi
from .nets.fc import fcEncoderNet, jfcEncoderNet, fcDecoderNet, sDecoderNet
from .nets.conv import convEncoderNet
from ._convplan import UnsupportedModel, conv_ops, fill_ops, bn_modules

ALIGN = 64      # floats: every tensor starts on a 256-byte boundary of the flat buffer
N_SCALARS = 4   # loss, ll, beta*log p(z), beta*log q(z|x)  (kl="analytic": the last two are those terms' expectations under q)


def _kl_name(kl) -> str:
    if kl not in _abi.KL:
        raise ValueError("kl must be 'sampled' or 'analytic' (got %r)" % (kl,))
    return kl


def _particle_count(p) -> int:
    if isinstance(p, bool) or not isinstance(p, int) or p < 1:
        raise ValueError("particles must be an int >= 1 (got %r)" % (p,))
    return p


def _renyi_alpha(a) -> Optional[float]:
    """None / False: the ELBO.  A float: the order alpha of the importance-weighted (Renyi) bound — finite and not 1."""
    if a is None or a is False:
        return None
    if isinstance(a, bool) or not isinstance(a, (int, float)):
        raise ValueError("renyi must be None or the bound's order alpha, a float (got %r)" % (a,))
    a = float(a)
    if not math.isfinite(a) or a == 1.0:
        raise ValueError("renyi: alpha must be a finite float other than 1 (got %r); alpha -> 1 is the multi-particle ELBO, "
                         "which particles=P without renyi computes" % (a,))
    return a


def _image_weights_flag(v) -> bool:
    """image_weights of engine() / configure(): a switch — the weights themselves come with every loss_and_grads call."""
    if v is None:
        return False
    if not isinstance(v, bool):
        raise ValueError("image_weights must be True or False here: the weights of a batch go to loss_and_grads(..., "
                         "image_weights=w) (got %s)" % type(v).__name__)
    return v


def _linears(seq: nn.Sequential) -> List[nn.Linear]:
    return [m for m in seq if isinstance(m, nn.Linear)]


# settings as given -> as the engine keeps them (pixel_weights needs the model: IVAEEngine._pixel_weight_tensor)
_NORMALISE = dict(fused=int, kl=_kl_name, particles=_particle_count, renyi=_renyi_alpha, fused_channels=bool,
                  image_weights=_image_weights_flag, fast_weights=bool, fused_any_size=bool)


class IVAEEngine:
    """Binds an iVAE-like model (encoder_z: fcEncoderNet, decoder: sDecoderNet | fcDecoderNet) to the HIP library.
    A multi-channel model (models.iVAE(..., channels=C), self.C > 1) takes x as (B, *data_dim, C), channel-last, and returns loc /
    decode in that shape.  The settings — fused, kl, particles, renyi, fused_channels, pixel_weights, image_weights, fast_weights,
    fused_any_size,
    each described at its class default below — are plain attributes read at every call; model.engine(**kw) and configure(**kw)
    set them.  Which combinations a model takes, and every refusal's text, is `_validate`'s rule list; which kernels a combination
    runs on is `_plan_fused` / `_plan_flags`.  Per-batch weights come with every call: loss_and_grads(..., image_weights=w)."""
    supports_scalars_out = True      # loss_and_grads can write the 4 loss scalars to a caller-given device slot
    supports_step = True             # loss_and_grads(step=True) = SVI.step in one library call
    # per-plan switches (ABI v14 / v15 plan fields; the library keeps no process-wide switch).  Set on an engine — or, in tests,
    # on the class — before the next call:
    dec_kernel = 0                   # pv_ivae_plan.dec_kernel: 0 = the library picks the decoder-kernel build by problem size
    enc_two_launch = False           # PV_PLAN_ENC_TWO_LAUNCH
    enc_no_wait = False              # PV_PLAN_ENC_NO_WAIT: the one-launch encoder's consumers compute their tiles themselves
    side_stream = True               # PV_PLAN_NO_SIDE_STREAM when False
    dec1d = True                     # PV_PLAN_NO_DEC1D when False (VED's Conv1d decoder layer by layer)
    enc_per_image = True             # the guide of a training step as one workgroup per image (False: PV_PLAN_ENC_TILED, the tiled one-launch encoder)
    conv_x3 = False                  # PV_PLAN_CONV_X3 / conv_bf16 = 0: fp32-class kernel-3 convolutions with both operands as two fp16 pieces
    enc_fold = True                  # PV_PLAN_NO_ENC_FOLD when False (the guide as its own launch even where the decoder launch could host it)
    full_tile_loop = True            # PV_PLAN_GENERIC_TILE_LOOP when False (the image-owning decoder launch keeps its generic tile loop; bit-identical)
    conv_events = None               # (start, stop, ctypes double for the launch's FLOPs) around the convolution launches, or None
    # the model's facts, established once by _check_model (set_encoder / set_decoder drop the engine):
    K = 0                            # classes of the discrete latent (jiVAE)
    C = 1                            # channels per grid position (models.iVAE(..., channels=C))
    conv_enc = False                 # encoder_z is a convEncoderNet
    ext_enc = ext_dec = False        # encoder_z / decoder is a user-defined module: it runs in torch
    ext_y = False                    # ... and so is the label network (SSEngine)
    own_fc = False                   # models.iVAE itself with its own fully connected encoder and decoder
    fw_blocker = None                # why the weighted bf16-class decoder kernel does not take this model (None: it does)
    # the settings (model.engine(**kw) / configure(**kw): normalise -> _validate -> assign):
    fused = 2                        # 0 layered kernels, 1 fused f32-MFMA decoder, 2 fused bf16x3 decoder, 3 fused plain-bf16 decoder
    fused_channels = False           # PV_PLAN_FUSED_CHANNELS (with C > 1 and fused = 1 or 2): the multi-channel fused f32 decoder kernel
                                     # (fp32-class; decoder hidden [128, 128], tanh, positions a multiple of 16 — layered elsewhere)
    kl = "sampled"                   # pv_ivae_plan.kl_mode / pv_ved_plan.kl_mode: "sampled" log q(z|x) - log p(z) at the drawn z
                                     # (Trace_ELBO) or "analytic", the closed-form KL(q || N(0, 1)) (TraceMeanField_ELBO)
    particles = 1                    # particles of the ELBO estimate (num_particles of the Pyro ELBO objects) — pv_ivae_particles_*
    renyi = None                     # None: the ELBO; a float alpha != 1: the importance-weighted bound of that order over the
                                     # `particles` samples (pyro.infer.RenyiELBO(alpha, num_particles); 0 = IWAE) — pv_ivae_renyi_*
    pixel_weights = None             # None, or the per-observation weights of the likelihood, shared by all images: one contiguous
                                     # float32 tensor of n_pix values (positions x channels, channel-last), on the device once the
                                     # engine is bound — pv_ivae_weighted_* (training step, evaluate, elbo_terms; not encode / decode)
    image_weights = False            # True: every loss_and_grads call takes image_weights=w, one weight >= 0 per observed value of
                                     # every image of the batch (x must be finite also where w = 0) — pv_ivae_weighted_images_*;
                                     # with pixel_weights as well the library gets the product
    fast_weights = False             # PV_PLAN_FAST_WEIGHTS: weighted steps on the 4-wave bf16-class fused decoder kernel (fused = 2:
                                     # where the model is one it takes, fp32-class results; fused = 3: refused elsewhere)
    fused_any_size = False           # PV_PLAN_FUSED_TAIL (with fused = 1 or 2): a spatial model whose grid positions are no multiple
                                     # of 16 runs on the fused f32 decoder kernel's tail form instead of the layer-by-layer kernels
                                     # (fp32-class; models.iVAE, decoder hidden [128, 128], tanh, per-value likelihoods, one channel —
                                     # or several with fused_channels; everything else keeps today's routing: _any_size_on)
    _ev_ws = None                    # log_evidence_chunk: the evidence workspace (grows to the largest layout asked for) and the
    _ev_need = None                  # sizes the library answered, per (batch, P, fused)
    _snap = None                     # _bound's snapshot of the module tree
    _conv_slices = None              # _check_conv_weight_range's weight slices (None: derive them at the next call)

    def __init__(self, model, lr: float = 1e-3, betas=(0.9, 0.999), eps: float = 1e-8, fused: int = 2, kl: str = "sampled",
                 particles: int = 1, renyi=None, fused_channels: bool = False, pixel_weights=None,
                 image_weights: bool = False, fast_weights: bool = False, fused_any_size: bool = False):
        self.model = model
        new = self._normalise(dict(image_weights=image_weights, fast_weights=fast_weights, fused_channels=fused_channels, kl=kl,
                                   particles=particles, renyi=renyi, fused=fused, fused_any_size=fused_any_size))
        self.lr, self.betas, self.adam_eps = float(lr), (float(betas[0]), float(betas[1])), float(eps)
        self.adam_t = 0                 # number of optimizer steps taken (incl. evaluate()'s, see SVItrainer)
        self.grads_live = False         # reference: .grad is None until the first backward
        self.device = None
        self.flat = self.grad = self.m = self.v = None
        self.ws = None
        self.events = (None, None)      # optional raw hipEvent_t pair recorded around the dominant kernel
        self._bn_enc, self._bn_dec = [], []   # batch-norm modules of the convolutional stacks
        self._enc_opt = None            # torch.optim.Adam of a user-defined encoder's parameters (ext_enc)
        self._enc_params = []
        self._layout: Dict[str, int] = {}
        self._views: Dict[str, torch.Tensor] = {}
        self._check_model()
        self.own_fc = type(self) is IVAEEngine and not (self.conv_enc or self.ext_enc or self.ext_dec)
        self.fw_blocker = self._fast_weights_blocker()
        new.update(self._normalise(dict(pixel_weights=pixel_weights)))      # (needs C)
        self._validate(dec_kernel=self.dec_kernel, **new)
        vars(self).update(new)
        self.bind()

    # ------------------------------------------------------------------ structure
    def _check_model(self):
        m = self.model
        enc, dec = m.encoder_z, m.decoder
        self.conv_enc = isinstance(enc, convEncoderNet)          # iVAE.set_encoder(convEncoderNet(...))
        # any other user module (models/base.py:173-177: "Sets a user-defined encoder neural network") runs in PyTorch
        # on the device: its (z_loc, z_scale) outputs enter the HIP step through plan.ext_head, the gradients come back
        # through plan.ext_dhead and are back-propagated with torch.autograd; its parameters get their own Adam
        self.ext_enc = not isinstance(enc, (fcEncoderNet, jfcEncoderNet, convEncoderNet))
        # a user-defined decoder (models/base.py:179-183) likewise: the library runs the guide half of the step
        # (pv_ivae_guide / pv_ivae_guide_backward), the decoder, the coordinate transform and the likelihood run in PyTorch
        self.ext_dec = not isinstance(dec, (sDecoderNet, fcDecoderNet))
        # channels per grid position (models.iVAE(..., channels=C)): observations are channel-last, n_pix = positions * C
        self.C = int(getattr(m, "channels", 1))
        if self.C != 1:
            if type(self) is not IVAEEngine or isinstance(enc, jfcEncoderNet):
                raise UnsupportedModel("channels=%d: multi-channel data is implemented for models.iVAE only (not for %s)"
                                       % (self.C, type(m).__name__))
            if isinstance(self.C, bool) or not 1 <= self.C <= _abi.PV_MAX_CHANNELS:
                raise UnsupportedModel("channels must be an int in 1 .. %d (got %r)" % (_abi.PV_MAX_CHANNELS, self.C))
            if self.ext_enc or self.conv_enc or self.ext_dec:
                raise UnsupportedModel("channels=%d: a multi-channel model needs its own fully connected encoder and decoder "
                                       "(no convolutional or user-defined networks)" % self.C)
            if isinstance(dec, sDecoderNet) and dec.out.out_features != self.C:
                raise UnsupportedModel("channels=%d, but decoder.out has %d outputs" % (self.C, dec.out.out_features))
        if self.ext_dec:
            if getattr(m, "discrete_dim", 0):
                raise UnsupportedModel("a user-defined decoder cannot be combined with discrete latents here")
            if m.sampler_d.name not in _abi.LIK:
                raise UnsupportedModel("decoder sampler %r is not implemented" % m.sampler_d.name)
        if self.ext_enc:
            if getattr(m, "c_dim", 0) != 0 or getattr(m, "discrete_dim", 0):
                raise UnsupportedModel("a user-defined encoder cannot be combined with c_dim / discrete latents here")
        elif self.conv_enc:
            if tuple(enc.input_dim) != tuple(int(d) for d in m.data_dim) or enc.input_channels != 1:
                raise UnsupportedModel("conv encoder: input_dim must equal the model's data_dim, one input channel")
            if enc.latent_dim != m.z_dim or getattr(m, "c_dim", 0) != 0:
                raise UnsupportedModel("conv encoder: latent_dim must equal the model's z_dim (latent + coord); no c_dim")
            conv_ops(enc.feature_extractor.layers, enc.feature_extractor.activation)      # validates
        elif not isinstance(enc, (fcEncoderNet, jfcEncoderNet)):
            raise UnsupportedModel("the HIP SVI path needs encoder_z to be pyroved_amd.nets.fcEncoderNet / "
                                   "jfcEncoderNet / convEncoderNet (got %s)" % type(enc).__name__)
        self.K = int(getattr(m, "discrete_dim", 0)) if isinstance(enc, jfcEncoderNet) else 0
        if self.ext_enc and self.ext_dec:
            return                                   # both user modules: the library keeps the reparameterisation + KL
        if self.ext_enc and isinstance(dec, (sDecoderNet, fcDecoderNet)):
            if len(_linears(dec.fc_layers)) > _abi.PV_MAX_LAYERS:
                raise UnsupportedModel("more than %d hidden layers" % _abi.PV_MAX_LAYERS)
            name = m.sampler_d.name
            if name not in _abi.LIK or (name not in ("gaussian", "poisson_log") and not dec.sigmoid_out):
                raise UnsupportedModel("decoder sampler %r / sigmoid_d combination is not implemented" % name)
            if name == "poisson_log" and dec.sigmoid_out:
                raise UnsupportedModel("poisson_log likelihood needs sigmoid_d=False (the decoder's output is the log-rate)")
            if (m.coord > 0) != isinstance(dec, sDecoderNet):
                raise UnsupportedModel("invariant models need the spatial decoder, vanilla models fcDecoderNet")
            return
        if not self.ext_enc and not enc.softplus_out:
            raise UnsupportedModel("encoder without softplus_out is not supported")
        if not self.conv_enc and len(_linears(enc.fc_layers)) > _abi.PV_MAX_LAYERS:
            raise UnsupportedModel("more than %d hidden layers" % _abi.PV_MAX_LAYERS)
        if self.ext_dec:
            return
        if m.coord > 0 and not isinstance(dec, sDecoderNet):
            raise UnsupportedModel("invariant models need the spatial decoder")
        if m.coord == 0 and not isinstance(dec, fcDecoderNet):
            raise UnsupportedModel("vanilla models need fcDecoderNet")
        name = m.sampler_d.name
        if name in _abi.LIK_JOINT:
            # the joint likelihood over a position's channels: models.iVAE with its own fully connected networks alone (the
            # per-value tests of every other engine, `name not in _abi.LIK`, refuse it with their own messages)
            if type(self) is not IVAEEngine or self.K > 0 or self.conv_enc:
                raise UnsupportedModel("sampler_d=%r is implemented for models.iVAE with its own fully connected encoder and "
                                       "decoder only (not for %s)" % (name, type(m).__name__))
            if self.C < 2:
                raise UnsupportedModel("sampler_d=%r needs channels >= 2, the classes per position (got channels=%d)"
                                       % (name, self.C))
            if dec.sigmoid_out:
                raise UnsupportedModel("%s likelihood needs sigmoid_d=False (the decoder's outputs are the class logits)" % name)
        elif name not in _abi.LIK:
            raise UnsupportedModel("decoder sampler %r is not implemented in the HIP path yet" % name)
        if name in ("bernoulli", "continuous_bernoulli") and not dec.sigmoid_out:
            raise UnsupportedModel("%s likelihood needs sigmoid_d=True" % name)
        if name == "poisson_log" and dec.sigmoid_out:
            raise UnsupportedModel("poisson_log likelihood needs sigmoid_d=False (the decoder's output is the log-rate)")
        if len(_linears(dec.fc_layers)) > _abi.PV_MAX_LAYERS:
            raise UnsupportedModel("more than %d hidden layers" % _abi.PV_MAX_LAYERS)

    def _param_order(self):
        """(key, tensor) in flat-buffer order: state_dict order, except that the heads are merged:
        fc11.weight, fc12.weight[, fc13.weight], then fc11.bias, fc12.bias[, fc13.bias]."""
        named = dict(self.model.named_parameters())
        if self.ext_enc:                         # only the decoder lives in the flat buffers (nothing if it is a user's too)
            return [(k, v) for k, v in named.items()
                    if not k.startswith("encoder_z.") and not (self.ext_dec and k.startswith("decoder."))]
        if self.ext_dec:                         # only the encoder does
            named = {k: v for k, v in named.items() if not k.startswith("decoder.")}
        if self.ext_y:                           # a user-defined label network (semi-supervised models) stays in torch
            named = {k: v for k, v in named.items() if not k.startswith("encoder_y.")}
        if self.conv_enc:
            return list(named.items())           # features2latent.fc_latent already is the merged [mu | sigma] head
        heads = ["fc11", "fc12"] + (["fc13"] if self.K > 0 else [])
        merged = ["encoder_z.%s.weight" % h for h in heads] + ["encoder_z.%s.bias" % h for h in heads]
        order = []
        for k in named:
            if k == merged[0]:
                order.extend(merged)
            elif k not in merged:
                order.append(k)
        return [(k, named[k]) for k in order]

    def _stat_buffers(self):
        """(key, tensor) of the batch-norm running statistics: they live in the flat buffer next to the parameters (the
        kernels update them in place; they never get a gradient, so Adam leaves them alone)."""
        return [(k, b) for k, b in self.model.named_buffers()
                if k.endswith(".running_mean") or k.endswith(".running_var")]

    def bind(self):
        """(Re)builds the flat buffers from the model's current parameters and re-points the
        parameters at them.  Called at construction and whenever the parameters were moved."""
        self._conv_slices = None                # (re-derived, and the weight-range check runs at the next call)
        self.wide_weights = False               # this model's kernel-3 weights fit the fp16-piece kernels until a check says otherwise
        items = self._param_order()
        n_par = len(items)
        items = items + self._stat_buffers()
        dev = items[0][1].device if items else next(self.model.parameters()).device
        if dev.type != "cuda":
            raise _abi.PvError(
                "pyroved_amd: the model lives on %s; the SVI path runs only on a HIP device "
                "(no CPU fallback). Construct the model with device='cuda'." % dev)
        _abi.lib()
        off = 0
        layout = {}
        for k, p in items:
            # tensors that the kernels address as one matrix must be packed back to back
            packed = k in ("encoder_z.fc12.weight", "encoder_z.fc12.bias", "encoder_z.fc13.weight", "encoder_z.fc13.bias")
            if not packed:
                off = (off + ALIGN - 1) // ALIGN * ALIGN
            layout[k] = off
            off += p.numel()
        total = max((off + ALIGN - 1) // ALIGN * ALIGN, ALIGN)      # (never empty: the ABI wants non-NULL buffers)
        old_m, old_v, old_layout = self.m, self.v, self._layout
        flat = torch.zeros(total, device=dev, dtype=torch.float32)
        for k, p in items:
            flat[layout[k]:layout[k] + p.numel()].copy_(p.detach().reshape(-1))
        self.flat = flat
        self.grad = torch.zeros(total + N_SCALARS, device=dev, dtype=torch.float32)
        self.m = torch.zeros(total, device=dev, dtype=torch.float32)
        self.v = torch.zeros(total, device=dev, dtype=torch.float32)
        if old_m is not None and old_layout == layout and old_m.numel() == total:
            self.m.copy_(old_m)
            self.v.copy_(old_v)
        self._views = {}
        for j, (k, p) in enumerate(items):
            view = flat[layout[k]:layout[k] + p.numel()].view(p.shape)
            if j < n_par:
                p.data = view
            else:                                    # a registered buffer: re-point the module's entry
                owner, _, leaf = k.rpartition(".")
                self.model.get_submodule(owner)._buffers[leaf] = view
            self._views[k] = view
        self._layout = layout
        self.n_flat = total
        self.device = dev
        self.scalars = self.grad[total:total + N_SCALARS]
        self.grid = self.model.grid.to(dev).contiguous() if self.model.coord > 0 else None
        if self.pixel_weights is not None:
            self.pixel_weights = self.pixel_weights.to(dev).contiguous()
        self.ws = None
        if self._torch_side:
            # the user module's parameters: their own torch Adam (zero_grads semantics)
            owners = ([self.model.encoder_z] if self.ext_enc else []) + ([self.model.decoder] if self.ext_dec else [])
            if not owners:
                owners = [self.model.encoder_y]
            self._enc_params = [q for o_ in owners for q in o_.parameters() if q.requires_grad]
            if self._enc_opt is None or [id(q) for q in self._enc_opt.param_groups[0]["params"]] != [id(q) for q in self._enc_params]:
                self._enc_opt = torch.optim.Adam(self._enc_params, lr=self.lr, betas=self.betas, eps=self.adam_eps)
        self._static = self._static_plan()

    def _pixel_weight_tensor(self, w):
        """pixel_weights as the library takes them: None / False -> None; a tensor, ndarray or bool mask of shape data_dim (the same
        weight in every channel) or (*data_dim, C) -> a contiguous float32 tensor of n_pix values, channel-last.  ValueError for
        another shape, negative or non-finite entries, or weights that are all zero."""
        if w is None or w is False:
            return None
        try:
            t = torch.as_tensor(w).detach()
        except Exception as e:
            raise ValueError("pixel_weights must be a tensor, an ndarray or a bool mask (got %s)" % type(w).__name__) from e
        dd = tuple(int(d) for d in self.model.data_dim)
        Cn = self.C
        if t.dtype == torch.bool:
            t = t.to(torch.float32)
        if not (t.is_floating_point() or t.dtype in (torch.uint8, torch.int8, torch.int16, torch.int32, torch.int64)):
            raise ValueError("pixel_weights must be real-valued or a bool mask (got dtype %s)" % t.dtype)
        t = t.to(torch.float32)
        if tuple(t.shape) == dd and Cn > 1:
            t = t.unsqueeze(-1).expand(*dd, Cn)
        elif tuple(t.shape) not in (dd + (Cn,), dd if Cn == 1 else None):
            want = "%s" % (dd,) if Cn == 1 else "%s (one weight per position, every channel) or %s" % (dd, dd + (Cn,))
            raise ValueError("pixel_weights must have shape %s (got %s)" % (want, tuple(t.shape)))
        t = t.reshape(-1).contiguous()
        if not bool(torch.isfinite(t).all()):
            raise ValueError("pixel_weights must be finite (found nan or inf)")
        if bool((t < 0).any()):
            raise ValueError("pixel_weights must be >= 0 (found %g)" % float(t.min()))
        if not bool((t > 0).any()):
            raise ValueError("pixel_weights are all zero: no observation would enter the loss")
        return t.to(self.device) if self.device is not None else t.clone()

    def _normalise(self, kw):
        """Settings as given -> as the engine keeps them; ValueError for a value that has no such form."""
        return {k: self._pixel_weight_tensor(v) if k == "pixel_weights" else _NORMALISE[k](v) for k, v in kw.items()}

    def _settings(self):
        return dict(fused=self.fused, kl=self.kl, particles=self.particles, renyi=self.renyi, fused_channels=self.fused_channels,
                    pixel_weights=self.pixel_weights, image_weights=self.image_weights, fast_weights=self.fast_weights,
                    fused_any_size=self.fused_any_size)

    def _validate(self, *, fused, kl, particles, renyi, fused_channels, pixel_weights, image_weights, fast_weights, dec_kernel,
                  fused_any_size=False):
        """The one rule list: which settings (normalised, _normalise) this model takes.  Raises the first rule the candidate breaks,
        in the order written; reads the model's facts (K, own_fc, fw_blocker) and no setting off self, and assigns nothing.  The
        constructor and configure() both validate here before they assign, so a refusal leaves no trace.
        On fast_weights: fused = 3 promises the bf16 kernel family, so a model the weighted bf16 decoder kernel does not take is
        refused; fused = 2 promises fp32-class results, which the weighted fused f32 / layer-by-layer kernels deliver as well, so
        such a model keeps that routing (_fast_weights_on)."""
        name = type(self.model).__name__
        multi = particles > 1 or renyi is not None
        what = "particles > 1" if renyi is None else "renyi"
        kw = " / ".join(k for k, on in (("pixel_weights", pixel_weights is not None), ("image_weights", image_weights)) if on)
        weighted = bool(kw)
        why = self.fw_blocker
        only_ivae = "%s is implemented for models.iVAE only (not for " + name + ")"

        def scope(on, what, discrete):
            """The scope rule of `what`: models.iVAE itself, no discrete latent, its own fully connected encoder and decoder."""
            return ((on and type(self) is not IVAEEngine, only_ivae % what),
                    (on and self.K > 0, discrete),
                    (on and not self.own_fc, "%s needs the model's own fully connected encoder and decoder (no convolutional or "
                                             "user-defined networks)" % what))
        rules = (
            (kl == "analytic" and self.K > 0,
             "kl='analytic' (TraceMeanField_ELBO) is not defined for models with a discrete latent (jiVAE): "
             "their objective enumerates or samples the class (TraceEnum_ELBO / Trace_ELBO)"),
            *scope(multi, what, "%s is not defined here for models with a discrete latent (jiVAE): their objective "
                                "enumerates or samples the class" % what),
            (multi and fused == 1, "%s runs on fused = 0, 2 or 3 (not on the f32-MFMA fused kernel, fused = 1)" % what),
            (renyi is not None and kl == "analytic",
             "renyi needs kl='sampled': the closed-form KL has no per-sample term for the bound to weigh"),
            (fused_channels and type(self) is not IVAEEngine, only_ivae % "fused_channels"),
            (fused_channels and multi,
             "fused_channels=True runs the one-particle ELBO only (not num_particles > 1 or the Renyi bound: "
             "the f32 fused kernel it selects has no multi-particle form)"),
            (fused_channels and fused == 3,
             "fused_channels=True selects the f32 fused decoder kernel; fused=3 (precision='bf16') asks for the "
             "bf16 throughput kernels, which have no multi-channel form"),
            (fused_channels and fused == 0,
             "fused_channels=True contradicts fused=0 (the layer-by-layer kernels): use fused=1 or 2"),
            (fused_any_size and type(self) is not IVAEEngine, only_ivae % "fused_any_size"),
            (fused_any_size and multi,
             "fused_any_size=True runs the one-particle ELBO only (not num_particles > 1 or the Renyi bound: "
             "the f32 fused kernel it selects has no multi-particle form)"),
            (fused_any_size and fused == 3,
             "fused_any_size=True selects the f32 fused decoder kernel; fused=3 (precision='bf16') asks for the "
             "bf16 throughput kernels, which have no form for positions that are no multiple of 16"),
            (fused_any_size and fused == 0,
             "fused_any_size=True contradicts fused=0 (the layer-by-layer kernels): use fused=1 or 2"),
            *scope(weighted, kw, only_ivae % kw),
            (weighted and multi, "%s runs the one-particle ELBO only (not num_particles > 1 or the Renyi bound)" % kw),
            (weighted and fused == 3 and not fast_weights,
             "%s is not implemented for fused=3 (precision='bf16'): the bf16 throughput kernels have "
             "no weighted form, and training at another precision than the one asked for is worse than refusing" % kw),
            (fast_weights and not weighted,
             "fast_weights=True selects the kernel of a WEIGHTED step: it needs pixel_weights and / or image_weights"),
            (fast_weights and fused in (0, 1),
             "fast_weights=True contradicts fused=%d (%s): it selects the bf16-class fused decoder kernels, use "
             "fused=2 or fused=3 (precision='bf16')"
             % (fused, "the layer-by-layer kernels" if fused == 0 else "the f32 fused kernel")),
            (fast_weights and fused == 3 and why is not None,
             "fast_weights=True with fused=3 (precision='bf16') needs a model the weighted bf16 decoder kernel "
             "takes, and %s" % why),
            (fast_weights and dec_kernel not in (0, 1) and why is None,
             "fast_weights=True runs the 4-wave bf16 decoder kernel (dec_kernel 0 or 1), not dec_kernel=%d" % dec_kernel),
        )
        for broken, message in rules:
            if broken:
                raise ValueError(message)

    @property
    def supports_dp_step(self) -> bool:
        """loss_and_grads(step=True, comm=NativeComm), the data-parallel step as one library call: the one-particle,
        single-channel, unweighted ELBO's."""
        return self.particles == 1 and self.renyi is None and self.C == 1 and not self._weighted() and not self._any_size_on()

    @property
    def _torch_side(self) -> bool:
        """Some module of this model runs in torch (a user-defined encoder_z, decoder or label network), with its own Adam."""
        return self.ext_enc or self.ext_dec or self.ext_y

    def _weighted(self) -> bool:
        """Whether the step runs the weighted entry points (pixel_weights, image_weights or both)."""
        return self.pixel_weights is not None or self.image_weights

    def _fast_weights_blocker(self) -> Optional[str]:
        """None where the weighted 4-wave bf16-class decoder kernel takes this model; otherwise the condition that fails.
        Asked once, by the constructor (self.fw_blocker): the model's structure is fixed for the engine's life."""
        m, dec = self.model, self.model.decoder
        if not self.own_fc:
            return "it is not models.iVAE with its own fully connected encoder and decoder"
        if self.C != 1:
            return "the model has %d channels (the kernel computes one)" % self.C
        if m.coord == 0 or not isinstance(dec, sDecoderNet):
            return "the decoder is the vanilla fully connected one (the kernel is the spatial decoder's)"
        lins = _linears(dec.fc_layers)
        if (len(lins) != 2 or any(l.in_features != 128 or l.out_features != 128 or l.bias is None for l in lins)
                or dec.activation != "tanh" or dec.coord_latent.fc_coord.out_features != 128):
            return ("the decoder is not two tanh layers of 128 (hidden_dim_d=[128, 128], activation='tanh'): it has %s, activation %r"
                    % ([l.out_features for l in lins], dec.activation))
        n_pos = math.prod(int(d) for d in m.data_dim)
        if n_pos % 16 != 0:
            return "the grid has %d positions, not a multiple of 16" % n_pos
        return None

    def _any_size_on(self) -> bool:
        """Whether fused_any_size takes effect (the plan then carries PV_PLAN_FUSED_TAIL and fused = 1): models.iVAE with its own
        fully connected networks and no discrete latent, the spatial decoder of two tanh layers of 128, a per-value likelihood, one
        channel or fused_channels, fused 1 or 2, and a number of grid positions that is NO multiple of 16.  Elsewhere the setting
        is a no-op: the model keeps the routing it has without it."""
        if not (self.fused_any_size and self.own_fc and self.K == 0 and self.fused in (1, 2)):
            return False
        m, dec = self.model, self.model.decoder
        if m.coord == 0 or not isinstance(dec, sDecoderNet) or m.sampler_d.name in _abi.LIK_JOINT:
            return False
        if (self.C > 1 and not self.fused_channels) or self.C == 7:      # (seven channels: the tail instance spills, none is built)
            return False
        lins = _linears(dec.fc_layers)
        if (len(lins) != 2 or any(l.in_features != 128 or l.out_features != 128 or l.bias is None for l in lins)
                or dec.activation != "tanh" or dec.coord_latent.fc_coord.out_features != 128):
            return False
        return math.prod(int(d) for d in m.data_dim) % 16 != 0

    def _fast_weights_on(self) -> bool:
        """Whether the weighted step runs the weighted bf16-class kernel (the plan then carries PV_PLAN_FAST_WEIGHTS and keeps `fused`)."""
        return self.fast_weights and self._weighted() and self.fused in (2, 3) and self.fw_blocker is None

    def _image_weight_tensor(self, w, b: int, n_pix: int):
        """image_weights of one call as the library takes them: a float / bool / integer tensor or ndarray of shape (b, *data_dim)
        (the same weight in every channel), (b, *data_dim, C) or (b, n_pix) -> one contiguous float32 device tensor (b, n_pix),
        channel-last.  Shape and dtype only: nothing here waits for the device."""
        try:
            t = torch.as_tensor(w).detach()
        except Exception as e:
            raise ValueError("image_weights must be a tensor, an ndarray or a bool mask (got %s)" % type(w).__name__) from e
        if not (t.is_floating_point() or t.dtype in (torch.bool, torch.uint8, torch.int8, torch.int16, torch.int32, torch.int64)):
            raise ValueError("image_weights must be real-valued or a bool mask (got dtype %s)" % t.dtype)
        dd = tuple(int(d) for d in self.model.data_dim)
        Cn = int(self.C)
        shape = tuple(t.shape)
        if shape == (b,) + dd and Cn > 1:
            t = t.to(self.device, torch.float32).unsqueeze(-1).expand(b, *dd, Cn)
        elif shape in ((b,) + dd + (Cn,), (b, n_pix)) or (Cn == 1 and shape == (b,) + dd):
            t = t.to(self.device, torch.float32)
        else:
            want = "(%d, %s)" % (b, ", ".join(str(d) for d in dd))
            if Cn > 1:
                want += " (one weight per position, every channel), (%d, %s, %d)" % (b, ", ".join(str(d) for d in dd), Cn)
            raise ValueError("image_weights must have shape %s or (%d, %d): one weight per observed value of every image of the "
                             "batch (got %s)" % (want, b, n_pix, shape))
        return t.reshape(b, n_pix).contiguous()

    def _plan_fused(self) -> int:
        """pv_ivae_plan.fused: the engine's `fused`, or 1 where fused_channels routes a multi-channel model to the f32 kernel —
        and where pixel_weights / image_weights route a one-channel model there (fused = 1 or 2: the weighted fused f32 kernel) unless
        fast_weights keeps it on the bf16-class kernels."""
        if self.fused_channels and self.C > 1 and self.fused in (1, 2):
            return 1
        if self._any_size_on():
            return 1
        if self._fast_weights_on():
            return int(self.fused)
        if self._weighted() and self.C == 1 and self.fused in (1, 2):
            return 1
        return int(self.fused)

    def configure(self, lr=None, betas=None, eps=None, fused=None, kl=None, particles=None, renyi=None, fused_channels=None,
                  pixel_weights=None, image_weights=None, fast_weights=None, fused_any_size=None):
        """Applies trainer-level settings to an engine that already exists (model.engine(**kw) on a model whose engine
        was created earlier — by encode(), manifold2d(), a previous trainer — must not silently drop them).
        renyi: a float alpha selects the importance-weighted bound, False returns to the ELBO, None leaves the setting.
        pixel_weights: weights set them, False removes them, None leaves the setting.
        image_weights: True turns the per-image weighted step on, False off, None leaves the setting.
        fast_weights: True / False switches the weighted step to / from the bf16-class decoder kernels, None leaves the setting.
        fused_any_size: True / False switches a model whose positions are no multiple of 16 to / from the fused f32 kernel's tail form."""
        given = dict(image_weights=image_weights, fast_weights=fast_weights, fused_channels=fused_channels, kl=kl,
                     particles=particles, renyi=renyi, fused=fused, pixel_weights=pixel_weights, fused_any_size=fused_any_size)
        new = self._normalise({k: v for k, v in given.items() if v is not None})
        adam = dict(lr=None if lr is None else float(lr), betas=None if betas is None else (float(betas[0]), float(betas[1])),
                    adam_eps=None if eps is None else float(eps))
        old = self._settings()
        self._validate(dec_kernel=self.dec_kernel, **{**old, **new})
        # accepted: nothing was assigned before this line.  The workspace's layout depends on the kernels the settings select
        if (any(k in new and new[k] != old[k] for k in ("fast_weights", "image_weights", "fused", "fused_channels", "fused_any_size"))
                or ("pixel_weights" in new and (new["pixel_weights"] is not None or old["pixel_weights"] is not None))):
            self.ws = None                                  # (pixel_weights=False on an unweighted engine: nothing to reset)
        vars(self).update(new)
        vars(self).update({k: v for k, v in adam.items() if v is not None})
        if self.flat is not None:
            self._static = self._static_plan()
        return self

    def reset_optimizer(self):
        """A fresh optimizer, as every trainer constructor of the reference makes one (trainers/svi.py:75-81:
        pyro.clear_param_store() + a new optim.Adam): zero moments, step count 0, no live gradients."""
        self.adam_t = 0
        self.grads_live = False
        if self.m is not None:
            self.m.zero_()
            self.v.zero_()
            self.grad.zero_()
        if self._enc_opt is not None:
            self._enc_opt = torch.optim.Adam(self._enc_params, lr=self.lr, betas=self.betas, eps=self.adam_eps)
            for q in self._enc_params:
                q.grad = None

    def _bound_snapshot(self):
        """What _bound's fast path compares against: the module tree (every submodule by identity, the number of parameters
        and buffers each one holds) and, per bound tensor, its owner's dict, leaf name, address and shape."""
        mods = [(mod, len(mod._parameters), len(mod._buffers), tuple(mod._modules.items())) for mod in self.model.modules()]
        tens = []
        for k, v in self._views.items():
            owner, _, leaf = k.rpartition(".")
            mod = self.model.get_submodule(owner) if owner else self.model
            tens.append((mod._parameters if leaf in mod._parameters else mod._buffers, leaf, v.data_ptr(), v.shape))
        return mods, tens

    def _bound(self) -> bool:
        """Do the model's parameters (and batch-norm statistics) still live in the flat buffer?  Asked at every call: the
        fast path walks the snapshot taken at the last full check (a few microseconds; nn.Module.named_parameters() of a
        small model costs ~40 — a third of a 0.1 ms step's host time); anything that differs from it — a tensor moved,
        replaced, added or removed, a submodule swapped — falls through to the full comparison."""
        snap = self._snap
        if snap is not None and snap[2] is self._views:
            ok = True
            for mod, npar, nbuf, kids in snap[0]:
                md = mod._modules
                if len(mod._parameters) != npar or len(mod._buffers) != nbuf or len(md) != len(kids):
                    ok = False
                    break
                for name, child in kids:
                    if md.get(name) is not child:
                        ok = False
                        break
                if not ok:
                    break
            if ok:
                for d, leaf, ptr, shape in snap[1]:
                    t = d.get(leaf)
                    if t is None or t.data_ptr() != ptr or t.shape != shape:
                        ok = False
                        break
            if ok:
                return True
        self._snap = None
        if self._views is None or not self._bound_full():
            return False
        self._snap = self._bound_snapshot() + (self._views,)
        return True

    def _bound_full(self) -> bool:
        named = dict(self.model.named_parameters())
        if self.ext_enc:
            named = {k: v for k, v in named.items() if not k.startswith("encoder_z.")}
        if self.ext_dec:
            named = {k: v for k, v in named.items() if not k.startswith("decoder.")}
        if self.ext_y:
            named = {k: v for k, v in named.items() if not k.startswith("encoder_y.")}
        named.update(dict(self._stat_buffers()))
        if len(named) != len(self._views):
            return False
        for k, v in self._views.items():
            p = named.get(k)
            if p is None or p.data_ptr() != v.data_ptr() or p.shape != v.shape:
                return False
        return True

    # ---- numeric range of the fp16-piece convolution kernels (include/pyroved_amd.h: pv_ivae_plan.conv_wide) ----
    _CONV_W_HI, _CONV_W_LO, _CONV_W_EVERY = 500.0, 2.0 ** -16, 64

    def _conv3_weight_slices(self):
        """(offset, numel) in the flat buffer of every kernel-3 convolution weight the model's conv stacks hold."""
        out = []
        for key, par in self._views.items():
            if key.endswith(".weight") and par.dim() >= 3 and par.shape[-1] == 3:
                out.append((self._layout[key], par.numel()))
        return out

    def _check_conv_weight_range(self, force: bool = False):
        """At the first call after a bind (training step, encode or decode alike) and every _CONV_W_EVERY-th call: if a
        kernel-3 convolution weight of THIS model left the range the fp16-piece kernels are exact in, its plans ask for the
        unbounded three-piece bf16 kernels from then on (plan field, ABI v14; other models in the process are unaffected).
        One scalar read-back per 64 calls; Adam moves a weight by at most lr per step, so the margin to fp16's limit (1023)
        cannot be crossed between two checks.  The read-back synchronises: while the current stream is being captured the
        check is skipped (captured steps are never range-checked — check before capturing)."""
        if self._conv_slices is None:
            self._conv_slices = self._conv3_weight_slices()
            self._conv_tick = 0
        if not self._conv_slices or self.wide_weights:
            return
        self._conv_tick += 1
        if not force and self._conv_tick % self._CONV_W_EVERY != 1:
            return
        if torch.cuda.is_current_stream_capturing():
            self._conv_tick -= 1                # (the next uncaptured call checks)
            return
        mx = float(torch.stack([self.flat[o:o + n].abs().max() for o, n in self._conv_slices]).max())
        if mx >= self._CONV_W_HI or 0.0 < mx < self._CONV_W_LO or mx != mx:
            import warnings
            warnings.warn("pyroved_amd: a convolution weight reached |w| = %.3g, outside the range of the fp16-piece "
                          "kernels; this model switches to the range-free bf16-piece convolution kernels (three pieces at "
                          "fp32-class precision, the two-piece mixed form at the throughput precision)" % mx)
            self.wide_weights = True

    def _plan_flags(self) -> int:
        """pv_ivae_plan.flags / pv_ved_plan.flags from the engine's switches (ABI v14; process-wide setters before)."""
        return ((_abi.PV_PLAN_ENC_TWO_LAUNCH if self.enc_two_launch else 0) |
                (0 if self.side_stream else _abi.PV_PLAN_NO_SIDE_STREAM) |
                (_abi.PV_PLAN_ENC_NO_WAIT if self.enc_no_wait else 0) |
                (0 if self.dec1d else _abi.PV_PLAN_NO_DEC1D) |
                (0 if self.enc_fold else _abi.PV_PLAN_NO_ENC_FOLD) |
                (0 if self.enc_per_image else _abi.PV_PLAN_ENC_TILED) |
                (0 if self.full_tile_loop else _abi.PV_PLAN_GENERIC_TILE_LOOP) |
                (_abi.PV_PLAN_FUSED_CHANNELS if (self.fused_channels and self.C > 1) else 0) |
                (_abi.PV_PLAN_FAST_WEIGHTS if self._fast_weights_on() else 0) |
                (_abi.PV_PLAN_FUSED_TAIL if self._any_size_on() else 0) |
                (_abi.PV_PLAN_CONV_X3 if self.conv_x3 else 0))

    def ensure_bound(self):
        if not self._bound():
            self.bind()

    # ------------------------------------------------------------------ plan
    def _layer(self, prefix: str, lin: nn.Linear, act) -> _abi.pv_layer:
        l = _abi.pv_layer()
        l.in_dim, l.out_dim, l.act = lin.in_features, lin.out_features, _abi.ACT[act]
        l.w_off = self._layout[prefix + ".weight"]
        l.b_off = self._layout[prefix + ".bias"] if lin.bias is not None else -1
        return l

    def _fc_encoder_plan(self, p, enc, m):
        idx = [i for i, mod in enumerate(enc.fc_layers) if isinstance(mod, nn.Linear)]
        p.n_enc = len(idx)
        for j, i in enumerate(idx):
            p.enc[j] = self._layer("encoder_z.fc_layers.%d" % i, enc.fc_layers[i], enc.activation)
        h = _abi.pv_layer()
        h.in_dim, h.out_dim, h.act = enc.fc11.in_features, 2 * m.z_dim + self.K, 0
        h.w_off, h.b_off = self._layout["encoder_z.fc11.weight"], self._layout["encoder_z.fc11.bias"]
        assert self._layout["encoder_z.fc12.weight"] == h.w_off + enc.fc11.weight.numel()
        assert self._layout["encoder_z.fc12.bias"] == h.b_off + enc.fc11.bias.numel()
        p.discrete_dim = self.K
        if self.K > 0:
            assert self._layout["encoder_z.fc13.weight"] == h.w_off + 2 * enc.fc11.weight.numel()
            assert self._layout["encoder_z.fc13.bias"] == h.b_off + 2 * enc.fc11.bias.numel()
        p.head = h

    def _static_plan(self) -> _abi.pv_ivae_plan:
        m = self.model
        enc, dec = m.encoder_z, m.decoder
        p = _abi.pv_ivae_plan()
        p.n_pix = 1
        for d in m.data_dim:
            p.n_pix *= int(d)
        p.n_pix *= self.C                              # observations per sample: positions * channels
        p.coord_dim = 0 if m.coord == 0 else (1 if m.ndim == 1 else 2)
        p.z_dim, p.c_dim = m.z_dim, m.c_dim
        p.latent_dim = m.z_dim - m.coord
        inv = m.invariances or []
        p.has_r, p.has_t, p.has_s = int('r' in inv), int('t' in inv), int('s' in inv)
        tp = getattr(m, "t_prior", None)
        if tp is not None:
            tpl = tp.detach().cpu().reshape(-1).tolist()
            p.t_prior[0] = tpl[0]
            p.t_prior[1] = tpl[1] if len(tpl) > 1 else tpl[0]
        sp = getattr(m, "sc_prior", None)
        p.sc_prior = float(sp) if sp is not None else 0.0
        p.lik = _abi.lik_code(m.sampler_d.name)
        p.sigmoid_out = int(getattr(dec, "sigmoid_out", True))
        p.decoder_sig = m.sampler_d.decoder_sig
        p.ext_decoder = int(self.ext_dec)
        p.fused = self._plan_fused()
        if self.ext_enc:
            p.n_enc = 0
            p.discrete_dim = 0
            p.ext_encoder = 1
            p.head.in_dim, p.head.out_dim = 1, 2 * m.z_dim
        elif self.conv_enc:
            p.n_enc = 0
            p.enc_ndim = len(enc.input_dim)
            for i, d in enumerate(enc.input_dim):
                p.enc_in_dim[i] = d
            eops = conv_ops(enc.feature_extractor.layers, enc.feature_extractor.activation,
                            "encoder_z.feature_extractor.layers")
            p.n_enc_ops = fill_ops(p.enc_ops, eops, self._layout)
            self._bn_enc = bn_modules(eops)
            p.head = self._layer("encoder_z.features2latent.fc_latent", enc.features2latent.fc_latent, None)
            p.discrete_dim = 0
        else:
            self._fc_encoder_plan(p, enc, m)
        if not self.ext_dec:
            if p.coord_dim > 0:
                p.fc_coord = self._layer("decoder.coord_latent.fc_coord", dec.coord_latent.fc_coord, "tanh")
                p.fc_latent = self._layer("decoder.coord_latent.fc_latent", dec.coord_latent.fc_latent, None)
            idx = [i for i, mod in enumerate(dec.fc_layers) if isinstance(mod, nn.Linear)]
            p.n_dec = len(idx)
            for j, i in enumerate(idx):
                p.dec[j] = self._layer("decoder.fc_layers.%d" % i, dec.fc_layers[i], dec.activation)
            p.out = self._layer("decoder.out", dec.out, None)
            if p.lik == _abi.PV_LIK_CATEGORICAL and p.coord_dim == 0:
                p.out._pad = self.C                    # the vanilla decoder's outputs are grouped C at a time (enum pv_lik's comment)
        p.params = self.flat.data_ptr()
        p.grads = self.grad.data_ptr()
        p.adam_m = self.m.data_ptr()
        p.adam_v = self.v.data_ptr()
        p.n_params = self.n_flat
        p.grid = self.grid.data_ptr() if self.grid is not None else None
        p.scalars = self.scalars.data_ptr()
        p.lr, p.adam_beta1, p.adam_beta2, p.adam_eps = self.lr, self.betas[0], self.betas[1], self.adam_eps
        self._objective = self._objective_desc()       # (rebuilt wherever the static plan is: bind, configure)
        return p

    def _objective_desc(self) -> _abi.pv_ivae_objective:
        """The step's objective as the library takes it (pv_ivae_objective), from the engine's settings; the two device pointers
        (obs_w, weights_out) are written per call.  Per-image weights carry the shared ones as a factor, so they win the kind."""
        o = _abi.pv_ivae_objective()
        o.num_particles = self.particles
        o.bound, o.alpha = (_abi.PV_BOUND_ELBO, 0.0) if self.renyi is None else (_abi.PV_BOUND_RENYI, self.renyi)
        o.obs_w_kind = (_abi.PV_OBS_W_PER_IMAGE if self.image_weights else
                        _abi.PV_OBS_W_SHARED if self.pixel_weights is not None else _abi.PV_OBS_W_NONE)
        return o

    def _plan(self, batch: int, beta: float = 1.0, what: int = 1) -> _abi.pv_ivae_plan:
        """what: 1 = training step, 2 = encode, 3 = decode (PV_WS_*): the workspace grows to what that call needs."""
        p = self._static
        p.batch = batch
        if isinstance(beta, (list, tuple)) or (torch.is_tensor(beta) and beta.ndim > 0):
            b0, b1 = (float(v) for v in beta)            # jiVAE: [continuous, discrete] KL scale factors
        else:
            b0 = b1 = float(beta)
        p.beta, p.beta_disc = b0, b1
        p.bn_eval = int(not self.model.training)
        p.conv_wide = int(self.wide_weights)
        p.flags = self._plan_flags()
        p.dec_kernel = int(self.dec_kernel)                     # 0: the library picks the decoder-kernel build by size (ABI v15)
        p.kl_mode = _abi.KL[self.kl]                            # (ABI v17)
        p.x = p.y = p.eps = p.z_loc = p.z_scale = p.loc = p.alpha = p.ext_head = p.ext_dhead = None
        p.row_w = p.row_elbo = p.dy = None
        p.ext_z = p.ext_dz = p.ext_ll = None
        p.class_onehot = None
        p.ev_start, p.ev_stop = self.events
        ce = self.conv_events                            # (start, stop, ctypes double for the launch's FLOPs) or None
        p.conv_ev_start, p.conv_ev_stop, p.conv_ev_flops = (ce[0], ce[1], C.addressof(ce[2])) if ce else (None, None, None)
        if what == 1:                                    # the training step's layout for this engine's objective
            need = _abi.lib().pv_ivae_objective_workspace_bytes(C.byref(p), C.byref(self._objective))
        else:
            need = _abi.lib().pv_ivae_workspace_bytes_for(C.byref(p), what)
        if need < 0:
            raise _abi.PvError("pyroved_amd: unsupported plan (pv_ivae_workspace_bytes_for -> %d)" % need)
        if self.ws is None or self.ws.numel() < need:
            self.ws = torch.empty(int(need), device=self.device, dtype=torch.uint8)
        p.ws = self.ws.data_ptr()
        p.ws_bytes = self.ws.numel()
        return p

    def _sample_shape(self):
        """One observation as the model's interface has it: data_dim, channel-last (*data_dim, C) when C > 1."""
        dd = tuple(int(d) for d in self.model.data_dim)
        return dd if self.C == 1 else dd + (self.C,)

    def _check_x(self, x, p):
        """Multi-channel input: (B, *data_dim, C) or already flat (B, n_pix) — anything else (channel-first, say) has the
        right number of values in the wrong order, so it is refused, not reshaped."""
        if self.C > 1 and tuple(x.shape[1:]) not in (self._sample_shape(), (p.n_pix,)):
            raise ValueError("channels=%d: x must be channel-last, (batch, %s) (got %s)"
                             % (self.C, ", ".join(str(d) for d in self._sample_shape()), tuple(x.shape)))

    def _prep(self, t: Optional[torch.Tensor], what: str, shape=None) -> Optional[torch.Tensor]:
        if t is None:
            return None
        _abi.require_device(t, what)
        t = t.contiguous()
        if shape is not None and tuple(t.shape) != tuple(shape):
            t = t.reshape(shape)
        return t

    def _prep_y(self, y, b: int, p) -> Optional[torch.Tensor]:
        """The conditioning vectors (b, c_dim) of a class-conditioned model; None for every other model."""
        if p.c_dim <= 0:
            return None
        if y is None:
            raise ValueError("class-conditioned model (c_dim=%d) needs y" % p.c_dim)
        return self._prep(y, "y", (b, p.c_dim))

    def _ext_head(self, x, b: int, p, want_grads: bool):
        """A user-defined encoder in PyTorch on the same stream: its outputs are the step's (z_loc, z_scale).  They enter the
        library through plan.ext_head, and the gradients come back through plan.ext_dhead.  -> (z_loc, z_scale, head, dhead)"""
        with torch.set_grad_enabled(want_grads):
            z_loc, z_scale = self.model.encoder_z(x)
        head = torch.cat([z_loc, z_scale], -1).detach().to(torch.float32).contiguous()
        if tuple(head.shape) != (b, 2 * p.z_dim):
            raise ValueError("encoder_z must return (z_loc, z_scale) of shape (batch, %d) each" % p.z_dim)
        dhead = torch.empty_like(head)
        p.ext_head, p.ext_dhead = head.data_ptr(), dhead.data_ptr()
        return z_loc, z_scale, head, dhead

    # ------------------------------------------------------------------ calls
    @_abi.on_device
    def loss_and_grads(self, x, eps, beta: float = 1.0, y=None, want_grads: bool = True,
                       scalars_out: Optional[torch.Tensor] = None, z_out=None, loc_out=None,
                       row_w: Optional[torch.Tensor] = None, row_elbo: Optional[torch.Tensor] = None,
                       dy: Optional[torch.Tensor] = None, step: bool = False,
                       class_onehot: Optional[torch.Tensor] = None, comm=None, hist_out: Optional[torch.Tensor] = None,
                       weights_out: Optional[torch.Tensor] = None, image_weights=None):
        """Enqueues Trace_ELBO.loss_and_grads (self.kl == "analytic": TraceMeanField_ELBO's) on the current stream.  Results land in
        self.scalars (device, 4 floats) and self.grad[:n_flat]; nothing is synchronised.
        The engine's objective goes to the library as one descriptor (self._objective: pv_ivae_objective_loss_and_grads /
        pv_ivae_objective_step); the entry points named below are the ones that descriptor stands for.
        row_w (B): per-sample weights of the ELBO terms; row_elbo (B) / dy (B, c_dim): extra outputs
        (include/pyroved_amd.h: pv_ivae_plan.row_w / row_elbo / dy).
        step=True: the whole SVI.step — the Adam update follows in the same library call (pv_ivae_step; on the fused
        decoder path it rides in the last gradient launch), identical in effect to loss_and_grads() + adam_step().
        class_onehot (B, discrete_dim): jiVAE WITHOUT enumeration — the class the guide drew for every sample
        (pv_ivae_plan.class_onehot; the trainer's default enumerate_parallel=False).
        step=True with comm (a dist.NativeComm): the DATA-PARALLEL step as one library call on this stream (pv_ivae_dp_step):
        this rank's shard's loss and gradients -> ncclAllReduce(SUM) of [gradients | loss scalars] -> Adam, with the reduced
        scalars written to hist_out (4 floats) in the optimizer's launch.
        particles = P > 1 (model.engine(particles=P)): eps is (P*B, z_dim) with rows ordered [p][b], loc_out (P*B, n_pix) in the
        same order, z_out stays (B, z_dim); the encoder runs once, the scalars hold means over particles
        (pv_ivae_particles_loss_and_grads / pv_ivae_particles_step).  Not with comm=, row_w / row_elbo / dy.
        renyi = alpha (model.engine(particles=P, renyi=alpha)): the importance-weighted bound over the same P samples
        (pv_ivae_renyi_loss_and_grads / pv_ivae_renyi_step): scalars[0] = -sum_b L_b, scalars[2] / [3] the weighted KL terms,
        scalars[1] the weighted log-likelihood plus the weights' entropy term; weights_out (P*B,), a device tensor, receives
        the normalised weights, rows [p][b].  Same restrictions as particles > 1.
        image_weights (an engine made with image_weights=True, and only there): this batch's weights, one per observed value of every
        image — (b, *data_dim), (b, *data_dim, C) or (b, n_pix); float, integer or bool; tensor or ndarray
        (pv_ivae_weighted_images_loss_and_grads / _step).  With pixel_weights as well the library gets the product.  Not with comm=,
        row_w / row_elbo / dy / class_onehot."""
        self.ensure_bound()
        P = self.particles
        alpha = self.renyi
        pw = self.pixel_weights
        extras = comm is not None or row_w is not None or row_elbo is not None or dy is not None or class_onehot is not None
        # (weights that do not match the engine's image_weights setting are refused for that, below)
        weighted = (pw is not None or image_weights is not None) and self.image_weights == (image_weights is not None)
        if extras and (P > 1 or alpha is not None or weighted):
            raise ValueError("%s cannot be combined with comm=, row_w, row_elbo, dy or class_onehot"
                             % ("particles > 1 / renyi" if (P > 1 or alpha is not None) else
                                "pixel_weights" if not self.image_weights else "image_weights"))
        if self.image_weights != (image_weights is not None):
            if image_weights is None:
                raise ValueError("this engine was made with image_weights=True: every call needs image_weights=w, the batch's weights")
            raise ValueError("image_weights= needs an engine configured for it: model.engine(image_weights=True)")
        iw = None
        if image_weights is not None:                     # (shape and dtype, before anything is planned or enqueued)
            iw = self._image_weight_tensor(image_weights, int(x.shape[0]), math.prod(int(d) for d in self.model.data_dim) * int(self.C))
            if pw is not None:
                iw = iw * pw                              # (b, n_pix) * (n_pix): one multiply on the device, then the per-image call
        if weights_out is not None and alpha is None:
            raise ValueError("weights_out belongs to the importance-weighted bound: model.engine(particles=P, renyi=alpha)")
        if self.conv_enc:
            self._check_conv_weight_range()
        if step and (self._torch_side or not want_grads):
            raise ValueError("step=True needs every parameter in the library (no user-defined modules) and want_grads")
        if comm is not None and (not step or scalars_out is not None):
            raise ValueError("comm= goes with step=True and the engine's own scalars (no scalars_out)")
        if self.ext_dec:
            return self._loss_and_grads_ext_decoder(x, eps, beta, y, want_grads, scalars_out, z_out, loc_out)
        b = x.shape[0]
        p = self._plan(b, beta)
        self._check_x(x, p)
        head = dhead = None
        if self.ext_enc:
            z_loc, z_scale, head, dhead = self._ext_head(x, b, p, want_grads)
        x = self._prep(x, "x", (b, p.n_pix))
        if P > 1 and eps.numel() != P * b * p.z_dim:
            raise ValueError("particles=%d: eps must be (%d, %d) = (particles * batch, z_dim), rows ordered [p][b] (got %s)"
                             % (P, P * b, p.z_dim, tuple(eps.shape)))
        eps = self._prep(eps, "eps", (P * b, p.z_dim))
        y = self._prep_y(y, b, p)
        if P > 1 and loc_out is not None and loc_out.numel() != P * b * p.n_pix:
            raise ValueError("particles=%d: loc_out must hold (%d, %d) values" % (P, P * b, p.n_pix))
        if weights_out is not None:
            _abi.require_device(weights_out, "weights_out")
            if not weights_out.is_contiguous() or weights_out.dtype != torch.float32 or weights_out.numel() != P * b:
                raise ValueError("weights_out must be a contiguous float32 tensor of %d = particles * batch values" % (P * b))
        p.x, p.eps = x.data_ptr(), eps.data_ptr()
        p.y = y.data_ptr() if y is not None else None
        if z_out is not None:
            p.z_loc, p.z_scale = z_out[0].data_ptr(), z_out[1].data_ptr()
        if loc_out is not None:
            p.loc = loc_out.data_ptr()
        if scalars_out is not None:
            p.scalars = scalars_out.data_ptr()
        row_w = self._prep(row_w, "row_w", (b,))
        for t_, name_, shape_ in ((row_elbo, "row_elbo", (b,)), (dy, "dy", (b, p.c_dim))):
            if t_ is not None:
                _abi.require_device(t_, name_)
                if not t_.is_contiguous() or tuple(t_.shape) != shape_:
                    raise ValueError("%s must be a contiguous float32 tensor of shape %s" % (name_, shape_))
        p.row_w = row_w.data_ptr() if row_w is not None else None
        p.row_elbo = row_elbo.data_ptr() if row_elbo is not None else None
        p.dy = dy.data_ptr() if dy is not None else None
        class_onehot = self._prep(class_onehot, "class_onehot", (b, self.K)) if class_onehot is not None else None
        if class_onehot is not None and self.K <= 0:
            raise ValueError("class_onehot needs a model with a discrete latent (models.jiVAE)")
        p.class_onehot = class_onehot.data_ptr() if class_onehot is not None else None
        obj = self._objective
        obj.obs_w = (iw if iw is not None else pw).data_ptr() if (iw is not None or pw is not None) else None
        obj.weights_out = weights_out.data_ptr() if weights_out is not None else None
        try:
            if step:
                p.lr, p.adam_beta1, p.adam_beta2, p.adam_eps = self.lr, self.betas[0], self.betas[1], self.adam_eps
                p.adam_step = self.adam_t + 1
                if comm is not None:
                    if hist_out is not None:
                        _abi.require_device(hist_out, "hist_out")
                    _abi.check(_abi.lib().pv_ivae_dp_step(C.byref(p), comm.handle, _abi.ptr(hist_out), _abi.current_stream()),
                               "pv_ivae_dp_step")
                else:
                    _abi.check(_abi.lib().pv_ivae_objective_step(C.byref(p), C.byref(obj), _abi.current_stream()),
                               "pv_ivae_objective_step")
                self.adam_t += 1
            else:
                _abi.check(_abi.lib().pv_ivae_objective_loss_and_grads(C.byref(p), C.byref(obj), int(want_grads),
                                                                       _abi.current_stream()), "pv_ivae_objective_loss_and_grads")
        finally:
            p.scalars = self.scalars.data_ptr()
            p.ext_head = p.ext_dhead = None
            p.row_w = p.row_elbo = p.dy = None
            p.class_onehot = None
        if self.ext_enc and want_grads:
            zd = p.z_dim
            for q in self._enc_params:
                q.grad = None
            torch.autograd.backward([z_loc, z_scale], [dhead[:, :zd], dhead[:, zd:]])
        if want_grads:
            self.grads_live = True
        self._count_bn(self._bn_enc)
        self._keep = (x, eps, y, head, dhead, row_w, class_onehot, iw)   # keep inputs alive until the stream has consumed them

    # ------------------------------------------------------------------ user-defined decoder (torch) around the HIP guide
    def _torch_decode(self, z, y=None, angle=None, shift=None, scale=None):
        """iVAE.model's decoder half in PyTorch (models/ivae.py:184-198): split, scale by the priors, transform the grid,
        decode.  Differentiable w.r.t. z and the decoder's parameters.  angle / shift / scale: the fixed transform of
        baseVAE._decode (models/base.py:153-170) instead of the one read off z (z is then the content part)."""
        m = self.model
        b = z.shape[0]
        if m.coord == 0:
            return m.decoder(z if y is None else torch.cat([z, y], -1))
        grid = m.grid.to(z.device).expand(b, *m.grid.shape)
        if angle is None:
            phi, dx, sc, zc = m._split_latent(z)
            if 't' in m.invariances:
                dx = (dx * m.t_prior.to(z.device)).unsqueeze(1)
        else:
            phi = torch.full((b,), float(angle), device=z.device)
            dx = torch.tensor([float(shift[0]), float(shift[1])][:m.ndim], device=z.device).expand(b, 1, m.ndim)
            sc = torch.full((b,), float(scale), device=z.device)
            zc = z
        if m.ndim == 1:
            xc = grid + dx
        else:
            phi = phi if phi.ndim else phi.expand(b)
            sc = sc if sc.ndim else sc.expand(b)
            rot = torch.stack([torch.stack([torch.cos(phi), torch.sin(phi)], 1),
                               torch.stack([-torch.sin(phi), torch.cos(phi)], 1)], 1)
            xc = torch.bmm(grid, rot) * sc.reshape(b, 1, 1) + dx                # utils/coord.py:47-88
        if y is not None:
            zc = torch.cat([zc, y], -1)
        return m.decoder(xc, zc)

    def _torch_loc(self, out):
        """The mean image from a user-defined decoder's output: the output itself, except for 'poisson_log' (the rate)."""
        return torch.exp(out.clamp(max=30)) if self.model.sampler_d.name == "poisson_log" else out

    def _torch_likelihood(self, loc):
        import torch.distributions as td
        s = self.model.sampler_d
        if s.name == "bernoulli":
            return td.Bernoulli(loc, validate_args=False)
        if s.name == "continuous_bernoulli":
            return td.ContinuousBernoulli(loc)
        if s.name == "poisson_log":
            return td.Poisson(torch.exp(loc.clamp(max=30)), validate_args=False)
        return td.Normal(loc, s.decoder_sig)

    def _loss_and_grads_ext_decoder(self, x, eps, beta, y, want_grads, scalars_out, z_out, loc_out):
        b = x.shape[0]
        p = self._plan(b, beta)
        x = self._prep(x, "x", (b, p.n_pix))
        eps = self._prep(eps, "eps", (b, p.z_dim))
        y = self._prep_y(y, b, p)
        z = torch.empty(b, p.z_dim, device=self.device, dtype=torch.float32)
        p.x, p.eps, p.y, p.ext_z = x.data_ptr(), eps.data_ptr(), (y.data_ptr() if y is not None else None), z.data_ptr()
        head = dhead = None
        if self.ext_enc:                             # a user-defined encoder as well (it sees x in the model's data_dim)
            z_loc, z_scale, head, dhead = self._ext_head(x.reshape(b, *self.model.data_dim), b, p, want_grads)
        if z_out is not None:
            p.z_loc, p.z_scale = z_out[0].data_ptr(), z_out[1].data_ptr()
        if scalars_out is not None:
            p.scalars = scalars_out.data_ptr()
        try:
            _abi.check(_abi.lib().pv_ivae_guide(C.byref(p), _abi.current_stream()), "pv_ivae_guide")
            zt = z.detach().requires_grad_(want_grads)
            with torch.set_grad_enabled(want_grads):
                loc = self._torch_decode(zt, y)
                ll = self._torch_likelihood(loc.reshape(b, -1)).log_prob(x).sum()
            if loc_out is not None:
                loc_out.copy_(self._torch_loc(loc.detach()).reshape(loc_out.shape))
            dz = None
            if want_grads:
                for q in self._enc_params:
                    q.grad = None
                (-ll).backward()
                dz = zt.grad.contiguous()
                p.ext_dz = dz.data_ptr()
            ll1 = ll.detach().reshape(1).to(torch.float32)
            p.ext_ll = ll1.data_ptr()
            _abi.check(_abi.lib().pv_ivae_guide_backward(C.byref(p), int(want_grads), _abi.current_stream()),
                       "pv_ivae_guide_backward")
            if self.ext_enc and want_grads:
                zd = p.z_dim
                torch.autograd.backward([z_loc, z_scale], [dhead[:, :zd], dhead[:, zd:]])
        finally:
            p.scalars = self.scalars.data_ptr()
            p.ext_z = p.ext_dz = p.ext_ll = None
            p.ext_head = p.ext_dhead = None
        if want_grads:
            self.grads_live = True
        self._count_bn(self._bn_enc)
        self._keep = (x, eps, y, z, dz, ll1, head, dhead)

    def _count_bn(self, mods):
        """nn.BatchNorm's num_batches_tracked (a forward in training mode counts; the statistics themselves are updated
        by the kernels)."""
        if self.model.training:
            for b_ in mods:
                b_.num_batches_tracked += 1

    @_abi.on_device
    def adam_step(self):
        """pyro.optim.Adam over every parameter + zero_grads (one fused kernel)."""
        self.adam_t += 1
        _abi.check(_abi.lib().pv_adam_step(
            _abi.ptr(self.flat), _abi.ptr(self.grad), _abi.ptr(self.m), _abi.ptr(self.v), self.n_flat,
            self.lr, self.betas[0], self.betas[1], self.adam_eps, self.adam_t, _abi.current_stream()),
            "pv_adam_step")
        if self._torch_side and any(q.grad is not None for q in self._enc_params):
            for g_ in self._enc_opt.param_groups:
                g_["lr"], g_["betas"], g_["eps"] = self.lr, self.betas, self.adam_eps
            self._enc_opt.step()
            for q in self._enc_params:               # pyro.infer.util.zero_grads: zero tensors, not None
                if q.grad is not None:
                    q.grad = torch.zeros_like(q.grad)

    @_abi.on_device
    def adam_step_hist(self, hist_slot: torch.Tensor):
        """adam_step() plus, in the same launch, the copy of the 4 (all-reduced) loss scalars into `hist_slot` — the
        data-parallel step after its one all-reduce (pv_adam_step_hist)."""
        if self._torch_side:
            hist_slot.copy_(self.scalars)
            return self.adam_step()
        self.adam_t += 1
        _abi.check(_abi.lib().pv_adam_step_hist(
            _abi.ptr(self.flat), _abi.ptr(self.grad), _abi.ptr(self.m), _abi.ptr(self.v), self.n_flat,
            self.lr, self.betas[0], self.betas[1], self.adam_eps, self.adam_t,
            _abi.ptr(self.scalars), _abi.ptr(hist_slot), N_SCALARS, _abi.current_stream()), "pv_adam_step_hist")

    def extra_grads(self):
        """Gradient tensors that live outside the flat buffer (a user-defined encoder's): reduced separately in
        data-parallel runs."""
        return [q.grad for q in self._enc_params if q.grad is not None] if self._torch_side else []

    @_abi.on_device
    def encode(self, x, y=None):
        self.ensure_bound()
        if self.ext_enc:
            with torch.no_grad():
                z_loc, z_scale = self.model.encoder_z(x)
            return z_loc.to(torch.float32), z_scale.to(torch.float32)
        if self.conv_enc:
            self._check_conv_weight_range()
        b = x.shape[0]
        p = self._plan(b, what=2)
        self._check_x(x, p)
        x = self._prep(x, "x", (b, p.n_pix))
        y = self._prep_y(y, b, p)
        p.x = x.data_ptr()
        p.y = y.data_ptr() if y is not None else None
        z_loc = torch.empty(b, p.z_dim, device=self.device, dtype=torch.float32)
        z_scale = torch.empty_like(z_loc)
        alpha = torch.empty(b, self.K, device=self.device, dtype=torch.float32) if self.K > 0 else None
        if alpha is not None:
            p.alpha = alpha.data_ptr()
        _abi.check(_abi.lib().pv_ivae_encode(C.byref(p), _abi.ptr(z_loc), _abi.ptr(z_scale), _abi.current_stream()),
                   "pv_ivae_encode")
        self._count_bn(self._bn_enc)
        self._keep = (x, y)
        if alpha is not None:
            return z_loc, z_scale, alpha
        return z_loc, z_scale

    # ------------------------------------------------------------------ held-out log-evidence
    def _check_evidence(self):
        """log_evidence's scope on the Python side: no observation weights (no kernel applies them to several particles)."""
        if self._weighted():
            raise ValueError("log_evidence: this engine is configured with %s, and no kernel applies observation weights to several "
                             "particles — evaluate on an engine without them"
                             % ("image_weights" if self.image_weights else "pixel_weights"))

    @_abi.on_device
    def log_evidence_chunk(self, x, eps, y=None, state: Optional[torch.Tensor] = None, first: bool = True):
        """Adds one chunk of P particles to the running log-evidence state of the batch x (pv_ivae_evidence_accumulate, beta = 1).
        eps: (P*B, z_dim) or (P, B, z_dim), rows ordered [p][b]; state: the device (B, 4) float32 tensor a previous chunk returned
        (None: a new one); first=True initialises it from this chunk.  Returns the state; log_evidence_finish reads it.
        An engine with fused=1 (fused_channels=True included) evaluates on the layer-by-layer plan, fused=0: both are fp32.
        The evidence workspace is cached per (batch, P) layout, the largest asked for so far."""
        self._check_evidence()
        self.ensure_bound()
        b = int(x.shape[0])
        p = self._plan(b, 1.0, what=2)
        self._check_x(x, p)
        if eps.numel() % (b * p.z_dim) != 0 or eps.numel() == 0:
            raise ValueError("log_evidence_chunk: eps must be (P * batch, z_dim) = (P * %d, %d), rows ordered [p][b] (got %s)"
                             % (b, p.z_dim, tuple(eps.shape)))
        P = eps.numel() // (b * p.z_dim)
        x = self._prep(x, "x", (b, p.n_pix))
        eps = self._prep(eps, "eps", (P * b, p.z_dim))
        y = self._prep_y(y, b, p)
        if state is None:
            if not first:
                raise ValueError("log_evidence_chunk: first=False continues a state, which it needs")
            state = torch.empty(b, 4, device=self.device, dtype=torch.float32)
        _abi.require_device(state, "state")
        if state.dtype != torch.float32 or not state.is_contiguous() or tuple(state.shape) != (b, 4):
            raise ValueError("log_evidence_chunk: state must be a contiguous float32 tensor of shape (%d, 4)" % b)
        fused, flags = p.fused, p.flags
        try:
            if p.fused == 1:
                p.fused = 0
            p.flags = flags & ~_abi.PV_PLAN_FUSED_CHANNELS
            if self._ev_need is None:
                self._ev_need = {}
            key = (b, P, int(p.fused))
            need = self._ev_need.get(key)
            if need is None:
                need = _abi.lib().pv_ivae_evidence_workspace_bytes(C.byref(p), P)
                if need < 0:
                    raise _abi.PvError("pyroved_amd: log-evidence unsupported for this plan or particle count %d "
                                       "(pv_ivae_evidence_workspace_bytes -> %d)" % (P, need))
                self._ev_need[key] = need
            if self._ev_ws is None or self._ev_ws.numel() < need:
                self._ev_ws = torch.empty(int(need), device=self.device, dtype=torch.uint8)
            p.ws, p.ws_bytes = self._ev_ws.data_ptr(), self._ev_ws.numel()
            p.x, p.eps = x.data_ptr(), eps.data_ptr()
            p.y = y.data_ptr() if y is not None else None
            _abi.check(_abi.lib().pv_ivae_evidence_accumulate(C.byref(p), P, _abi.ptr(state), int(bool(first)), _abi.current_stream()),
                       "pv_ivae_evidence_accumulate")
        finally:
            p.fused, p.flags = fused, flags
        self._keep = (x, eps, y, state)
        return state

    @_abi.on_device
    def log_evidence_finish(self, state, num_samples: int, want_ess: bool = False):
        """(log p^(x_b), ESS_b or None) on the device from a state that num_samples particles went into (pv_logmeanexp_finish)."""
        b = int(state.shape[0])
        out = torch.empty(b, device=self.device, dtype=torch.float32)
        ess = torch.empty_like(out) if want_ess else None
        _abi.check(_abi.lib().pv_logmeanexp_finish(_abi.ptr(state), b, int(num_samples), _abi.ptr(out), _abi.ptr(ess),
                                                   _abi.current_stream()), "pv_logmeanexp_finish")
        return out, ess

    @_abi.on_device
    def decode(self, z, angle: float = 0.0, shift=(0.0, 0.0), scale: float = 1.0):
        """z: (B, latent_dim + c_dim) content latents [+ class vector]."""
        self.ensure_bound()
        if self.ext_dec:
            with torch.no_grad():
                loc = self._torch_decode(z.to(self.device, torch.float32), None, angle, shift, scale)
            return self._torch_loc(loc).reshape(z.shape[0], *self.model.data_dim)
        b = z.shape[0]
        p = self._plan(b, what=3)
        lat_in = (p.latent_dim if p.coord_dim > 0 else p.z_dim) + p.c_dim + self.K
        z = self._prep(z, "z", (b, lat_in))
        loc = torch.empty(b, p.n_pix, device=self.device, dtype=torch.float32)
        _abi.check(_abi.lib().pv_ivae_decode(C.byref(p), _abi.ptr(z), float(angle), float(shift[0]), float(shift[1]),
                                             float(scale), _abi.ptr(loc), _abi.current_stream()), "pv_ivae_decode")
        self._keep = (z,)
        return loc.view(b, *self._sample_shape())

    @_abi.on_device
    def uses_fused(self, batch: int) -> bool:
        """Whether loss_and_grads runs the fused persistent decoder kernel for this batch size."""
        if self._weighted():
            return bool(_abi.lib().pv_ivae_weighted_uses_fused(C.byref(self._plan(batch))))
        return bool(_abi.lib().pv_ivae_uses_fused(C.byref(self._plan(batch))))

    # views for tests / data-parallel reduction
    def grad_of(self, key: str) -> torch.Tensor:
        n = self._views[key].numel()
        return self.grad[self._layout[key]:self._layout[key] + n].view(self._views[key].shape)
