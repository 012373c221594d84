"""
The engines' settings as a table: which combinations of model.engine(**kw) / engine.configure(**kw) are accepted, what the engine
then hands to the library, and the exact refusal otherwise.  tests/golden/make_engine_settings.py records the table
(tests/golden/engine_settings.json), tests/test_engine_settings_cpu.py replays it.  Nothing here reaches a device: bind() is stubbed.

Only the surface that every version of the engines has is used: model.engine / configure, _plan_fused, _plan_flags,
supports_dp_step, _objective_desc's num_particles / bound / alpha / obs_w_kind, the setting attributes and `ws`.
"""
import contextlib
import itertools
import json

import torch

import pyroved_amd as pv
from pyroved_amd.engine import IVAEEngine
from pyroved_amd.engine_ss import SSEngine
from pyroved_amd.engine_ved import VEDEngine

SENTINEL = "primed"


class UserEncoder(torch.nn.Module):
    """A user-defined encoder_z (set_encoder): it runs in torch, so the engine counts it as an external module."""

    def __init__(self, z_dim):
        super().__init__()
        self.z_dim = z_dim

    def forward(self, x):
        return x.reshape(x.shape[0], -1)[:, :self.z_dim], torch.ones(x.shape[0], self.z_dim)


def _ivae(dims=(8, 8), inv=("r", "t", "s"), **kw):
    return pv.models.iVAE(dims, 2, list(inv) if inv else None, seed=1, device="cpu", **kw)


def _user_encoder():
    m = _ivae()
    m.set_encoder(UserEncoder(m.z_dim))
    return m


# the constructor table's eight models, then the three of the smaller cross
MODELS = {
    "ivae_8x8_rts": _ivae,
    "ivae_c3": lambda: _ivae(channels=3),
    "ivae_noinv": lambda: _ivae(inv=None),
    "ivae_d72_40": lambda: _ivae(hidden_dim_d=[72, 40]),
    "ivae_7x9_rt": lambda: _ivae(dims=(7, 9), inv=("r", "t")),
    "jivae": lambda: pv.models.jiVAE((8, 8), 2, 3, ["r"], seed=1, device="cpu"),
    "ivae_c3_categorical": lambda: _ivae(channels=3, sampler_d="categorical", sigmoid_d=False),
    "ivae_user_encoder": _user_encoder,
}
SMALL_MODELS = {
    "ssivae": lambda: pv.models.ssiVAE((8, 8), 2, 3, ["r"], seed=1, device="cpu"),
    "ss_reg_ivae": lambda: pv.models.ss_reg_iVAE((8, 8), 2, 2, ["r"], seed=1, device="cpu"),
    "ved": lambda: pv.models.VED((8, 8), (8, 8), seed=1, device="cpu"),
}
CONFIGURE_MODELS = ("ivae_8x8_rts", "ivae_c3", "jivae")

# (keyword, values): "ones" stands for a tensor of ones of the model's data_dim
AXES = (("fused", (0, 1, 2, 3)), ("kl", ("sampled", "analytic")), ("particles", (1, 3)), ("renyi", (None, 0.0)),
        ("fused_channels", (False, True)), ("pixel_weights", (None, "ones")), ("image_weights", (False, True)),
        ("fast_weights", (False, True)))
SMALL_AXES = tuple((k, v) for k, v in AXES if k in ("kl", "particles", "pixel_weights", "image_weights", "fast_weights"))

# configure: every single-keyword change of the same value sets, the values that remove a setting, an optimizer setting, and
# the two changes that break the KL rule and the particle rule at once (the rules' order shows only there)
CHANGES = tuple({k: v} for k, vals in AXES for v in vals) + (
    {"pixel_weights": False}, {"renyi": False}, {"lr": 2e-3},
    {"kl": "analytic", "particles": 3}, {"kl": "analytic", "renyi": 0.0})
DEC_KERNELS = (0, 1, 28)          # engine.dec_kernel before the configure call (0: left alone)


def cases(axes=AXES):
    """Every combination of the axes' values as a keyword dict, in a fixed order."""
    return [dict(zip((k for k, _ in axes), vals)) for vals in itertools.product(*(v for _, v in axes))]


def key(kw):
    return tuple(sorted(kw.items(), key=lambda kv: kv[0]))


@contextlib.contextmanager
def unbound():
    """Engines that never reach the device: bind() does nothing."""
    saved = [(cls, cls.__dict__["bind"]) for cls in (IVAEEngine, SSEngine, VEDEngine) if "bind" in cls.__dict__]
    for cls, _ in saved:
        cls.bind = lambda self: None
    try:
        yield
    finally:
        for cls, fn in saved:
            cls.bind = fn


def _kw(model, kw):
    """The keyword dict as the engine gets it: "ones" becomes the tensor."""
    if kw.get("pixel_weights") == "ones":
        kw = dict(kw, pixel_weights=torch.ones(*(int(d) for d in model.data_dim)))
    return kw


def plan_of(eng):
    o = eng._objective_desc()
    return [int(eng._plan_fused()), int(eng._plan_flags()), bool(eng.supports_dp_step),
            int(o.num_particles), int(o.bound), float(o.alpha), int(o.obs_w_kind)]


def settings_of(eng):
    return [eng.fused, eng.kl, eng.particles, eng.renyi, eng.fused_channels, eng.pixel_weights is not None, eng.image_weights,
            eng.fast_weights, eng.dec_kernel]


def optimizer_of(eng):
    return [eng.lr, list(eng.betas), eng.adam_eps]


def construct(model, kw):
    """(engine or None, outcome): ["ok", plan] or [exception type, message]."""
    model._engine = None
    try:
        eng = model.engine(**_kw(model, kw))
    except Exception as e:          # (recorded, whatever it is: the replay compares type and text)
        return None, [type(e).__name__, str(e)]
    return eng, ["ok", plan_of(eng)]


def configure(model, start, dec_kernel, change):
    """From the accepted constructor state `start`: (engine, outcome), the outcome being
    ["ok" or exception type, message or None, settings, optimizer settings, plan, whether ws kept its sentinel] — the settings as
    "kept" (those before the call), "set" (those the call asked for) or, if neither, the list itself."""
    eng, first = construct(model, start)
    assert first[0] == "ok", (start, first)
    eng.ws = SENTINEL
    if dec_kernel:
        eng.dec_kernel = dec_kernel
    before = settings_of(eng)
    try:
        eng.configure(**_kw(model, change))
        how, msg = "ok", None
    except Exception as e:
        how, msg = type(e).__name__, str(e)
    after, want = settings_of(eng), target(start, change)
    asked = [want[k] for k, _ in AXES[:5]] + [want["pixel_weights"] is not None, want["image_weights"], want["fast_weights"], before[-1]]
    return eng, [how, msg, "kept" if after == before else "set" if after == asked else after, optimizer_of(eng), plan_of(eng),
                 eng.ws is SENTINEL]


def target(start, change):
    """The settings a configure(**change) from `start` asks for, as a constructor keyword dict (None leaves a setting)."""
    kw = dict(start)
    for k, v in change.items():
        if k in kw and v is not None:
            kw[k] = None if v is False and k in ("renyi", "pixel_weights") else v
    return kw


def record():
    """The whole table: {"constructor": {model: [outcome]}, "small": {model: [outcome]},
    "configure": {model: [[outcome per (dec_kernel, change)] per accepted constructor case, in the cases' order]}}."""
    out = {"constructor": {}, "small": {}, "configure": {}}
    with unbound():
        for name, make in MODELS.items():
            m = make()
            out["constructor"][name] = [construct(m, kw)[1] for kw in cases()]
        for name, make in SMALL_MODELS.items():
            m = make()
            out["small"][name] = [construct(m, kw)[1] for kw in cases(SMALL_AXES)]
        for name in CONFIGURE_MODELS:
            m = MODELS[name]()
            rows = []
            for kw, res in zip(cases(), out["constructor"][name]):
                if res[0] == "ok":
                    rows.append([configure(m, kw, dk, ch)[1] for dk in DEC_KERNELS for ch in CHANGES])
            out["configure"][name] = rows
    return out


def pack(table):
    """Distinct messages and distinct outcomes once each, the cases as indices."""
    messages, outcomes, seen = [], [], {}

    def idx(lst, v):
        k = (id(lst), json.dumps(v))            # (by text: 1, 1.0 and True stay apart)
        if k not in seen:
            seen[k] = len(lst)
            lst.append(v)
        return seen[k]

    def enc(o):
        o = list(o)
        if isinstance(o[1], str):
            o[1] = idx(messages, o[1])
        return idx(outcomes, o)

    packed = {"constructor": {k: [enc(o) for o in v] for k, v in table["constructor"].items()},
              "small": {k: [enc(o) for o in v] for k, v in table["small"].items()},
              "configure": {k: [[enc(o) for o in row] for row in v] for k, v in table["configure"].items()}}
    return dict(axes=[[k, list(v)] for k, v in AXES], changes=list(CHANGES), dec_kernels=list(DEC_KERNELS),
                messages=messages, outcomes=outcomes, **packed)


def unpack(data):
    def dec(i):
        o = list(data["outcomes"][i])
        if isinstance(o[1], int):               # (a message's index; an accepted constructor case has its plan there)
            o[1] = data["messages"][o[1]]
        return o
    return {"constructor": {k: [dec(i) for i in v] for k, v in data["constructor"].items()},
            "small": {k: [dec(i) for i in v] for k, v in data["small"].items()},
            "configure": {k: [[dec(i) for i in row] for row in v] for k, v in data["configure"].items()}}
