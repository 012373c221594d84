"""
_multichannel_ref.py — the reference of multi-channel models, iVAE(..., channels=C), and the data their tests run on.

Semantics: the data has P = prod(data_dim) grid positions and C values per position, channel-last: x is (B, *data_dim, C).
The spatial decoder is the single-channel one up to its last hidden layer (one row per sample and position); its output
layer is Linear(H, C).  The likelihood and the output sigmoid apply per value, log p(x_b | z_b) sums over positions and
channels, the encoder sees the flattened (B, P*C [+ c_dim]).  A vanilla model's decoder ends in Linear(H, P*C).

oracle/svi_oracle.py decodes one value per position and is not edited: `attach(o, C)` gives an oracle of that module (or of
tests/_meanfield_ref, _particles_ref, _renyi_ref, which subclass it) a `Config.custom_decoder` — a closure over the oracle's
OWN parameter dict o.p, so autograd reaches the leaves its Adam steps — that restates the C-output decoder and returns
(B, P*C) channel-last.  Everything else (encoder, priors, KL forms, likelihoods incl. tests/_poisson_ref.poisson_reference(),
Adam, the epoch loops) is the oracle's, unchanged.  With C = 1 the closure is oracle.svi_oracle.sdecoder_forward /
fcdecoder_forward up to the final reshape (tests/test_multichannel_cpu.py pins that to 1e-12 in float64).
"""
import torch
import torch.nn.functional as F

from oracle import svi_oracle as orc


def config(dims, inv, **kw):
    return orc.Config(data_dim=tuple(dims), latent_dim=2, invariances=inv, **kw)


def attach(o, C):
    """Make oracle `o` a C-channel model: its cfg gets the custom decoder described above.  Returns o."""
    cfg, p = o.cfg, o.p
    act = orc._ACT[cfg.activation]

    def head(h, b):
        out = F.linear(h, p["decoder.out.weight"], p["decoder.out.bias"])
        if cfg.sigmoid_d:
            out = torch.sigmoid(out)
        return out.reshape(b, -1)

    if cfg.coord > 0:
        assert p["decoder.out.weight"].shape[0] == C

        def decoder(x_coord, z):
            b, n = x_coord.shape[:2]
            h_x = F.linear(x_coord.reshape(b * n, -1), p["decoder.coord_latent.fc_coord.weight"],
                           p["decoder.coord_latent.fc_coord.bias"]).reshape(b, n, -1)
            h_z = F.linear(z, p["decoder.coord_latent.fc_latent.weight"])
            h = torch.tanh((h_x + h_z.unsqueeze(1)).reshape(b * n, -1))
            h = orc._fc_stack(p, "decoder.fc_layers", cfg.n_hidden_d, act, h)
            return head(h, b)                       # rows (b, n) x C values -> (b, n*C): channel-last
    else:
        assert p["decoder.out.weight"].shape[0] == cfg.n_pix * C

        def decoder(z):
            return head(orc._fc_stack(p, "decoder.fc_layers", cfg.n_hidden_d, act, z), z.shape[0])

    cfg.custom_decoder = decoder
    o.channels = C
    return o


def decode(o, z, y=None, angle=0.0, shift=0.0, scale=1.0):
    """SVIOracle.decode for an attached oracle: (n, *data_dim, C); Poisson models: the rate."""
    cfg = o.cfg
    with torch.no_grad():
        z = z.to(o.dtype)
        if y is not None:
            z = torch.cat([z, y.to(o.dtype)], -1)
        if cfg.coord > 0:
            g = o.grid.unsqueeze(0)
            a = torch.as_tensor(angle, dtype=o.dtype).reshape(1)
            t = torch.as_tensor(shift, dtype=o.dtype).reshape(-1)          # (a 1-D grid takes the first entry, as the model does)
            t = (t.expand(cfg.ndim) if t.numel() == 1 else t[:cfg.ndim]).unsqueeze(0)
            s = torch.as_tensor(scale, dtype=o.dtype).reshape(1)
            g = orc.transform_coordinates(g, a, t, s).squeeze(0)
            out = cfg.custom_decoder(g.expand(z.shape[0], *g.shape), z)
        else:
            out = cfg.custom_decoder(z)
        if cfg.sampler == "poisson_log":
            out = torch.exp(out.clamp(max=30.0))
        return out.reshape(z.shape[0], *cfg.data_dim, o.channels)


# ------------------------------------------------------------------------------- data
def _bumps(g, batch, dims, C):
    """exp(-d^2 / 0.18) around a centre per (image, channel), rand - 0.5 per axis, on linspace(-1, 1) axes: (batch, C, *dims);
    and the amplitudes 0.5 + 0.4 c / (C - 1), shaped to broadcast."""
    cen = torch.rand(batch, C, len(dims), generator=g) - 0.5
    mesh = torch.meshgrid(*[torch.linspace(-1.0, 1.0, d) for d in dims], indexing="ij")
    d2 = 0.0
    for i, m in enumerate(mesh):
        d2 = d2 + (m.reshape(1, 1, *dims) - cen[:, :, i].reshape(batch, C, *([1] * len(dims)))) ** 2
    amp = 0.5 + 0.4 * torch.arange(C, dtype=torch.float32) / max(C - 1, 1)
    return torch.exp(-d2 / 0.18), amp.reshape(1, C, *([1] * len(dims)))


def _channel_last(t):
    return t.permute(0, *range(2, t.dim()), 1).contiguous()


def images(g, batch, dims, C):
    """(batch, *dims, C) in (0, 1): x = 0.05 + amp_c exp(-d^2 / 0.18).  The channels differ in centre and amplitude, so an
    implementation that swaps or merges channels cannot pass.  The caller draws its eps from g afterwards."""
    e, amp = _bumps(g, batch, tuple(dims), C)
    return _channel_last(0.05 + amp * e)


def counts(g, batch, dims, C):
    """(batch, *dims, C) Poisson counts of rate 1 + 2 amp_c exp(-d^2 / 0.18)."""
    e, amp = _bumps(g, batch, tuple(dims), C)
    return _channel_last(torch.poisson(1.0 + 2.0 * amp * e, generator=g))


# ------------------------------------------------------------------------------- the GPU tests' cases
# (tests/test_gpu_multichannel.py runs them; tests/test_multichannel_cpu.py confirms, with the reference alone, the condition
#  its parameter check rests on).  Hidden sizes [128, 128] unless stated; no lrelu / relu decoder: their exact zeros of the
#  activation's derivative put ~7 % of a gradient tensor's entries under the near-zero threshold, above the 1 % cap.
CASES = {
    "c01_8x8_rts_c2_b6": dict(dims=(8, 8), inv=["r", "t", "s"], C=2, b=6),                                  # 384 rows: whole workgroups
    "c02_7x9_rt_c3_b3_gauss_nosig_72_40_softplus": dict(dims=(7, 9), inv=["r", "t"], C=3, b=3, sampler="gaussian",
                                                        sigmoid_d=False, hidden_d=[72, 40], activation="softplus"),
    "c03_1d16_t_c4_b5_gelu": dict(dims=(16,), inv=["t"], C=4, b=5, activation="gelu"),
    "c04_8x8_r_c3_b6_poisson": dict(dims=(8, 8), inv=["r"], C=3, b=6, sampler="poisson_log", sigmoid_d=False),
    "c05_4x4_r_c8_b2_512_512": dict(dims=(4, 4), inv=["r"], C=8, b=2, hidden_d=[512, 512]),
    "c06_8x8_rts_c2_cdim3_b6": dict(dims=(8, 8), inv=["r", "t", "s"], C=2, b=6, c_dim=3),
    "c07_6x6_r_c5_b4_softplus": dict(dims=(6, 6), inv=["r"], C=5, b=4, activation="softplus"),
    "c08_6x6_r_c7_b4_gauss": dict(dims=(6, 6), inv=["r"], C=7, b=4, sampler="gaussian"),
    "c09_6x6_r_c6_b4_cbern": dict(dims=(6, 6), inv=["r"], C=6, b=4, sampler="continuous_bernoulli"),
    "c10_28x28_rt_c3_b16": dict(dims=(28, 28), inv=["r", "t"], C=3, b=16),                                  # 12 544 rows, 196 workgroups
    "c11_8x8_none_c2_b6": dict(dims=(8, 8), inv=None, C=2, b=6),                                            # vanilla decoder
}


def model_kwargs(c):
    """models.iVAE keyword arguments of a case."""
    kw = dict(channels=c["C"], c_dim=c.get("c_dim", 0), activation=c.get("activation", "tanh"),
              sampler_d=c.get("sampler", "bernoulli"), sigmoid_d=c.get("sigmoid_d", True))
    if "hidden_d" in c:
        kw["hidden_dim_d"] = list(c["hidden_d"])
    return kw


def case_config(c):
    return config(c["dims"], c["inv"], c_dim=c.get("c_dim", 0), activation=c.get("activation", "tanh"),
                  sampler=c.get("sampler", "bernoulli"), sigmoid_d=c.get("sigmoid_d", True))


def case_data(c, particles=1):
    """(x, y, [eps of step 0, eps of step 1]) from torch.Generator().manual_seed(0): the data first, then the eps draws
    (each (particles * b, z_dim), rows [p][b])."""
    g = torch.Generator().manual_seed(0)
    make = counts if c.get("sampler") == "poisson_log" else images
    x = make(g, c["b"], c["dims"], c["C"])
    z_dim = case_config(c).z_dim
    eps = [torch.randn(particles * c["b"], z_dim, generator=g) for _ in range(2)]
    y = None
    if c.get("c_dim"):
        y = torch.zeros(c["b"], c["c_dim"])
        y[torch.arange(c["b"]), torch.arange(c["b"]) % c["c_dim"]] = 1.0
    return x, y, eps


def round_to_float32(o):
    """Both sides of a step test continue from the SAME float32 parameters."""
    with torch.no_grad():
        for v in o.p.values():
            v.copy_(v.float().to(v.dtype))
