"""
_pixel_weight_cases.py — the weights, the reference and the case table the tests of per-observation weights run on
(SVItrainer(model, pixel_weights=w) / model.engine(pixel_weights=w); pv_ivae_weighted_* in the C ABI).

The objective: loss = -( sum_b sum_i w_i log p(x_bi | z_b) + beta sum_b [log p(z_b) - log q(z_b | x_b)] ), w >= 0 shared by all
images, one entry per observed value (positions x channels, channel-last).  The reference is WeightedOracle below: orc.elbo for
one particle restated with ll = (log_prob * w).sum(-1).  Data and eps come from _multichannel_cases.case_data (one channel: the
channel axis squeezed away).
"""
import torch
import torch.distributions as td

from oracle import svi_oracle as orc
import _multichannel_cases as mc


# ------------------------------------------------------------------------------- weights, (*dims, C)
def disc(dims, C):
    """1 where the pixel's linspace(-1, 1) coordinates have r^2 <= 1, else 0; the same in every channel."""
    mesh = torch.meshgrid(*[torch.linspace(-1.0, 1.0, d) for d in dims], indexing="ij")
    r2 = sum(m ** 2 for m in mesh)
    return (r2 <= 1.0).to(torch.float32).unsqueeze(-1).expand(*dims, C).contiguous()


def ramp(dims, C):
    """2 rand per (position, channel), entries below 0.3 set to 0: fractional weights and exact zeros."""
    w = 2.0 * torch.rand(*dims, C, generator=torch.Generator().manual_seed(7))
    return torch.where(w < 0.3, torch.zeros_like(w), w)


def soft(dims, C):
    """0.25 + 1.5 rand: strictly positive."""
    return 0.25 + 1.5 * torch.rand(*dims, C, generator=torch.Generator().manual_seed(7))


MAKERS = {"disc": disc, "ramp": ramp, "soft": soft}


def weights(c, kind=None):
    """The case's weights as the engine takes them: (*dims, C), or (*dims) for one channel."""
    w = MAKERS[kind or c["w"]](tuple(c["dims"]), c["C"])
    return w[..., 0].contiguous() if c["C"] == 1 else w


# ------------------------------------------------------------------------------- the reference
class WeightedOracle(orc.SVIOracle):
    """SVIOracle whose objective is the one-particle ELBO with per-observation weights: orc.elbo's statements in orc.elbo's order
    (so that weights of ones give its bits), with ll = (log_prob * w).sum(-1).  Same keys in the returned dict."""

    def __init__(self, params, cfg, w, lr=1e-3, dtype=torch.float32, kl="sampled"):
        super().__init__(params, cfg, lr=lr, dtype=dtype, kl=kl)
        self.w = torch.as_tensor(w).reshape(-1).to(dtype)
        assert self.w.numel() == cfg.n_pix * cfg.channels, "one weight per observed value (positions x channels)"

    def loss_and_grads(self, x, eps, beta=1.0, y=None):
        p, cfg = self.p, self.cfg
        x, eps = x.to(self.dtype), eps.to(self.dtype)
        y = None if y is None else y.to(self.dtype)
        b = x.shape[0]
        z_loc, z_scale = orc._encode_any(p, cfg, x, y)
        z = z_loc + z_scale * eps
        if self.kl == "analytic":
            kl_b, t_lp, t_lq = orc._kl_and_slots(z_loc, z_scale, beta)
        else:
            logq = td.Normal(z_loc, z_scale).log_prob(z).sum(-1)
            logp = td.Normal(torch.zeros_like(z), torch.ones_like(z)).log_prob(z).sum(-1)
        loc, xc = orc.decode_from_latent(p, cfg, z, y, self.grid)
        lp = orc.likelihood(cfg, loc.reshape(b, -1)).log_prob(x.reshape(b, -1))
        ll = (lp * self.w).sum(-1)
        out = dict(z_loc=z_loc, z_scale=z_scale, z=z, loc=loc, x_coord_prime=xc, ll_per_sample=ll)
        t_ll = ll.sum()
        if self.kl == "analytic":
            out.update(loss=-t_ll + (beta * kl_b).sum(), kl=kl_b)
        else:
            t_lp, t_lq = (beta * logp).sum(), (beta * logq).sum()
            out.update(loss=-(t_ll + t_lp - t_lq))
        out = dict(out, ll=t_ll, logpz=t_lp, logqz=t_lq)
        if out["loss"].requires_grad:
            out["loss"].backward()
        self.last = out
        return out


# ------------------------------------------------------------------------------- cases
# entries as _multichannel_cases.CASES, plus  w: the weight maker;  paths: the engine keywords of every path the GPU step test
# runs the case on (next to pixel_weights);  fused: whether that path is the weighted fused f32 kernel.
# Hidden sizes [128, 128], tanh unless stated.  The vanilla cases use strictly positive weights: with a 0 / 1 mask half of
# decoder.out.weight's rows have an exactly zero gradient, which breaches the parameter check's 1 % cap (a separate GPU test
# covers the mask).
FUSED, FUSED_MC, LAYERED = dict(), dict(fused_channels=True), dict(fused=0)
CASES = {
    # fused weighted C = 1, one unit per workgroup
    "w01_8x8_rts_c1_b6_disc": dict(dims=(8, 8), inv=["r", "t", "s"], C=1, b=6, w="disc", paths=[(FUSED, True)]),
    # one coordinate
    "w02_1d32_t_c1_b5_gauss_nosig_ramp": dict(dims=(32,), inv=["t"], C=1, b=5, sampler="gaussian", sigmoid_d=False, w="ramp",
                                              paths=[(FUSED, True)]),
    # the weighted normaliser, fused and layered
    "w03_8x8_r_c3_b6_poisson_ramp": dict(dims=(8, 8), inv=["r"], C=3, b=6, sampler="poisson_log", sigmoid_d=False, w="ramp",
                                         paths=[(FUSED_MC, True), (LAYERED, False)]),
    # [z | y], weighted log C
    "w04_8x8_rts_c2_cdim3_b6_cbern_disc": dict(dims=(8, 8), inv=["r", "t", "s"], C=2, b=6, c_dim=3,
                                               sampler="continuous_bernoulli", w="disc", paths=[(FUSED_MC, True)]),
    # 784 units on 256 workgroups, images split over workgroups
    "w05_28x28_rt_c1_b16_gauss_disc": dict(dims=(28, 28), inv=["r", "t"], C=1, b=16, sampler="gaussian", w="disc",
                                           paths=[(FUSED, True)]),
    # 10 units per workgroup, n wrapping at an image boundary inside a workgroup, the widest C
    "w06_16x16_r_c8_b160_ramp": dict(dims=(16, 16), inv=["r"], C=8, b=160, w="ramp", paths=[(FUSED_MC, None)]),
    # layered pv_out_lik (63 positions)
    "w07_7x9_rt_c1_b3_72_40_softplus_ramp": dict(dims=(7, 9), inv=["r", "t"], C=1, b=3, hidden_d=[72, 40], activation="softplus",
                                                 w="ramp", paths=[(FUSED, False)]),
    # layered pv_out_lik_mc
    "w08_7x9_rt_c3_b3_gauss_nosig_72_40_softplus_ramp": dict(dims=(7, 9), inv=["r", "t"], C=3, b=3, sampler="gaussian",
                                                             sigmoid_d=False, hidden_d=[72, 40], activation="softplus", w="ramp",
                                                             paths=[(FUSED, False)]),
    # vanilla decoder
    "w09_8x8_none_c1_b6_soft": dict(dims=(8, 8), inv=None, C=1, b=6, w="soft", paths=[(FUSED, False)]),
    "w10_8x8_none_c2_b6_soft": dict(dims=(8, 8), inv=None, C=2, b=6, w="soft", paths=[(FUSED, False)]),
}
CASE1 = "w01_8x8_rts_c1_b6_disc"


def case_data(c):
    """_multichannel_cases.case_data; one channel: x is (b, *dims)."""
    x, y, eps = mc.case_data(c)
    return (x[..., 0].contiguous() if c["C"] == 1 else x), y, eps


def case_config(c):
    return mc.case_config(c)
