"""
_image_weight_cases.py — the weights, the reference and the case table the tests of per-IMAGE observation weights run on
(SVItrainer(model, image_weights=True) / model.engine(image_weights=True) + loss_and_grads(..., image_weights=w);
pv_ivae_weighted_images_* in the C ABI).

The objective: loss = -( sum_b sum_i w_bi log p(x_bi | z_b) + beta sum_b [log p(z_b) - log q(z_b | x_b)] ), w_bi >= 0, one entry
per observed value of every image (the layout of x, channel-last).  The reference is ImageWeightedOracle below:
_pixel_weight_cases.WeightedOracle with self.w shaped (b, n_pix * C) — its line ll = (lp * self.w).sum(-1) does the rest.
The cases are _pixel_weight_cases.CASES with per-image makers in place of the shared ones (disc -> pdisc, ramp -> pramp,
soft -> psoft), the same paths and uses_fused expectations, and some images masked out completely.
"""
import torch

from oracle import svi_oracle as orc
import _pixel_weight_cases as pw


# ------------------------------------------------------------------------------- weights, (b, *dims, C)
def pdisc(b, dims, C):
    """A disc per image on linspace(-1, 1) axes: centre 0.5 (rand(b, ndim) - 0.5), radius 0.55 + 0.4 rand(b), drawn in that order
    from generator seed 11; 1 inside, 0 outside, the same in every channel."""
    g = torch.Generator().manual_seed(11)
    centre = 0.5 * (torch.rand(b, len(dims), generator=g) - 0.5)
    radius = 0.55 + 0.4 * torch.rand(b, generator=g)
    mesh = torch.meshgrid(*[torch.linspace(-1.0, 1.0, d) for d in dims], indexing="ij")
    r2 = sum((m.unsqueeze(0) - centre[:, k].reshape(b, *([1] * len(dims)))) ** 2 for k, m in enumerate(mesh))
    inside = r2 <= (radius ** 2).reshape(b, *([1] * len(dims)))
    return inside.to(torch.float32).unsqueeze(-1).expand(b, *dims, C).contiguous()


def pramp(b, dims, C):
    """2 rand per (image, position, channel), entries below 0.3 set to 0: fractional weights and exact zeros."""
    w = 2.0 * torch.rand(b, *dims, C, generator=torch.Generator().manual_seed(7))
    return torch.where(w < 0.3, torch.zeros_like(w), w)


def psoft(b, dims, C):
    """0.25 + 1.5 rand: strictly positive."""
    return 0.25 + 1.5 * torch.rand(b, *dims, C, generator=torch.Generator().manual_seed(7))


MAKERS = {"pdisc": pdisc, "pramp": pramp, "psoft": psoft}
_PER_IMAGE = {"disc": "pdisc", "ramp": "pramp", "soft": "psoft"}


def weights(c):
    """The case's weights, (b, *dims, C) — the images listed in c["zero"] masked out completely."""
    w = MAKERS[c["w"]](c["b"], tuple(c["dims"]), c["C"])
    for i in c.get("zero", ()):
        w[i] = 0.0
    return w


def shared_as_images(c):
    """A _pixel_weight_cases case's SHARED weights repeated for every image: (b, *dims, C)."""
    w = pw.MAKERS[c["w"]](tuple(c["dims"]), c["C"])
    return w.unsqueeze(0).expand(c["b"], *w.shape).contiguous()


# ------------------------------------------------------------------------------- the reference
class ImageWeightedOracle(pw.WeightedOracle):
    """WeightedOracle with one weight per observed value of every image: self.w is (b, n_pix * C), so that WeightedOracle's
    ll = (lp * self.w).sum(-1) weighs image b's log-probabilities with row b.  set_weights swaps in another batch's rows."""

    def __init__(self, params, cfg, w, lr=1e-3, dtype=torch.float32, kl="sampled"):
        orc.SVIOracle.__init__(self, params, cfg, lr=lr, dtype=dtype, kl=kl)
        self.set_weights(w)

    def set_weights(self, w):
        w = torch.as_tensor(w)
        self.w = w.reshape(w.shape[0], -1).to(self.dtype)
        assert self.w.shape[1] == self.cfg.n_pix * self.cfg.channels, "one weight per observed value of every image"


# ------------------------------------------------------------------------------- cases
def _case(name, zero=()):
    c = dict(pw.CASES[name])
    c["w"] = _PER_IMAGE[c["w"]]
    if zero:
        c["zero"] = tuple(zero)
    return c


CASES = {
    "i01_8x8_rts_c1_b6_pdisc": _case("w01_8x8_rts_c1_b6_disc", zero=(2,)),
    "i02_1d32_t_c1_b5_gauss_nosig_pramp": _case("w02_1d32_t_c1_b5_gauss_nosig_ramp"),
    "i03_8x8_r_c3_b6_poisson_pramp": _case("w03_8x8_r_c3_b6_poisson_ramp"),
    "i04_8x8_rts_c2_cdim3_b6_cbern_pdisc": _case("w04_8x8_rts_c2_cdim3_b6_cbern_disc"),
    "i05_28x28_rt_c1_b16_gauss_pdisc": _case("w05_28x28_rt_c1_b16_gauss_disc"),
    "i06_16x16_r_c8_b160_pramp": _case("w06_16x16_r_c8_b160_ramp", zero=(0, 159)),
    "i07_7x9_rt_c1_b3_72_40_softplus_pramp": _case("w07_7x9_rt_c1_b3_72_40_softplus_ramp"),
    "i08_7x9_rt_c3_b3_gauss_nosig_72_40_softplus_pramp": _case("w08_7x9_rt_c3_b3_gauss_nosig_72_40_softplus_ramp"),
    "i09_8x8_none_c1_b6_psoft": _case("w09_8x8_none_c1_b6_soft"),
    "i10_8x8_none_c2_b6_psoft": _case("w10_8x8_none_c2_b6_soft"),
}
CASE1 = "i01_8x8_rts_c1_b6_pdisc"

case_data = pw.case_data
case_config = pw.case_config
