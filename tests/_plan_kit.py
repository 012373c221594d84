"""
_plan_kit.py — what the CPU tests of the objectives, likelihoods and channel counts share: the pv_ivae_plan structs they
validate through the library's host-side queries, the pinned field list, a stand-in engine for the trainer's argument
handling, and the small float64 inputs of the reference-only tests.
"""
import torch

import pyroved_amd as pv
from pyroved_amd import _abi

SLOTS = ("loss", "ll", "logpz", "logqz")
# (data_dim, invariances, c_dim)
CASES = [((8, 8), ["r", "t", "s"], 0), ((16,), ["t"], 0), ((8, 8), None, 0), ((8, 8), ["r", "t"], 3)]


# ------------------------------------------------------------------------------- reference-only inputs
def _params(cfg, seed=0, c_dim=0):
    model = pv.models.iVAE(cfg.data_dim, cfg.latent_dim, cfg.invariances, c_dim=c_dim, seed=1, device="cpu")
    g = torch.Generator().manual_seed(seed)
    return {k: (v.detach() + 0.05 * torch.randn(v.shape, generator=g)).double() for k, v in model.state_dict().items()}


def _inputs(cfg, b, P, seed=3, c_dim=0):
    g = torch.Generator().manual_seed(seed)
    x = torch.rand(b, *cfg.data_dim, generator=g, dtype=torch.float64)
    eps = torch.randn(P * b, cfg.z_dim, generator=g, dtype=torch.float64)
    y = None
    if c_dim:
        y = torch.zeros(b, c_dim, dtype=torch.float64)
        y[torch.arange(b), torch.arange(b) % c_dim] = 1.0
        x = x.flatten(1)
    return x, eps, y


# ------------------------------------------------------------------------------- trainer arguments
class _StandInEngine:
    device = torch.device("cpu")
    grads_live = False
    kl = "unset"
    particles = "unset"

    def __init__(self):
        self.lr = self.betas = self.adam_eps = None

    def reset_optimizer(self):
        pass


def _ivae():
    return pv.models.iVAE((8, 8), 2, ["r"], seed=1, device="cpu")


def _plain_loop(loader, z_dim, P):
    """What Pyro's P runs of the guide per step draw: P tensors torch.empty(B, z_dim).normal_() in particle order."""
    out = []
    for data in loader:
        b = data[0].shape[0]
        out.append(torch.cat([torch.empty(b, z_dim).normal_() for _ in range(P)]))
    return out


def _free_port():
    import socket
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


# ------------------------------------------------------------------------------- ABI
PLAN_FIELDS = [
    "batch", "n_pix", "coord_dim", "z_dim", "latent_dim", "c_dim", "has_r", "has_t", "has_s", "t_prior", "sc_prior", "beta", "lik",
    "sigmoid_out", "decoder_sig", "fused", "discrete_dim", "beta_disc", "n_enc", "n_dec", "enc", "head", "fc_coord", "fc_latent",
    "dec", "out", "n_enc_ops", "enc_ndim", "enc_in_dim", "enc_ops", "params", "grads", "adam_m", "adam_v", "n_params", "x", "y",
    "eps", "grid", "ws", "ws_bytes", "scalars", "z_loc", "z_scale", "loc", "alpha", "ext_head", "ext_dhead", "ext_encoder",
    "bn_eval", "row_w", "row_elbo", "dy", "ext_z", "ext_dz", "ext_ll", "ext_decoder", "conv_wide", "lr", "adam_beta1", "adam_beta2",
    "adam_eps", "adam_step", "flags", "ev_start", "ev_stop", "class_onehot", "conv_ev_start", "conv_ev_stop", "conv_ev_flops",
    "dec_kernel", "kl_mode",
]


def _small_plan(discrete_dim=0, fused=2):
    p = _abi.pv_ivae_plan()
    p.batch, p.n_pix, p.coord_dim, p.z_dim, p.latent_dim = 16, 784, 2, 5, 2
    p.has_r = p.has_t = 1
    p.lik, p.sigmoid_out, p.fused = _abi.LIK["bernoulli"], 1, fused

    def layer(i, o, act):
        l = _abi.pv_layer()
        l.in_dim, l.out_dim, l.act, l.b_off = i, o, _abi.ACT[act], 0
        return l
    p.n_enc = 2
    p.enc[0], p.enc[1] = layer(784, 128, "tanh"), layer(128, 128, "tanh")
    p.discrete_dim = discrete_dim
    p.head = layer(128, 10 + discrete_dim, None)
    p.fc_coord, p.fc_latent = layer(2, 128, "tanh"), layer(2 + discrete_dim, 128, None)
    p.n_dec = 2
    p.dec[0], p.dec[1] = layer(128, 128, "tanh"), layer(128, 128, "tanh")
    p.out = layer(128, 1, None)
    return p


def _plan(fused=2, channels=1, discrete_dim=0):
    """_small_plan with `channels` observations per position: 784 positions x channels, batch 16"""
    p = _small_plan(discrete_dim=discrete_dim, fused=fused)
    p.out.out_dim = channels
    p.n_pix = 784 * channels
    p.enc[0].in_dim = 784 * channels
    return p


def _vanilla_plan(fused=2):
    p = _plan(fused)
    p.coord_dim, p.z_dim, p.latent_dim, p.has_r, p.has_t = 0, 2, 2, 0, 0
    p.head.out_dim = 4
    p.dec[0].in_dim = 2
    p.out.out_dim = 784
    return p
