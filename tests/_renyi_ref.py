"""
_renyi_ref.py — the reference of the importance-weighted (Renyi / IWAE) bound the tests of
SVItrainer(loss="RenyiELBO") / engine(particles=P, renyi=alpha) compare against.

What it restates: pyro.infer.RenyiELBO(alpha, num_particles=P) on iVAE.guide / iVAE.model.  The `data` plate encloses
every site of these models, so Pyro's log-weights stay per image; the encoder's output does not depend on the draw, so
it is evaluated once (as tests/_particles_ref.py does):

    z_pb  = mu_b + sigma_b * eps_pb
    lw_pb = log p(x_b | z_pb) + beta * (log p(z_pb) - log q(z_pb | x_b))
    a_pb  = (1 - alpha) * lw_pb,   w_pb = softmax over p of a_pb
    L_b   = (logsumexp_p a_pb - log P) / (1 - alpha)
    loss  = -sum_b L_b

`eps` is ONE (P*B, z_dim) tensor with rows ordered [p][b].  The gradient of `loss` is autograd's — it equals
-sum_b sum_p w_pb grad lw_pb with w held constant, which is what the library computes; `weights=` (a (P*B) tensor, rows
[p][b]) evaluates exactly that surrogate, -sum w lw + const, with the GIVEN weights held fixed (const places the value on
the bound of those weights: their entropy term).

The four scalars keep the slots every other objective has, loss = -(ll + logpz - logqz):
    logpz = sum_b sum_p w_pb beta log p(z_pb),   logqz = sum_b sum_p w_pb beta log q(z_pb | x_b)
    ll    = sum_b (sum_p w_pb ll_pb + c_b),      c_b = L_b - sum_p w_pb lw_pb = (H(w_b) - log P) / (1 - alpha)

RenyiOracle subclasses oracle.svi_oracle.SVIOracle and overrides only the loss.  tests/test_renyi_cpu.py pins it: P = 1
is the parent exactly, alpha -> 1 meets tests/_particles_ref.ParticlesOracle.
"""
import math

import torch
import torch.distributions as td

from oracle import svi_oracle as orc


def renyi_elbo(p, cfg, x, eps, particles, alpha=0.0, beta=1.0, y=None, grid=None, weights=None):
    b, P = x.shape[0], int(particles)
    assert eps.shape[0] == P * b, "eps must be (particles * batch, z_dim), rows [p][b]"
    assert alpha != 1.0 and math.isfinite(alpha)
    z_loc, z_scale = orc._encode_any(p, cfg, x, y)                              # once, on the B images
    zl, zs = z_loc.repeat(P, 1), z_scale.repeat(P, 1)                           # row p*B + b = image b
    z = zl + zs * eps
    logq = beta * td.Normal(zl, zs).log_prob(z).sum(-1)
    logp = beta * td.Normal(torch.zeros_like(z), torch.ones_like(z)).log_prob(z).sum(-1)
    yy = None if y is None else y.repeat(P, 1)
    loc, xc = orc.decode_from_latent(p, cfg, z, yy, grid)
    ll = orc.likelihood(cfg, loc.reshape(P * b, -1)).log_prob(x.reshape(b, -1).repeat(P, 1)).sum(-1)
    if P == 1:
        # one sample: L_b = lw_b whatever alpha is — written as oracle.svi_oracle.elbo writes it, so that P = 1 is that
        # oracle bit for bit
        t_ll, t_lp, t_lq = ll.sum(), logp.sum(), logq.sum()
        w = torch.ones_like(ll)
        return dict(loss=-(t_ll + t_lp - t_lq), ll=t_ll, logpz=t_lp, logqz=t_lq, weights=w, log_weights=torch.zeros_like(ll),
                    ll_per_sample=ll, z_loc=z_loc, z_scale=z_scale, z=z, loc=loc, x_coord_prime=xc)
    lw = (ll + logp - logq).view(P, b)
    a = (1.0 - alpha) * lw
    if weights is None:
        logw = torch.log_softmax(a, 0).detach()
        w = logw.exp()
        bound = (torch.logsumexp(a, 0) - math.log(P)) / (1.0 - alpha)           # L_b
        loss = -bound.sum()
    else:
        w = weights.detach().to(lw.dtype).view(P, b)
        logw = torch.log(w.clamp_min(torch.finfo(lw.dtype).tiny))
        # the surrogate: value sum_p w lw + (H(w) - log P) / (1 - alpha) per image, gradient that of sum_p w lw
        ent = -(w * logw).sum(0)
        bound = (w * lw).sum(0) + (ent - math.log(P)) / (1.0 - alpha)
        loss = -bound.sum()
    wf = w.reshape(-1)
    t_lp, t_lq = (wf * logp).sum(), (wf * logq).sum()
    t_ll = -loss - t_lp + t_lq                                                  # sum_b (sum_p w ll + c_b)
    return dict(loss=loss, ll=t_ll, logpz=t_lp, logqz=t_lq, weights=wf, log_weights=logw.reshape(-1), ll_per_sample=ll,
                z_loc=z_loc, z_scale=z_scale, z=z, loc=loc, x_coord_prime=xc, bound_per_image=bound)


class RenyiOracle(orc.SVIOracle):
    """SVI.step with RenyiELBO(alpha, num_particles=P).  `weights` (set by a test, consumed by the next evaluation): the
    surrogate with those weights held fixed."""

    def __init__(self, params, cfg, particles, alpha=0.0, lr=1e-3, dtype=torch.float64):
        super().__init__(params, cfg, lr=lr, dtype=dtype)
        self.particles, self.alpha = int(particles), float(alpha)
        self.weights = None

    def loss_and_grads(self, x, eps, beta=1.0, y=None):
        assert self.cfg.discrete_dim == 0, "the Renyi reference covers iVAE-class models only"
        w, self.weights = self.weights, None
        out = renyi_elbo(self.p, self.cfg, x.to(self.dtype), eps.to(self.dtype), self.particles, self.alpha, beta,
                         None if y is None else y.to(self.dtype), self.grid, weights=w)
        if out["loss"].requires_grad:
            out["loss"].backward()
        self.last = out
        return out

    def draw_eps(self, b):
        """P sequential draws on the global CPU generator (P runs of the guide), stacked [p][b]."""
        return torch.cat([torch.empty(b, self.cfg.z_dim).normal_() for _ in range(self.particles)])
