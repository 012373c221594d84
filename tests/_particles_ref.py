"""
_particles_ref.py — the reference of the multi-particle ELBO the tests of SVItrainer(num_particles=P) /
engine(particles=P) compare against.

What it restates: pyro.infer.Trace_ELBO(num_particles=P) and TraceMeanField_ELBO(num_particles=P) on iVAE.guide /
iVAE.model.  Pyro's (non-vectorised) particles run the guide P times on the same minibatch and average the P
one-particle estimates; the encoder's output does not depend on the draw, so it is evaluated once here:

    z_pb = mu_b + sigma_b * eps_pb
    e_pb = log p(x_b | z_pb) + beta * (log p(z_pb) - log q(z_pb | x_b))          sampled form
    e_pb = log p(x_b | z_pb) - beta * KL(N(mu_b, sigma_b) || N(0, 1))            analytic form
    loss = -(1/P) * sum_p sum_b e_pb

`eps` is ONE (P*B, z_dim) tensor with rows ordered [p][b]; `loc` comes back (P*B, ...) in the same order, z_loc and
z_scale stay (B, z_dim).  The four scalars keep the one-particle slots and loss = -(ll + logpz - logqz): each is the mean
over particles of the term it holds there.

The oracles subclass oracle.svi_oracle.SVIOracle and tests/_meanfield_ref.MeanFieldOracle and override only the loss;
Adam, zero_grads and the epoch loops' step are inherited.  tests/test_particles_cpu.py pins them to their parents: P = 1
is the parent exactly, P = 3 the mean of three parent evaluations.
"""
import torch
import torch.distributions as td

from oracle import svi_oracle as orc
import _meanfield_ref as mf


def particles_elbo(p, cfg, x, eps, particles, beta=1.0, y=None, grid=None, analytic=False):
    b, P = x.shape[0], int(particles)
    assert eps.shape[0] == P * b, "eps must be (particles * batch, z_dim), rows [p][b]"
    z_loc, z_scale = orc._encode_any(p, cfg, x, y)                              # once, on the B images
    zl, zs = z_loc.repeat(P, 1), z_scale.repeat(P, 1)                           # row p*B + b = image b
    z = zl + zs * eps
    kl = None
    if analytic:
        kl, t_lp, t_lq = mf._kl_and_slots(z_loc, z_scale, beta)                 # does not depend on p
    else:
        logq = td.Normal(zl, zs).log_prob(z).sum(-1)
        logp = td.Normal(torch.zeros_like(z), torch.ones_like(z)).log_prob(z).sum(-1)
        t_lp, t_lq = (beta * logp).sum() / P, (beta * logq).sum() / P
    yy = None if y is None else y.repeat(P, 1)
    loc, xc = orc.decode_from_latent(p, cfg, z, yy, grid)
    ll = orc.likelihood(cfg, loc.reshape(P * b, -1)).log_prob(x.reshape(b, -1).repeat(P, 1)).sum(-1)
    t_ll = ll.sum() / P
    # (the analytic form as tests/_meanfield_ref.py writes it, so that P = 1 is that oracle bit for bit)
    loss = -t_ll + (beta * kl).sum() if analytic else -(t_ll + t_lp - t_lq)
    return dict(loss=loss, ll=t_ll, logpz=t_lp, logqz=t_lq, z_loc=z_loc, z_scale=z_scale, z=z, loc=loc,
                x_coord_prime=xc, ll_per_sample=ll)


class _ParticlesMixin:
    analytic = False

    def __init__(self, params, cfg, particles, lr=1e-3, dtype=torch.float64):
        super().__init__(params, cfg, lr=lr, dtype=dtype)
        self.particles = int(particles)

    def loss_and_grads(self, x, eps, beta=1.0, y=None):
        assert self.cfg.discrete_dim == 0, "the multi-particle reference covers iVAE-class models only"
        out = particles_elbo(self.p, self.cfg, x.to(self.dtype), eps.to(self.dtype), self.particles, beta,
                             None if y is None else y.to(self.dtype), self.grid, self.analytic)
        if out["loss"].requires_grad:
            out["loss"].backward()
        self.last = out
        return out

    def draw_eps(self, b):
        """P sequential draws on the global CPU generator (P runs of the guide), stacked [p][b]."""
        return torch.cat([torch.empty(b, self.cfg.z_dim).normal_() for _ in range(self.particles)])


class ParticlesOracle(_ParticlesMixin, orc.SVIOracle):
    """SVI.step with Trace_ELBO(num_particles=P)."""


class ParticlesMeanFieldOracle(_ParticlesMixin, mf.MeanFieldOracle):
    """SVI.step with TraceMeanField_ELBO(num_particles=P)."""
    analytic = True
