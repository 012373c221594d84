"""
_meanfield_ref.py — the reference of the analytic-KL (mean-field) objective the tests of
SVItrainer(loss="TraceMeanField_ELBO") / engine(kl="analytic") compare against.

What it restates: pyro.infer.TraceMeanField_ELBO on iVAE.guide / iVAE.model (and VED's).  The `latent` sites of guide
and model are both Normal, so that objective takes kl_divergence(guide site, model site) instead of the sampled
log q(z|x) - log p(z), under the same poutine.scale(beta); z = mu + sigma * eps is still drawn once per sample for the
likelihood:

    loss = -sum_b log p(x_b | z_b) + beta * sum_b sum_i KL(N(mu_bi, sigma_bi) || N(0, 1))

Pyro is not a dependency of this repository and is not run here: the pin is torch.distributions.kl_divergence (the
function Pyro's objective calls), the same way oracle/svi_oracle.py pins Trace_ELBO to torch's Normal.log_prob.

The oracles subclass oracle.svi_oracle.SVIOracle / VedOracle and override only the loss; Adam, zero_grads and the epoch
loops are inherited.  The four scalars keep the sampled objective's slots and relation loss = -(ll + logpz - logqz), with
logpz / logqz the analytic expectations of the terms they hold there (logqz - logpz = beta * KL).
"""
import math

import torch
import torch.distributions as td

from oracle import svi_oracle as orc

LOG_SQRT_2PI = 0.5 * math.log(2.0 * math.pi)


def _kl_and_slots(z_loc, z_scale, beta):
    kl = td.kl_divergence(td.Normal(z_loc, z_scale), td.Normal(torch.zeros_like(z_loc), torch.ones_like(z_scale))).sum(-1)
    # E_q log p(z), E_q log q(z|x): the slots' analytic expectations
    e_logp = (-(z_loc ** 2 + z_scale ** 2) / 2 - LOG_SQRT_2PI).sum(-1)
    e_logq = (-0.5 - torch.log(z_scale) - LOG_SQRT_2PI).sum(-1)
    return kl, (beta * e_logp).sum(), (beta * e_logq).sum()


def meanfield_elbo(p, cfg, x, eps, beta=1.0, y=None, grid=None):
    b = x.shape[0]
    z_loc, z_scale = orc._encode_any(p, cfg, x, y)
    z = z_loc + z_scale * eps
    kl, t_lp, t_lq = _kl_and_slots(z_loc, z_scale, beta)
    loc, xc = orc.decode_from_latent(p, cfg, z, y, grid)
    ll = orc.likelihood(cfg, loc.reshape(b, -1)).log_prob(x.reshape(b, -1)).sum(-1)
    t_ll = ll.sum()
    loss = -t_ll + (beta * kl).sum()
    return dict(loss=loss, ll=t_ll, logpz=t_lp, logqz=t_lq, kl=kl, z_loc=z_loc, z_scale=z_scale, z=z, loc=loc,
                x_coord_prime=xc, ll_per_sample=ll)


def meanfield_ved_elbo(p, cfg, x, y, eps, beta=1.0, bufs=None, training=True, decisions=None):
    b = x.shape[0]
    z_loc, z_scale = orc.conv_encoder_forward(p, cfg, x, bufs, training, decisions)
    z = z_loc + z_scale * eps
    kl, t_lp, t_lq = _kl_and_slots(z_loc, z_scale, beta)
    loc = orc.conv_decoder_forward(p, cfg, z, bufs, training)
    ll = orc.likelihood(cfg, loc.flatten(1)).log_prob(y.reshape(b, -1)).sum(-1)
    t_ll = ll.sum()
    return dict(loss=-t_ll + (beta * kl).sum(), ll=t_ll, logpz=t_lp, logqz=t_lq, kl=kl, z_loc=z_loc, z_scale=z_scale, z=z,
                loc=loc)


class MeanFieldOracle(orc.SVIOracle):
    """SVI.step with TraceMeanField_ELBO for iVAE-class models (no discrete latent)."""

    def loss_and_grads(self, x, eps, beta=1.0, y=None):
        assert self.cfg.discrete_dim == 0, "the mean-field objective is not defined for jiVAE"
        out = meanfield_elbo(self.p, self.cfg, x.to(self.dtype), eps.to(self.dtype), beta,
                             None if y is None else y.to(self.dtype), self.grid)
        if out["loss"].requires_grad:
            out["loss"].backward()
        self.last = out
        return out


class MeanFieldVedOracle(orc.VedOracle):
    """SVI.step with TraceMeanField_ELBO for VED."""

    def step(self, x, y, eps, beta=1.0) -> float:
        out = meanfield_ved_elbo(self.p, self.cfg, x.to(self.dtype), y.to(self.dtype), eps.to(self.dtype), beta, self.bufs,
                                 self.training)
        if out["loss"].requires_grad:
            out["loss"].backward()
        self.last = out
        self.last_grads = {k: (None if v.grad is None else v.grad.detach().clone()) for k, v in self.p.items()}
        if any(v.grad is not None for v in self.p.values()):
            self.opt.step()
        for v in self.p.values():
            if v.grad is not None:
                v.grad = torch.zeros_like(v.grad)
        return out["loss"].item()
