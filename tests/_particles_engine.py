"""
The CPU stand-in engine of tests/_oracle_engine.py for the multi-particle ELBO: compute is tests/_particles_ref.py's
oracle with the particle count the trainer hands the engine (`engine.particles`), and every `eps` it is handed is
recorded — what the generator-order and data-parallel tests of tests/test_particles_cpu.py look at.
"""
import _particles_ref as pr
from _oracle_engine import OracleEngine


class ParticlesOracleEngine(OracleEngine):
    particles = 1

    def __init__(self, model, cfg, lr=1e-3, analytic=False):
        super().__init__(model, cfg, lr=lr)
        cls = pr.ParticlesMeanFieldOracle if analytic else pr.ParticlesOracle
        self.o = cls(model.state_dict(), cfg, 1, lr=lr, dtype=self.o.dtype)       # (same keys, sizes and flat order)
        self.seen_eps = []

    def loss_and_grads(self, x, eps, beta=1.0, y=None, want_grads=True, **kw):
        self.o.particles = self.particles
        self.seen_eps.append(eps.detach().clone())
        return super().loss_and_grads(x, eps, beta, y, want_grads, **kw)
