"""
The CPU stand-in engine of tests/_oracle_engine.py for the importance-weighted bound: compute is tests/_renyi_ref.py's
oracle with the particle count and the order the trainer hands the engine (`engine.particles`, `engine.renyi`), and
every `eps` it is handed is recorded — what the generator-order and data-parallel tests of tests/test_renyi_cpu.py look at.
"""
import _renyi_ref as rr
from _oracle_engine import OracleEngine


class RenyiOracleEngine(OracleEngine):
    particles = 1
    renyi = None

    def __init__(self, model, cfg, lr=1e-3):
        super().__init__(model, cfg, lr=lr)
        self.o = rr.RenyiOracle(model.state_dict(), cfg, 1, 0.0, lr=lr, dtype=self.o.dtype)   # (same keys, sizes and flat order)
        self.seen_eps = []

    def loss_and_grads(self, x, eps, beta=1.0, y=None, want_grads=True, **kw):
        assert self.renyi is not None, "the trainer did not hand the engine the bound's order"
        self.o.particles, self.o.alpha = self.particles, float(self.renyi)
        self.seen_eps.append(eps.detach().clone())
        return super().loss_and_grads(x, eps, beta, y, want_grads, **kw)
