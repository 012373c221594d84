"""
The judge of the GPU objective tests (tests/_judge.py) judged: on one small case with the reference alone — iVAE (8, 8) `rts`,
B = 6, seed 1, two steps, float64 oracle — a stand-in engine serves scalars, gradients and a model state taken from the oracle's
own results.  Every check passes on the exact values and with every checked quantity half a bar off; each raises when exactly
one thing is two bars off.  The bars themselves are pinned.
"""
import types

import numpy as np
import pytest
import torch

from conftest import make_x

import pyroved_amd as pv
from oracle import svi_oracle as orc
import _judge as J

KEYS = ("loss", "ll", "logpz", "logqz")


class _Engine:
    def __init__(self, scalars, grads):
        self.scalars, self.grads = np.array(scalars, dtype=np.float64), grads

    def grad_of(self, key):
        return self.grads[key]


class _Model:
    def __init__(self, sd):
        self.sd = sd

    def state_dict(self):
        return self.sd


@pytest.fixture(scope="module")
def case():
    """(the oracle after its second step, exact scalars, exact float32 parameters after Adam)"""
    data_dim, inv, b = (8, 8), ["r", "t", "s"], 6
    model = pv.models.iVAE(data_dim, 2, inv, seed=1, device="cpu")
    cfg = orc.Config(data_dim=data_dim, latent_dim=2, invariances=inv)
    o = orc.SVIOracle(J.state(model), cfg, lr=J.LR, dtype=torch.float64)
    x = make_x("rand", b, data_dim)
    g = torch.Generator().manual_seed(1)
    for _ in range(2):
        J.round_to_float32(o)
        o.step(x, torch.randn(b, cfg.z_dim, generator=g))
    assert all(J.near_zero_share(v) < J.ILL_SHARE for v in o.last_grads.values())      # the case meets the rule's condition
    return o, [o.last[k].item() for k in KEYS], {k: v.detach().float().clone() for k, v in o.p.items()}


def _grads(o, scale_err=0.0, only=None):
    """the reference's gradients, each (or `only`) moved by scale_err of its own norm along a fixed random direction"""
    g = torch.Generator().manual_seed(3)
    out = {}
    for k, v in o.last_grads.items():
        u = torch.randn(v.shape, generator=g, dtype=torch.float64)
        out[k] = v + (scale_err if only in (None, k) else 0.0) * v.norm() * u / u.norm()
    return out


def _z(o, f):
    """z_loc, z_scale with every entry f bars (atol + rtol |ref|) off"""
    return [o.last[k].detach() + f * (J.Z_ATOL + J.RTOL_KL * o.last[k].detach().abs()) for k in ("z_loc", "z_scale")]


def _moved(params, key, index, delta):
    sd = {k: v.clone() for k, v in params.items()}
    sd[key].view(-1)[index] += delta
    return _Model(sd)


def _well_conditioned(o, key):
    ill = J.near_zero(o.last_grads[key]).reshape(-1)
    return int((~ill).nonzero()[0]), o.p[key].detach().float().reshape(-1)[~ill].norm().item()


# ------------------------------------------------------------------------------- the bars
def test_constants_are_the_projects_bars():
    assert (J.RTOL_ELBO, J.RTOL_KL, J.RTOL_GRAD, J.Z_ATOL, J.LR) == (2e-5, 1e-4, 1e-4, 2e-6, 1e-3)
    assert J.ADAM_BAR == {2: 1e-4, None: 5e-5} and (J.ILL_REL, J.ILL_SHARE) == (1e-5, 0.01)


def test_rel_l2_floor():
    zero = torch.zeros(4)
    assert J.rel_l2(zero, zero) == 0.0
    assert J.rel_l2(torch.full((4,), 1e-35, dtype=torch.float64), zero) > 1.0         # the floor is below 1e-35
    assert J.rel_l2(torch.tensor([1.0, 2.0]), torch.tensor([1.0, 2.0])) == 0.0
    np.testing.assert_allclose(J.rel_l2(torch.tensor([3.0, 0.0]), torch.tensor([0.0, 4.0])), 1.25)


# ------------------------------------------------------------------------------- passes
def test_exact_values_pass(case):
    o, s, params = case
    J.check_scalars(np.array(s), o.last, "exact")
    J.check_z(*_z(o, 0.0), o.last, J.RTOL_KL, J.Z_ATOL, "exact")
    J.check_grads(_Engine(s, _grads(o)), o, "exact")
    for fused in (0, 2):
        J.check_params_after_adam(_Model(params), o, fused, "exact")


def test_half_a_bar_off_passes(case):
    o, s, params = case
    half = [s[0] * (1 + 0.5 * J.RTOL_ELBO), s[1] * (1 - 0.5 * J.RTOL_ELBO), s[2] * (1 + 0.5 * J.RTOL_KL), s[3] * (1 - 0.5 * J.RTOL_KL)]
    J.check_scalars(np.array(half), o.last, "half", relation=False)
    s0 = -(s[1] + s[2] - s[3])
    J.check_scalars(np.array([s0 * (1 + 1e-6)] + s[1:]), o.last, "half the relation's bar")
    J.check_z(*_z(o, 0.5), o.last, J.RTOL_KL, J.Z_ATOL, "half")
    J.check_grads(_Engine(s, _grads(o, 0.5 * J.RTOL_GRAD)), o, "half")
    for fused in (0, 2):
        for key in o.p:
            i, norm = _well_conditioned(o, key)
            J.check_params_after_adam(_moved(params, key, i, 0.5 * J.ADAM_BAR.get(fused, J.ADAM_BAR[None]) * norm), o, fused, "half")


# ------------------------------------------------------------------------------- exactly one thing two bars off
def test_loss_two_bars_off_raises(case):
    o, s, _ = case
    with pytest.raises(AssertionError, match="two loss"):
        J.check_scalars(np.array([s[0] * (1 + 2 * J.RTOL_ELBO)] + s[1:]), o.last, "two", relation=False)
    with pytest.raises(AssertionError, match="two s1"):
        J.check_scalars(np.array([s[0], s[1] * (1 + 2 * J.RTOL_ELBO)] + s[2:]), o.last, "two", relation=False)


def test_kl_slot_two_bars_off_raises(case):
    o, s, _ = case
    with pytest.raises(AssertionError, match="two s2"):
        J.check_scalars(np.array(s[:2] + [s[2] * (1 + 2 * J.RTOL_KL), s[3]]), o.last, "two", relation=False)
    with pytest.raises(AssertionError, match="two s3"):
        J.check_scalars(np.array(s[:3] + [s[3] * (1 + 2 * J.RTOL_KL)]), o.last, "two", relation=False)


def test_broken_slots_relation_raises(case):
    o, s, _ = case
    off = np.array([-(s[1] + s[2] - s[3]) * (1 + 4e-6)] + s[1:])
    with pytest.raises(AssertionError, match=r"loss = -\(s1 \+ s2 - s3\)"):
        J.check_scalars(off, o.last, "two")
    J.check_scalars(off, o.last, "two", relation=False)                                # (within the loss bar: only the relation sees it)


def test_z_two_bars_off_raises(case):
    o, _, _ = case
    for which in (0, 1):
        z = _z(o, 0.0)
        z[which].view(-1)[7] = _z(o, 2.0)[which].view(-1)[7]                           # one entry
        with pytest.raises(AssertionError, match="two z_" + ("loc", "scale")[which]):
            J.check_z(*z, o.last, J.RTOL_KL, J.Z_ATOL, "two")


def test_one_gradient_tensor_two_bars_off_raises(case):
    o, s, _ = case
    smallest = min(o.last_grads, key=lambda k: o.last_grads[k].norm().item())
    with pytest.raises(AssertionError, match="two grad %s: rel l2 error 2.000e-04" % smallest):
        J.check_grads(_Engine(s, _grads(o, 2 * J.RTOL_GRAD, only=smallest)), o, "two")
    J.check_grads(_Engine(s, _grads(o, 2 * J.RTOL_GRAD, only=smallest)), o, "two", skip=(smallest,))
    J.check_grads(_Engine(s, _grads(o, 2 * J.RTOL_GRAD, only=smallest)), o, "two", bar=3 * J.RTOL_GRAD)


@pytest.mark.parametrize("fused", [0, 2])
def test_one_well_conditioned_parameter_entry_two_bars_off_raises(case, fused):
    o, _, params = case
    key = "decoder.fc_layers.0.weight"
    i, norm = _well_conditioned(o, key)
    with pytest.raises(AssertionError, match="two %s after Adam" % key):
        J.check_params_after_adam(_moved(params, key, i, 2 * J.ADAM_BAR.get(fused, J.ADAM_BAR[None]) * norm), o, fused, "two")


def _with_zeroed_gradient_entries(o, key, n):
    """a stand-in for the oracle whose reference gradient `key` has its first n entries exactly zero"""
    grads = {k: v.clone() for k, v in o.last_grads.items()}
    grads[key].view(-1)[:n] = 0.0
    return types.SimpleNamespace(p=o.p, last_grads=grads)


def test_near_zero_gradient_entry_is_held_to_two_lr(case):
    o, _, params = case
    key = "decoder.fc_layers.0.weight"                                                # 128 x 128: one entry is 0.006 %
    held = _with_zeroed_gradient_entries(o, key, 1)
    # far beyond the well-conditioned entries' bar, yet within Adam's own bound: passes
    J.check_params_after_adam(_moved(params, key, 0, 1.0 * J.LR), held, 0, "one lr")
    with pytest.raises(AssertionError, match="three lr %s: a near-zero-gradient entry moved" % key):
        J.check_params_after_adam(_moved(params, key, 0, 3.0 * J.LR), held, 0, "three lr")
    with pytest.raises(AssertionError, match="after Adam"):                            # the same move on a well-conditioned entry
        J.check_params_after_adam(_moved(params, key, 0, 1.0 * J.LR), o, 0, "one lr")


def test_too_many_near_zero_gradient_entries_raise(case):
    o, _, params = case
    key = "decoder.fc_layers.0.weight"
    n = o.last_grads[key].numel() // 50                                                # 2 %
    many = _with_zeroed_gradient_entries(o, key, n)
    assert 0.02 <= J.near_zero_share(many.last_grads[key]) < 0.021
    with pytest.raises(AssertionError, match="near-zero gradient entries"):
        J.check_params_after_adam(_Model(params), many, 0, "2 %")
    J.check_params_after_adam(_Model(params), many, 0, "2 %, no cap", ill_share=None)
