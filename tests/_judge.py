"""
_judge.py — what "parity with the reference" means for the fp32-class paths, once: the bars, the comparisons of one step's
scalars, z, loc_out and gradients with oracle.svi_oracle, the rule for the parameters after an Adam step, and the loop "two
steps, each from identical parameters" built from them.  tests/test_judge_cpu.py shows that each check sees an error of twice
its bar and pins the constants.

Helper modules are not assertion-rewritten by pytest: every bare assert here carries the tag, the measured value and the bar.
"""
import numpy as np
import pytest
import torch

from _multichannel_cases import round_to_float32

RTOL_ELBO = 2e-5      # loss and s1 (ll) against the reference, relative
RTOL_KL = 1e-4        # s2 (logpz), s3 (logqz), and z_loc / z_scale's rtol
RTOL_GRAD = 1e-4      # every gradient tensor, relative L2, fused 0 / 1 / 2
Z_ATOL = 2e-6         # z_loc / z_scale's atol (an fp32 rounding of values of order 1)
LR = 1e-3             # Adam's step size in every step test, the engine's default
ADAM_BAR = {2: 1e-4, None: 5e-5}      # parameters after Adam, relative L2 over the well-conditioned entries: fused == 2 / else
ILL_REL = 1e-5        # an entry with |g| < ILL_REL max|g| is "near zero": summation noise decides the sign of Adam's first step
ILL_SHARE = 0.01      # ... and such entries must stay below this share of a tensor (the CPU tests confirm it per case table)


def rel_l2(a, b, floor=1e-300):
    """|a - b| / |b| in float64; a zero reference with a zero result gives 0, with anything else a huge number"""
    a, b = a.double().flatten().cpu(), b.double().flatten().cpu()
    return ((a - b).norm() / b.norm().clamp_min(floor)).item()


def state(model):
    return {k: v.detach().cpu() for k, v in model.state_dict().items()}


def reload(model, o, round32=False):
    """The model continues from the reference's parameters, so that every step is compared from an identical state.
    round32: a float64 reference first rounds its own parameters to float32 — both sides continue from the SAME values."""
    if round32:
        round_to_float32(o)
    model.load_state_dict({k: v.detach().float() for k, v in o.p.items()})


@pytest.fixture(autouse=True)
def cpu_threads_16():
    """the float64 references run on 16 threads; the setting is restored for whatever runs next"""
    n = torch.get_num_threads()
    torch.set_num_threads(16)
    try:
        yield
    finally:
        torch.set_num_threads(n)


def h2_grad_tol(rows, kind):
    """The fp16 builds round activations and dL/dpre to ONE 16-bit piece where the rounding errors are independent from row to
    row: what is left in a gradient shrinks with the rows it sums.  At the sizes the launcher selects H231 for (>= 16 384 rows)
    the fp32-class bar holds; forced on toy problems the bar follows 1 / sqrt(rows)."""
    if kind == 28 and rows >= 16384:
        return RTOL_GRAD
    return max(RTOL_GRAD if kind == 28 else (2.5 if kind == 21 else 3.5) * RTOL_GRAD, 0.03 / rows ** 0.5)


# ------------------------------------------------------------------------------- one step against the reference
def check_scalars(s, last, tag, loss_rtol=RTOL_ELBO, atol=0.0, kl_rtol=RTOL_KL, relation=True):
    """The engine's four scalars s against the reference's `last`: loss and s1 to loss_rtol (+ atol), s2 and s3 to kl_rtol;
    relation: s0 == -(s1 + s2 - s3) to 2e-6 among the engine's own."""
    ref = [last[k].item() for k in ("loss", "ll", "logpz", "logqz")]
    print("%s: loss %.6f (ref %.6f) s1 %.6f (ref %.6f) s2 %.6f (ref %.6f) s3 %.6f (ref %.6f)"
          % ((tag,) + tuple(v for pair in zip(s[:4], ref) for v in pair)))
    np.testing.assert_allclose(s[0], ref[0], rtol=loss_rtol, atol=atol, err_msg="%s loss" % tag)
    np.testing.assert_allclose(s[1], ref[1], rtol=loss_rtol, atol=atol, err_msg="%s s1" % tag)
    np.testing.assert_allclose(s[2], ref[2], rtol=kl_rtol, err_msg="%s s2" % tag)
    np.testing.assert_allclose(s[3], ref[3], rtol=kl_rtol, err_msg="%s s3" % tag)
    if relation:
        np.testing.assert_allclose(s[0], -(s[1] + s[2] - s[3]), rtol=2e-6, err_msg="%s loss = -(s1 + s2 - s3)" % tag)


def check_z(zl, zs, last, rtol, atol, tag=""):
    np.testing.assert_allclose(zl.cpu().numpy(), last["z_loc"].detach().numpy(), rtol=rtol, atol=atol, err_msg="%s z_loc" % tag)
    np.testing.assert_allclose(zs.cpu().numpy(), last["z_scale"].detach().numpy(), rtol=rtol, atol=atol, err_msg="%s z_scale" % tag)


def check_loc(loc, o, last, tag, rtol=1e-4, atol=2e-6):
    """loc_out against the decoder's mean, (rows, positions * channels) channel-last; the rate for the Poisson."""
    want = last["loc"].detach()
    if o.cfg.sampler == "poisson_log":
        want = torch.exp(want.clamp(max=30.0))
    want = want.reshape(loc.shape[0], -1).numpy()
    print("%s: loc_out max abs error %.2e" % (tag, np.abs(loc.cpu().numpy() - want).max()))
    np.testing.assert_allclose(loc.cpu().numpy(), want, rtol=rtol, atol=atol, err_msg="%s loc_out" % tag)


def check_grads(eng, o, tag, bar=RTOL_GRAD, skip=(), grads=None):
    """Every gradient tensor of the engine (but `skip`) to `bar` relative L2 of the reference's (o.last_grads, or `grads`)."""
    grads = o.last_grads if grads is None else grads
    errs = {key: rel_l2(eng.grad_of(key), grads[key]) for key in o.p if key not in skip}
    for key in sorted(errs, key=errs.get)[-1:]:              # (none where a user-defined encoder and decoder leave the library no tensor)
        print("%s: worst gradient rel l2 %.2e (%s)" % (tag, errs[key], key))
    for key, err in errs.items():
        assert err < bar, "%s grad %s: rel l2 error %.3e vs the reference (bar %.1e)" % (tag, key, err, bar)


# ------------------------------------------------------------------------------- the parameters after Adam
def near_zero(g):
    """the entries whose gradient is within the summation-order noise of zero: |g| < ILL_REL max|g|"""
    return g.abs() < ILL_REL * g.abs().max()


def near_zero_share(g):
    return near_zero(g).float().mean().item()


def check_params_after_adam(model, o, fused, tag, lr=LR, ill_share=ILL_SHARE):
    """Adam divides by |g|: an entry whose reference gradient is near zero takes a first step of up to lr in a direction that
    summation noise decides.  Such entries are held to Adam's own bound, |dp| <= 2 lr, and their share of a tensor must stay
    below ill_share (None: no cap — conv stacks with dead units have many exactly-zero gradients in the reference itself);
    every other entry to ADAM_BAR relative L2."""
    bar = ADAM_BAR.get(fused, ADAM_BAR[None])
    for key, p in model.state_dict().items():
        ill = near_zero(o.last_grads[key]).reshape(p.shape)
        pc, pr = p.detach().cpu(), o.p[key].detach().float()
        share = ill.float().mean().item()
        assert ill_share is None or share < ill_share, \
            "%s %s: %d near-zero gradient entries, a share of %.3e (bar %.1e)" % (tag, key, int(ill.sum()), share, ill_share)
        if ill.any():
            d = (pc - pr)[ill].abs().max().item()
            assert d <= 2 * lr, "%s %s: a near-zero-gradient entry moved %.3e from the reference (bar 2 lr = %.1e)" % (tag, key, d, 2 * lr)
        err = rel_l2(pc[~ill], pr[~ill])
        assert err < bar, "%s %s after Adam: rel l2 error %.3e (bar %.1e)" % (tag, key, err, bar)


# ------------------------------------------------------------------------------- two steps, each from identical parameters
def steps_vs_reference(eng, model, o, x, y, eps_list, beta, tag, fused, z_atol, atol=0.0, relation=True, checks=(), **outs):
    """One step per eps: loss_and_grads -> o.step -> scalars, z, loc (when outs has loc_out), gradients, then
    checks[i](eng, o, tag) -> adam_step -> check_params_after_adam(fused) -> reload with both sides on the same float32
    values.  `outs` goes to loss_and_grads as it is."""
    xg, yg = x.cuda(), None if y is None else y.cuda()
    zl, zs = (torch.empty(x.shape[0], eps_list[0].shape[1], device="cuda") for _ in range(2))
    for k, eps in enumerate(eps_list):
        t = "%s step %d" % (tag, k)
        eng.loss_and_grads(xg, eps.cuda(), beta, yg, z_out=(zl, zs), **outs)
        o.step(x, eps, beta, y)
        check_scalars(eng.scalars.cpu().numpy(), o.last, t, atol=atol, relation=relation)
        check_z(zl, zs, o.last, RTOL_KL, z_atol, t)
        if "loc_out" in outs:
            check_loc(outs["loc_out"], o, o.last, t)
        check_grads(eng, o, t)
        for check in checks:
            check(eng, o, t)
        eng.adam_step()
        check_params_after_adam(model, o, fused, t)
        reload(model, o, round32=True)
