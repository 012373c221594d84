"""
The importance-weighted (Renyi / IWAE) bound — SVItrainer(loss="RenyiELBO"), engine(particles=P, renyi=alpha),
pv_ivae_renyi_* — where no GPU is needed: the reference itself (oracle.svi_oracle with renyi=alpha) against its other objectives, the
trainer's argument handling and generator order, a two-rank gloo run, the library's entry points as far as they are host
arithmetic, and the condition tests/test_gpu_renyi.py puts on its inputs.
"""
import ctypes as C
import math
import os
import sys

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

from conftest import ROOT

import pyroved_amd as pv
from pyroved_amd import _abi
from oracle import svi_oracle as orc
from _oracle_engine import OracleEngine
from _judge import ILL_SHARE, near_zero_share
from _particles_cases import STEP_CASES
from _plan_kit import _params, _inputs, _small_plan, _free_port, _plain_loop, _StandInEngine, _ivae, CASES, SLOTS, PLAN_FIELDS
from _renyi_cases import CASES as GPU_CASES, ALPHAS, BETA, case_inputs


def _rel(a, b):
    a, b = (float(v.detach()) if torch.is_tensor(v) else float(v) for v in (a, b))
    return abs(a - b) / max(abs(b), 1e-300)


# ------------------------------------------------------------------------------- 1. one particle is the plain oracle
@pytest.mark.parametrize("alpha", [0.0, 0.5, -1.0])
@pytest.mark.parametrize("data_dim,inv,c_dim", CASES)
def test_reference_with_one_particle_is_the_svi_oracle(data_dim, inv, c_dim, alpha):
    cfg = orc.Config(data_dim=data_dim, latent_dim=2, invariances=inv, c_dim=c_dim)
    p = _params(cfg, c_dim=c_dim)
    x, eps, y = _inputs(cfg, 5, 1, c_dim=c_dim)
    a, b = orc.SVIOracle(p, cfg, dtype=torch.float64, particles=1, renyi=alpha), orc.SVIOracle(p, cfg, dtype=torch.float64)
    oa, ob = a.loss_and_grads(x, eps, 1.7, y), b.loss_and_grads(x, eps, 1.7, y)
    for k in SLOTS + ("z_loc", "z_scale", "loc"):
        assert torch.equal(oa[k], ob[k]), k
    assert torch.equal(oa["weights"], torch.ones(5, dtype=torch.float64))
    for k in a.p:
        assert torch.equal(a.p[k].grad, b.p[k].grad), k


# ------------------------------------------------------------------------------- 2. the gradient is the weighted-sample one
@pytest.mark.parametrize("alpha", [0.0, 0.5, -1.0])
@pytest.mark.parametrize("data_dim,inv,c_dim", CASES)
def test_autograd_of_the_bound_is_autograd_of_the_surrogate_with_its_own_weights(data_dim, inv, c_dim, alpha):
    """grad(-sum_b L_b) = -sum_b sum_p w_pb grad lw_pb with w held constant — what the library's backward computes — to
    1e-12 relative in float64; the surrogate's value sits on the bound too."""
    cfg = orc.Config(data_dim=data_dim, latent_dim=2, invariances=inv, c_dim=c_dim)
    p = _params(cfg, c_dim=c_dim)
    b, P, beta = 5, 3, 1.7
    x, eps, y = _inputs(cfg, b, P, c_dim=c_dim)
    free = orc.SVIOracle(p, cfg, dtype=torch.float64, particles=P, renyi=alpha)
    of = free.loss_and_grads(x, eps, beta, y)
    assert torch.allclose(of["weights"].view(P, b).sum(0), torch.ones(b, dtype=torch.float64), rtol=0, atol=1e-14)
    held = orc.SVIOracle(p, cfg, dtype=torch.float64, particles=P, renyi=alpha)
    held.weights = of["weights"].clone()
    oh = held.loss_and_grads(x, eps, beta, y)
    assert held.weights is None
    for k in SLOTS:
        assert _rel(oh[k], of[k]) <= 1e-12, k
    for k in free.p:
        gf, gh = free.p[k].grad, held.p[k].grad
        assert ((gf - gh).norm() / gf.norm()).item() <= 1e-12, k


# ------------------------------------------------------------------------------- 3. where the bound sits
@pytest.mark.parametrize("data_dim,inv,c_dim", CASES)
def test_bound_dominates_the_elbo_grows_with_alpha_and_meets_the_elbo_at_one(data_dim, inv, c_dim):
    cfg = orc.Config(data_dim=data_dim, latent_dim=2, invariances=inv, c_dim=c_dim)
    p = _params(cfg, c_dim=c_dim)
    b, P, beta = 5, 3, 1.7
    x, eps, y = _inputs(cfg, b, P, c_dim=c_dim)
    with torch.no_grad():
        elbo = orc.SVIOracle(p, cfg, dtype=torch.float64, particles=P).loss_and_grads(x, eps, beta, y)["loss"].item()
        loss = {a: orc.SVIOracle(p, cfg, dtype=torch.float64, particles=P, renyi=a).loss_and_grads(x, eps, beta, y)["loss"].item()
                for a in (-1.0, 0.0, 0.5, 0.9, 1.0 - 1e-6)}
    assert loss[0.0] <= elbo                                  # IWAE bound >= ELBO on the same draws (Jensen)
    seq = [loss[a] for a in (-1.0, 0.0, 0.5, 0.9)]
    assert all(u <= v for u, v in zip(seq, seq[1:])), seq     # the loss is monotone non-decreasing in alpha
    assert seq[-1] <= elbo
    assert _rel(loss[1.0 - 1e-6], elbo) <= 1e-4


# ------------------------------------------------------------------------------- 4. the four slots
@pytest.mark.parametrize("alpha", [0.0, 0.5, -1.0])
@pytest.mark.parametrize("data_dim,inv,c_dim", CASES)
def test_slots_relation_and_what_each_slot_holds(data_dim, inv, c_dim, alpha):
    cfg = orc.Config(data_dim=data_dim, latent_dim=2, invariances=inv, c_dim=c_dim)
    p = _params(cfg, c_dim=c_dim)
    b, P, beta = 5, 3, 1.7
    x, eps, y = _inputs(cfg, b, P, c_dim=c_dim)
    with torch.no_grad():
        o = orc.SVIOracle(p, cfg, dtype=torch.float64, particles=P, renyi=alpha).loss_and_grads(x, eps, beta, y)
    assert abs((o["loss"] + (o["ll"] + o["logpz"] - o["logqz"])).item()) <= 1e-12 * abs(o["loss"].item())
    # s1 = sum_b (sum_p w ll + c_b), c_b = (H(w_b) - log P) / (1 - alpha)
    w, ll = o["weights"].view(P, b), o["ll_per_sample"].view(P, b)
    ent = -(w * o["log_weights"].view(P, b)).sum(0)
    s1 = ((w * ll).sum(0) + (ent - math.log(P)) / (1.0 - alpha)).sum()
    assert _rel(s1, o["ll"]) <= 1e-12


# ------------------------------------------------------------------------------- 5. trainer arguments
def test_trainer_defaults_to_two_particles_and_alpha_zero():
    eng = _StandInEngine()
    tr = pv.trainers.SVItrainer(_ivae(), loss="RenyiELBO", seed=1, engine=eng)
    assert tr.num_particles == 2 and eng.particles == 2 and tr.alpha == 0.0 and eng.renyi == 0.0 and eng.kl == "sampled"
    eng = _StandInEngine()
    tr = pv.trainers.SVItrainer(_ivae(), loss="RenyiELBO", seed=1, engine=eng, num_particles=5, alpha=-0.5)
    assert tr.num_particles == 5 and eng.particles == 5 and eng.renyi == -0.5
    for loss in (None, "Trace_ELBO", "TraceMeanField_ELBO"):         # every other objective: one particle, no order
        eng = _StandInEngine()
        tr = pv.trainers.SVItrainer(_ivae(), loss=loss, seed=1, engine=eng)
        assert tr.num_particles == 1 and tr.alpha is None and eng.renyi is None


@pytest.mark.parametrize("bad", [1, 1.0, float("nan"), float("inf"), "0", None, True])
def test_trainer_rejects_alpha_one_and_what_is_no_finite_float(bad):
    with pytest.raises(ValueError, match="alpha"):
        pv.trainers.SVItrainer(_ivae(), loss="RenyiELBO", seed=1, engine=_StandInEngine(), alpha=bad)


@pytest.mark.parametrize("loss", [None, "Trace_ELBO", "TraceMeanField_ELBO"])
def test_trainer_rejects_alpha_with_another_loss(loss):
    with pytest.raises(ValueError, match="alpha"):
        pv.trainers.SVItrainer(_ivae(), loss=loss, seed=1, engine=_StandInEngine(), alpha=0.0)


@pytest.mark.parametrize("enumerate_parallel", [False, True])
def test_trainer_rejects_the_bound_for_jivae(enumerate_parallel):
    model = pv.models.jiVAE((8, 8), 2, 3, None, seed=1, device="cpu")
    for kw in (dict(), dict(num_particles=1), dict(num_particles=3)):
        with pytest.raises(ValueError, match="RenyiELBO"):
            pv.trainers.SVItrainer(model, loss="RenyiELBO", enumerate_parallel=enumerate_parallel, seed=1, engine=_StandInEngine(),
                                   **kw)


def test_engine_rejects_what_the_bound_does_not_cover():
    from pyroved_amd.engine import _renyi_alpha
    assert _renyi_alpha(None) is None and _renyi_alpha(False) is None and _renyi_alpha(0) == 0.0 and _renyi_alpha(-2.5) == -2.5
    for bad in (1, 1.0, float("nan"), float("-inf"), "0", True):
        with pytest.raises(ValueError, match="renyi"):
            _renyi_alpha(bad)
    ivae = lambda: pv.models.iVAE((8, 8), 2, ["r"], seed=1, device="cpu")
    with pytest.raises(ValueError, match="alpha"):
        ivae().engine(particles=2, renyi=1.0)
    with pytest.raises(ValueError, match="kl='sampled'"):
        ivae().engine(particles=2, renyi=0.0, kl="analytic")
    with pytest.raises(ValueError, match="fused = 1"):
        ivae().engine(fused=1, particles=2, renyi=0.0)
    with pytest.raises(ValueError, match="jiVAE"):
        pv.models.jiVAE((8, 8), 2, 3, ["r"], seed=1, device="cpu").engine(particles=2, renyi=0.0)
    with pytest.raises(ValueError, match="iVAE only"):
        pv.models.VED((32, 32), (32,), latent_dim=2, seed=1, device="cpu").engine(particles=2, renyi=0.0)
    with pytest.raises(TypeError):                                    # (what the parent commit answers to the keyword at all)
        ivae().engine(particles=2, renyi=0.0, no_such_keyword=1)


@pytest.mark.parametrize("inv,n,batch", [(["r"], 18, 6), (["r", "t", "s"], 20, 8)])
@pytest.mark.parametrize("device_feed", [True, False])
def test_epoch_consumes_the_generator_as_the_particle_trainer_does(inv, n, batch, device_feed):
    """The eps draw order is the particle path's: P sequential draws per step (tests/_plan_kit.py's plain loop), and
    the same tensors SVItrainer(num_particles=P) hands its engine."""
    P = 3
    cfg = orc.Config(data_dim=(8, 8), latent_dim=2, invariances=inv)
    x = torch.rand(n, 8, 8, generator=torch.Generator().manual_seed(9))
    loader = pv.utils.init_dataloader(x, batch_size=batch)
    model = pv.models.iVAE((8, 8), 2, inv, seed=1, device="cpu")
    eng = OracleEngine(model, cfg, expect_renyi=True)
    tr = pv.trainers.SVItrainer(model, loss="RenyiELBO", alpha=0.5, seed=1, engine=eng, device="cpu", num_particles=P,
                                device_feed=device_feed)
    st0 = torch.get_rng_state()
    tr.step(loader)
    st1 = torch.get_rng_state()
    torch.set_rng_state(st0)
    want = _plain_loop(loader, cfg.z_dim, P)
    assert torch.equal(torch.get_rng_state(), st1)
    assert len(eng.seen_eps) == len(want) == (n + batch - 1) // batch
    for got, w in zip(eng.seen_eps, want):
        assert got.shape == w.shape and torch.equal(got, w)
    model2 = pv.models.iVAE((8, 8), 2, inv, seed=1, device="cpu")
    eng2 = OracleEngine(model2, cfg)
    tr2 = pv.trainers.SVItrainer(model2, seed=1, engine=eng2, device="cpu", num_particles=P, device_feed=device_feed)
    torch.set_rng_state(st0)
    tr2.step(loader)
    assert torch.equal(torch.get_rng_state(), st1)
    for got, w in zip(eng.seen_eps, eng2.seen_eps):
        assert torch.equal(got, w)
    assert tr.loss_history["training_loss"][0] < tr2.loss_history["training_loss"][0]     # (the bound, not the ELBO)


# ------------------------------------------------------------------------------- 6. two ranks over gloo
def _dp_run(P, alpha):
    inv = ["r", "t"]
    model = pv.models.iVAE((8, 8), 2, inv, seed=1, device="cpu")
    cfg = orc.Config(data_dim=(8, 8), latent_dim=2, invariances=inv)
    x = torch.rand(10, 8, 8, generator=torch.Generator().manual_seed(5))
    loader = pv.utils.init_dataloader(x, batch_size=5)              # two steps; two ranks take 3 + 2 rows of each
    eng = OracleEngine(model, cfg, expect_renyi=True)
    tr = pv.trainers.SVItrainer(model, loss="RenyiELBO", alpha=alpha, seed=1, engine=eng, device="cpu", num_particles=P)
    tr.step(loader)
    return tr.loss_history, {k: v.detach().numpy().copy() for k, v in eng.o.p.items()}, eng.adam_t, [e.shape[0] for e in eng.seen_eps]


def _dp_worker(rank, world, port, P, alpha, q):
    import torch.distributed as td
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    torch.set_num_threads(1)
    td.init_process_group("gloo", init_method="tcp://127.0.0.1:%d" % port, rank=rank, world_size=world)
    try:
        q.put((rank,) + _dp_run(P, alpha))
    finally:
        td.destroy_process_group()


def test_data_parallel_world2_gloo_matches_single_process():
    """Two ranks over gloo, each taking rows [lo, hi) of EVERY particle of every global minibatch, one all-reduce of
    [grads | scalars] per step: the bound is a sum over images, so the shards add up to the single-process run — loss
    history to 2e-5, parameters to 2e-4 of their rms (tests/test_host_cpu.py's data-parallel bars), replicas bit-identical."""
    P, world, alpha = 3, 2, 0.5
    hist1, params1, steps1, rows1 = _dp_run(P, alpha)
    assert steps1 == 2 and rows1 == [P * 5, P * 5]
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_dp_worker, args=(r, world, port, P, alpha, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = [q.get(timeout=300) for _ in range(world)]
    for p in procs:
        p.join(60)
        assert p.exitcode == 0
    res.sort(key=lambda t: t[0])
    assert res[0][4] == [P * 3, P * 3] and res[1][4] == [P * 2, P * 2]
    for rank, hist, params, steps, _ in res:
        assert steps == 2
        np.testing.assert_allclose(hist["training_loss"], hist1["training_loss"], rtol=2e-5)
        for key, v in params.items():
            rms = float(np.sqrt(np.mean(params1[key].astype(np.float64) ** 2)))
            np.testing.assert_allclose(v, params1[key], rtol=2e-4, atol=max(1e-7, 2e-4 * rms), err_msg="%s rank %d" % (key, rank))
    for key in res[0][2]:
        assert np.array_equal(res[0][2][key], res[1][2][key]), key


# ------------------------------------------------------------------------------- 7. ABI
RENYI_SYMBOLS = ("pv_ivae_renyi_workspace_bytes", "pv_ivae_renyi_loss_and_grads", "pv_ivae_renyi_step")


def test_abi_version_symbols_and_unchanged_plan_struct():
    """The feature arrives as three entry points next to an unchanged v17 plan."""
    lib = _abi.lib()
    assert _abi.PV_ABI_VERSION == 17 and lib.pv_version() == 17
    for name in RENYI_SYMBOLS:
        assert name in _abi.SIGNATURES and getattr(lib, name) is not None
    src = open(os.path.join(ROOT, "include", "pyroved_amd.h")).read()
    assert src.count("v17, added without a layout change") == 2
    for name in RENYI_SYMBOLS:
        assert name in src
    assert [f[0] for f in _abi.pv_ivae_plan._fields_] == PLAN_FIELDS


def test_renyi_workspace_query_validates_and_forwards():
    lib = _abi.lib()
    ws, lg, st = (getattr(lib, n) for n in RENYI_SYMBOLS)
    for fused in (0, 2, 3):
        p = _small_plan(fused=fused)
        one = lib.pv_ivae_workspace_bytes_for(C.byref(p), 1)
        assert one > 0 and ws(C.byref(p), 1) == one
        two, four = (ws(C.byref(p), n) for n in (2, 4))
        assert one < two < four
        assert two >= lib.pv_ivae_particles_workspace_bytes(C.byref(p), 2)        # (the particle layout plus c_b)
        assert ws(C.byref(p), 1024) > four                                        # the documented cap: 1024 particles
        for bad in (0, -1, 1025):
            assert ws(C.byref(p), bad) == -1
            assert lg(C.byref(p), bad, 0.0, 1, None, None) == -1
            assert st(C.byref(p), bad, 0.0, None, None) == -1
        for bad in (1.0, float("nan"), float("inf"), float("-inf")):
            for P in (1, 2):
                assert lg(C.byref(p), P, bad, 1, None, None) == -1, (bad, P)
                assert st(C.byref(p), P, bad, None, None) == -1, (bad, P)
    keep = C.create_string_buffer(64)
    pj = _small_plan(discrete_dim=3)
    p1 = _small_plan(fused=1)
    pa = _small_plan()
    pa.kl_mode = _abi.KL["analytic"]
    refused = [("jiVAE", pj), ("fused=1", p1), ("analytic", pa)]
    for field in ("row_w", "row_elbo"):
        pw = _small_plan()
        setattr(pw, field, C.addressof(keep))
        refused.append((field, pw))
    for what, q in refused:
        for P in (1, 2):
            assert ws(C.byref(q), P) == -1, (what, P)
            assert lg(C.byref(q), P, 0.0, 1, None, None) == -1, (what, P)
            assert st(C.byref(q), P, 0.0, None, None) == -1, (what, P)
    # the calls refuse a plan without buffers before they touch a pointer (weights_out included)
    p = _small_plan()
    for P in (1, 2):
        assert lg(C.byref(p), P, 0.0, 1, C.addressof(keep), None) == -1 and st(C.byref(p), P, 0.5, C.addressof(keep), None) == -1


# ------------------------------------------------------------------------------- 8. the GPU cases' condition
def test_gpu_cases_have_spread_weights_and_a_bound_away_from_the_elbo():
    """A test whose weights collapse onto one particle shows nothing about the weighting.  With the reference alone, for
    every case of tests/_renyi_cases.py and each alpha it uses: at least one image has effective sample size
    1 / sum_p w^2 >= 1.9, and bound - ELBO summed over the batch exceeds 0.25 nats.  And the condition of
    check_params_after_adam (tests/_judge.py) on the step cases: entries with |g| < 1e-5 max|g| stay below 1 % of
    every tensor over the two steps."""
    for name in sorted(GPU_CASES):
        cfg, params, x, y, eps, b, P, beta, _ = case_inputs(name, "cpu")
        assert beta == BETA
        for alpha in (ALPHAS if name != "28x28_r_b128_p2" else (0.0,)):
            with torch.no_grad():
                o = orc.SVIOracle(params, cfg, dtype=torch.float64, particles=P, renyi=alpha).loss_and_grads(x, eps[0], beta, y)
                e = orc.SVIOracle(params, cfg, dtype=torch.float64, particles=P).loss_and_grads(x, eps[0], beta, y)
            ess = (1.0 / (o["weights"].view(P, b) ** 2).sum(0)).max().item()
            gap = e["loss"].item() - o["loss"].item()
            print("%s alpha=%g: max ESS %.3f, bound - ELBO %.3f nats" % (name, alpha, ess, gap))
            assert ess >= 1.9, (name, alpha, ess)
            assert gap > 0.25, (name, alpha, gap)
            if name not in STEP_CASES:
                continue
            o = orc.SVIOracle(params, cfg, dtype=torch.float64, particles=P, renyi=alpha)
            for k in range(2):
                o.step(x, eps[k], beta, y)
                for key, g in o.last_grads.items():
                    share = near_zero_share(g)
                    assert share < ILL_SHARE, (name, alpha, k, key, share)
