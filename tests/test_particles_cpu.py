"""
The multi-particle ELBO — SVItrainer(num_particles=P), engine(particles=P), pv_ivae_particles_* — where no GPU is needed:
the reference itself (oracle.svi_oracle with particles=P) against its one-particle path, the trainer's argument handling and
generator order, a two-rank gloo run, and the library's entry points as far as they are host arithmetic.
"""
import ctypes as C
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
from _particles_cases import STEP_CASES, step_case, oracle_of
from _plan_kit import _params, _inputs, _small_plan, _free_port, _plain_loop, _StandInEngine, _ivae, CASES, SLOTS, PLAN_FIELDS

# the KL form of the particle oracle and of its one-particle parent (the ids are the ones these cases have always had)
PAIRS = [pytest.param("sampled", id="ParticlesOracle-SVIOracle"),
         pytest.param("analytic", id="ParticlesMeanFieldOracle-MeanFieldOracle")]


# ------------------------------------------------------------------------------- the reference against its parents
@pytest.mark.parametrize("data_dim,inv,c_dim", CASES)
@pytest.mark.parametrize("kl", PAIRS)
def test_reference_with_one_particle_is_the_parent_oracle(kl, data_dim, inv, c_dim):
    cfg = orc.Config(data_dim=data_dim, latent_dim=2, invariances=inv, c_dim=c_dim)
    p = _params(cfg, c_dim=c_dim)
    x, eps, y = _inputs(cfg, 5, 1, c_dim=c_dim)
    a, b = orc.SVIOracle(p, cfg, dtype=torch.float64, kl=kl, particles=1), orc.SVIOracle(p, cfg, dtype=torch.float64, kl=kl)
    oa, ob = a.loss_and_grads(x, eps, 1.7, y), b.loss_and_grads(x, eps, 1.7, y)
    for k in SLOTS + ("z_loc", "z_scale", "loc"):
        assert torch.equal(oa[k], ob[k]), k
    for k in a.p:
        assert torch.equal(a.p[k].grad, b.p[k].grad), k


@pytest.mark.parametrize("data_dim,inv,c_dim", CASES)
@pytest.mark.parametrize("kl", PAIRS)
def test_reference_with_three_particles_is_the_mean_of_three_parent_evaluations(kl, data_dim, inv, c_dim):
    cfg = orc.Config(data_dim=data_dim, latent_dim=2, invariances=inv, c_dim=c_dim)
    p = _params(cfg, c_dim=c_dim)
    b, P, beta = 5, 3, 1.7
    x, eps, y = _inputs(cfg, b, P, c_dim=c_dim)
    a = orc.SVIOracle(p, cfg, dtype=torch.float64, kl=kl, particles=P)
    oa = a.loss_and_grads(x, eps, beta, y)
    assert abs((oa["loss"] + (oa["ll"] + oa["logpz"] - oa["logqz"])).item()) <= 1e-12 * abs(oa["loss"].item())
    assert oa["z_loc"].shape == (b, cfg.z_dim) and oa["loc"].shape[0] == P * b
    outs, grads = [], []
    for q in range(P):
        o = orc.SVIOracle(p, cfg, dtype=torch.float64, kl=kl)
        outs.append(o.loss_and_grads(x, eps[q * b:(q + 1) * b], beta, y))
        grads.append({k: v.grad for k, v in o.p.items()})
    for k in SLOTS:
        want = sum(o[k] for o in outs) / P
        assert torch.allclose(oa[k], want, rtol=1e-12, atol=0), k
    for q in range(P):                                 # the decoder samples are ordered [p][b]
        assert torch.allclose(oa["loc"][q * b:(q + 1) * b], outs[q]["loc"], rtol=1e-12, atol=1e-300)
    for k in a.p:
        want = sum(g[k] for g in grads) / P
        err = (a.p[k].grad - want).norm().item()
        assert err <= 1e-12 * want.norm().item(), (k, err)


def test_reference_oracles_inherit_adam_and_draw_particles_in_order():
    cfg = orc.Config(data_dim=(8, 8), latent_dim=2, invariances=["r"])
    p = {k: v.float() for k, v in _params(cfg).items()}
    o = orc.SVIOracle(p, cfg, dtype=torch.float32, particles=3)
    torch.manual_seed(4)
    eps = o.draw_eps(5)
    torch.manual_seed(4)
    want = torch.cat([torch.empty(5, cfg.z_dim).normal_() for _ in range(3)])
    assert torch.equal(eps, want)
    x = torch.rand(5, 8, 8)
    o.step(x, eps)
    k = "encoder_z.fc11.weight"
    assert not torch.equal(o.p[k].detach(), p[k]) and float(o.p[k].grad.abs().sum()) == 0.0       # Adam stepped, grads zeroed


# ------------------------------------------------------------------------------- trainer arguments
@pytest.mark.parametrize("loss", [None, "Trace_ELBO", "TraceMeanField_ELBO"])
def test_trainer_hands_the_particle_count_to_the_engine(loss):
    eng = _StandInEngine()
    tr = pv.trainers.SVItrainer(_ivae(), loss=loss, seed=1, engine=eng)
    assert tr.num_particles == 1 and eng.particles == 1
    eng = _StandInEngine()
    tr = pv.trainers.SVItrainer(_ivae(), loss=loss, seed=1, engine=eng, num_particles=4)
    assert tr.num_particles == 4 and eng.particles == 4


@pytest.mark.parametrize("bad", [0, -2, 2.0, "3", None, True])
def test_trainer_rejects_particle_counts_that_are_not_positive_ints(bad):
    with pytest.raises(ValueError, match="num_particles"):
        pv.trainers.SVItrainer(_ivae(), seed=1, engine=_StandInEngine(), num_particles=bad)


@pytest.mark.parametrize("kw", [dict(optimizer=object()), dict(loss=object()), dict(optimizer=object(), loss="Trace_ELBO")])
def test_trainer_sends_pyro_objects_to_their_own_num_particles(kw):
    """With a Pyro optimizer / loss object the count belongs on the Pyro ELBO object: said so, before anything is imported."""
    with pytest.raises(ValueError, match=r"num_particles on the Pyro ELBO object"):
        pv.trainers.SVItrainer(_ivae(), seed=1, num_particles=2, **kw)


@pytest.mark.parametrize("enumerate_parallel", [False, True])
def test_trainer_rejects_particles_for_jivae(enumerate_parallel):
    model = pv.models.jiVAE((8, 8), 2, 3, None, seed=1, device="cpu")
    with pytest.raises(ValueError, match="num_particles"):
        pv.trainers.SVItrainer(model, enumerate_parallel=enumerate_parallel, seed=1, engine=_StandInEngine(), num_particles=2)
    pv.trainers.SVItrainer(model, enumerate_parallel=enumerate_parallel, seed=1, engine=_StandInEngine(), num_particles=1)


def test_engine_rejects_particle_counts_that_are_not_positive_ints():
    from pyroved_amd.engine import _particle_count
    assert _particle_count(1) == 1 and _particle_count(7) == 7
    for bad in (0, -1, 1.0, "2", None, False):
        with pytest.raises(ValueError):
            _particle_count(bad)


# ------------------------------------------------------------------------------- generator order
# z_dim = 3: 6 * 3 = 18 values per draw, no multiple of 16 (CPU normal_ re-draws a short tail: every draw on its own);
# z_dim = 6: 8 * 6 = 48 values, a multiple of 16 (runs of draws are merged), with a ragged last batch of 4 * 6 = 24
@pytest.mark.parametrize("inv,n,batch", [(["r"], 18, 6), (["r", "t", "s"], 20, 8)])
@pytest.mark.parametrize("device_feed", [True, False])
@pytest.mark.parametrize("P", [1, 3])
def test_epoch_consumes_the_generator_as_sequential_particle_draws(inv, n, batch, device_feed, P):
    model = pv.models.iVAE((8, 8), 2, inv, seed=1, device="cpu")
    cfg = orc.Config(data_dim=(8, 8), latent_dim=2, invariances=inv)
    assert (batch * cfg.z_dim) % 16 == (2 if inv == ["r"] else 0)
    x = torch.rand(n, 8, 8, generator=torch.Generator().manual_seed(9))
    loader = pv.utils.init_dataloader(x, batch_size=batch)
    eng = OracleEngine(model, cfg)
    tr = pv.trainers.SVItrainer(model, seed=1, engine=eng, device="cpu", num_particles=P, device_feed=device_feed)
    st0 = torch.get_rng_state()
    tr.step(loader)
    st1 = torch.get_rng_state()
    assert (tr._feed_cache is not None) == device_feed
    torch.set_rng_state(st0)
    want = _plain_loop(loader, cfg.z_dim, P)
    assert torch.equal(torch.get_rng_state(), st1)
    assert len(eng.seen_eps) == len(want) == (n + batch - 1) // batch
    for got, w in zip(eng.seen_eps, want):
        assert got.shape == w.shape and torch.equal(got, w)


# ------------------------------------------------------------------------------- two ranks over gloo
def _dp_run(P, analytic):
    inv = ["r", "t"]
    model = pv.models.iVAE((8, 8), 2, inv, seed=1, device="cpu")
    cfg = orc.Config(data_dim=(8, 8), latent_dim=2, invariances=inv)
    x = torch.rand(10, 8, 8, generator=torch.Generator().manual_seed(5))
    loader = pv.utils.init_dataloader(x, batch_size=5)              # two steps; two ranks take 3 + 2 rows of each
    eng = OracleEngine(model, cfg)                                  # (the trainer hands it kl="analytic" with that loss)
    tr = pv.trainers.SVItrainer(model, loss="TraceMeanField_ELBO" if analytic else None, seed=1, engine=eng, device="cpu",
                                num_particles=P)
    tr.step(loader)
    return tr.loss_history, {k: v.detach().numpy().copy() for k, v in eng.o.p.items()}, eng.adam_t, [e.shape[0] for e in eng.seen_eps]


def _dp_worker(rank, world, port, P, analytic, q):
    import torch.distributed as td
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    torch.set_num_threads(1)
    td.init_process_group("gloo", init_method="tcp://127.0.0.1:%d" % port, rank=rank, world_size=world)
    try:
        q.put((rank,) + _dp_run(P, analytic))
    finally:
        td.destroy_process_group()


@pytest.mark.parametrize("analytic", [False, True])
def test_data_parallel_world2_gloo_with_two_particles_matches_single_process(analytic):
    """Two ranks over gloo, each taking rows [lo, hi) of EVERY particle of every global minibatch, one all-reduce of
    [grads | scalars] per step: after two steps the loss history and the parameters equal the single-process run's, to
    the bars of tests/test_host_cpu.py's data-parallel test (losses 2e-5, parameters 2e-4 of their rms), and the replicas
    stay bit-identical."""
    P, world = 2, 2
    hist1, params1, steps1, rows1 = _dp_run(P, analytic)
    assert steps1 == 2 and rows1 == [P * 5, P * 5]
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_dp_worker, args=(r, world, port, P, analytic, q)) for r in range(world)]
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


# ------------------------------------------------------------------------------- ABI
def test_abi_version_symbols_and_unchanged_plan_struct():
    """The feature arrives as three entry points next to an unchanged v17 plan."""
    lib = _abi.lib()
    assert _abi.PV_ABI_VERSION == 17 and lib.pv_version() == 17
    for name in ("pv_ivae_particles_workspace_bytes", "pv_ivae_particles_loss_and_grads", "pv_ivae_particles_step"):
        assert name in _abi.SIGNATURES and getattr(lib, name) is not None
    src = open(os.path.join(ROOT, "include", "pyroved_amd.h")).read()
    assert "v17, added without a layout change" in src
    assert [f[0] for f in _abi.pv_ivae_plan._fields_] == PLAN_FIELDS


def test_particle_workspace_query_validates_and_forwards():
    lib = _abi.lib()
    for fused in (0, 2, 3):
        p = _small_plan(fused=fused)
        one = lib.pv_ivae_workspace_bytes_for(C.byref(p), 1)
        assert one > 0 and lib.pv_ivae_particles_workspace_bytes(C.byref(p), 1) == one
        two, four = (lib.pv_ivae_particles_workspace_bytes(C.byref(p), n) for n in (2, 4))
        assert one < two < four
        for bad in (0, -1):
            assert lib.pv_ivae_particles_workspace_bytes(C.byref(p), bad) == -1
            assert lib.pv_ivae_particles_loss_and_grads(C.byref(p), bad, 1, None) == -1
            assert lib.pv_ivae_particles_step(C.byref(p), bad, None) == -1
    pj = _small_plan(discrete_dim=3)
    assert lib.pv_ivae_particles_workspace_bytes(C.byref(pj), 1) > 0 and lib.pv_ivae_particles_workspace_bytes(C.byref(pj), 2) == -1
    keep = C.create_string_buffer(64)
    for field in ("row_w", "row_elbo"):
        pw = _small_plan()
        setattr(pw, field, C.addressof(keep))
        assert lib.pv_ivae_particles_workspace_bytes(C.byref(pw), 1) > 0, field
        assert lib.pv_ivae_particles_workspace_bytes(C.byref(pw), 2) == -1, field
        assert lib.pv_ivae_particles_loss_and_grads(C.byref(pw), 2, 1, None) == -1, field
    p1 = _small_plan(fused=1)
    assert lib.pv_ivae_particles_workspace_bytes(C.byref(p1), 2) == -1
    # the calls refuse a plan without buffers before they touch a pointer
    p = _small_plan()
    assert lib.pv_ivae_particles_loss_and_grads(C.byref(p), 2, 1, None) == -1 and lib.pv_ivae_particles_step(C.byref(p), 2, None) == -1


# ------------------------------------------------------------------------------- the GPU step cases' condition
@pytest.mark.parametrize("kl", ["sampled", "analytic"])
def test_gpu_step_cases_keep_near_zero_gradient_entries_below_one_percent(kl):
    """tests/_judge.py's check_params_after_adam holds entries with |g| < 1e-5 max|g| to 2 lr only, on the condition that they
    are fewer than 1 % of a tensor: confirmed here, with the reference alone, for tests/_particles_cases.py's cases and
    seeds over their two steps."""
    for name in sorted(STEP_CASES):
        model, cfg, x, y, eps, b, P = step_case(name, "cpu")
        o = oracle_of(kl, {k: v.detach() for k, v in model.state_dict().items()}, cfg, P)
        for k in range(2):
            o.step(x, eps[k], 1.7, y)
            for key, g in o.last_grads.items():
                share = near_zero_share(g)
                assert share < ILL_SHARE, (name, kl, k, key, share)


# ------------------------------------------------------------------------------- out of scope raises at construction
def test_engine_rejects_what_the_particle_step_does_not_cover():
    """particles > 1 outside the fc-encoder iVAE on fused 0 / 2 / 3 is a ValueError when the engine is made (before it
    binds any device memory) — never another computation."""
    with pytest.raises(ValueError, match="jiVAE"):
        pv.models.jiVAE((8, 8), 2, 3, ["r"], seed=1, device="cpu").engine(particles=2)
    with pytest.raises(ValueError, match="fused = 1"):
        pv.models.iVAE((8, 8), 2, ["r"], seed=1, device="cpu").engine(fused=1, particles=2)
    with pytest.raises(ValueError, match="iVAE only"):
        pv.models.VED((32, 32), (32,), latent_dim=2, seed=1, device="cpu").engine(particles=2)
    with pytest.raises(ValueError, match="particles must be an int"):
        pv.models.iVAE((8, 8), 2, ["r"], seed=1, device="cpu").engine(particles=0)
    # through the trainer the same errors surface at construction
    with pytest.raises(ValueError, match="fused = 1"):
        pv.trainers.SVItrainer(pv.models.iVAE((8, 8), 2, ["r"], seed=1, device="cpu"), num_particles=2, fused=1)
