"""
The opt-in fused f32 decoder kernel for multi-channel models — PV_PLAN_FUSED_CHANNELS in the C ABI, fused_channels= in Python —
where no GPU is needed: the flag's value, which plans it takes effect for (through pv_ivae_uses_fused and the workspace
queries: host arithmetic), that it does nothing everywhere else, and what the engine and the trainer build and refuse.
Plans are tests/_plan_kit.py's: 784 positions x ch observations, batch 16.
"""
import ctypes as C
import os
import re

import pytest

from conftest import ROOT

import pyroved_amd as pv
from pyroved_amd import _abi
from _plan_kit import _plan, _vanilla_plan

EINVAL = -1
FLAG = 256


def flagged(fused=1, channels=2):
    p = _plan(fused, channels)
    p.flags |= FLAG
    return p


def sizes(p):
    lib = _abi.lib()
    return [lib.pv_ivae_workspace_bytes_for(C.byref(p), w) for w in range(4)]


def test_flag_value_and_unchanged_abi():
    src = open(os.path.join(ROOT, "include", "pyroved_amd.h")).read()
    m = re.search(r"#define\s+PV_PLAN_FUSED_CHANNELS\s+(\d+)", src)
    assert m and int(m.group(1)) == FLAG == _abi.PV_PLAN_FUSED_CHANNELS
    assert _abi.PV_ABI_VERSION == 17 and _abi.lib().pv_version() == 17 and C.sizeof(_abi.pv_ivae_plan) == 2824


@pytest.mark.parametrize("ch", range(2, 9))
def test_flagged_plan_runs_fused(ch):
    """fused = 1 + the flag, 2 .. 8 channels: the fused kernel, its (smaller) step layout, decode and encode layouts."""
    lib = _abi.lib()
    p = flagged(1, ch)
    assert lib.pv_ivae_uses_fused(C.byref(p)) == 1
    all_, step, enc, dec = sizes(p)
    layered = lib.pv_ivae_workspace_bytes_for(C.byref(_plan(0, ch)), 1)
    assert 0 < step < layered                     # no per-row activations
    assert enc > 0 and dec > 0 and all_ >= max(step, enc, dec)
    # decode on the fused kernel too: no (rows x 128) activations in its layout either
    assert dec < lib.pv_ivae_workspace_bytes_for(C.byref(_plan(0, ch)), 3)


def test_flag_does_nothing_elsewhere():
    """uses_fused and every workspace size are those of the same plan without the flag."""
    lib = _abi.lib()

    def same(p, want_fused):
        q = type(p).from_buffer_copy(p)
        q.flags &= ~FLAG
        assert p.flags & FLAG
        assert lib.pv_ivae_uses_fused(C.byref(p)) == lib.pv_ivae_uses_fused(C.byref(q)) == want_fused
        assert sizes(p) == sizes(q) and sizes(q)[0] > 0

    for ch in (2, 3, 8):
        for fused in (0, 2, 3):
            same(flagged(fused, ch), 0)
    for fused, want in ((0, 0), (1, 1), (2, 1), (3, 1)):                # one channel: today's plan, fused or not
        same(flagged(fused, 1), want)
    p = flagged(1, 3)                                                   # 63 positions (7 x 9): not a multiple of 16
    p.n_pix = 63 * 3
    p.enc[0].in_dim = 63 * 3
    same(p, 0)
    p = flagged(1, 2)                                                   # a 72 / 40 decoder
    p.fc_coord.out_dim = p.fc_latent.out_dim = p.dec[0].in_dim = 72
    p.dec[0].out_dim = p.dec[1].in_dim = 40
    same(p, 0)
    p = flagged(1, 2)                                                   # softplus
    p.dec[0].act = p.dec[1].act = _abi.ACT["softplus"]
    same(p, 0)
    p = _vanilla_plan(1)
    p.flags |= FLAG
    same(p, 0)


def test_one_channel_flagged_is_the_parent_commits_fused_plan():
    """fused = 1, one channel, with and without the flag: the same four sizes."""
    assert sizes(flagged(1, 1)) == sizes(_plan(1, 1))
    assert _abi.lib().pv_ivae_uses_fused(C.byref(flagged(1, 1))) == 1


def test_other_objectives_and_missing_buffers_are_refused():
    lib = _abi.lib()
    for ch in (2, 5, 8):
        p = flagged(1, ch)
        assert lib.pv_ivae_particles_workspace_bytes(C.byref(p), 3) == EINVAL
        assert lib.pv_ivae_renyi_workspace_bytes(C.byref(p), 3) == EINVAL
        assert lib.pv_ivae_loss_and_grads(C.byref(p), 1, None) == EINVAL          # no buffers: refused before any pointer
        assert lib.pv_ivae_step(C.byref(p), None) == EINVAL


# ------------------------------------------------------------------------------- Python: engine and trainer
def model(channels=2, **kw):
    return pv.models.iVAE((8, 8), 2, ["r", "t", "s"], channels=channels, seed=1, device="cpu", **kw)


def test_refusals_name_the_keyword():
    with pytest.raises(ValueError, match="fused_channels"):
        pv.trainers.SVItrainer(model(), fused_channels=True, num_particles=3)
    with pytest.raises(ValueError, match="fused_channels"):
        pv.trainers.SVItrainer(model(), loss="RenyiELBO", fused_channels=True)
    with pytest.raises(ValueError, match="fused_channels"):
        pv.trainers.SVItrainer(model(), fused_channels=True, fused=3)
    with pytest.raises(ValueError, match="fused_channels"):
        pv.trainers.SVItrainer(model(), fused_channels=True, precision="bf16")
    with pytest.raises(ValueError, match="fused_channels"):
        pv.trainers.SVItrainer(model(), fused_channels=True, fused=0)
    for kw in (dict(particles=3), dict(particles=3, renyi=0.0), dict(fused=3), dict(fused=0)):
        m = model()
        with pytest.raises(ValueError, match="fused_channels"):
            m.engine(fused_channels=True, **kw)
        assert m._engine is None                                       # raised before anything was bound


@pytest.fixture
def unbound(monkeypatch):
    """Engines here never reach the device: bind() (flat buffers on a HIP device; it refuses a CPU model) is stubbed, everything
    in front of it — the model and keyword checks — and the plan's `fused` / `flags` values behind it are the engine's own.
    (The whole plan struct of a bound engine is compared on the GPU: tests/test_gpu_multichannel_fused.py.)"""
    from pyroved_amd.engine import IVAEEngine
    monkeypatch.setattr(IVAEEngine, "bind", lambda self: None)


def bits(eng):
    return eng._plan_fused(), eng._plan_flags()


def test_configure_rolls_back(unbound):
    m = model()
    eng = m.engine(fused_channels=True)
    assert eng.fused_channels is True and bits(eng) == (1, FLAG)
    with pytest.raises(ValueError, match="fused_channels"):
        eng.configure(fused=0)
    assert eng.fused == 2 and eng.fused_channels is True
    with pytest.raises(ValueError, match="fused_channels"):
        eng.configure(particles=2)
    assert eng.particles == 1 and eng.fused_channels is True
    eng.configure(fused_channels=False)
    assert bits(eng) == (2, 0)
    eng.configure(fused=0)
    with pytest.raises(ValueError, match="fused_channels"):
        eng.configure(fused_channels=True)
    assert eng.fused_channels is False and eng.fused == 0


def test_engine_plan_bits(unbound):
    """C > 1: fused 1 or 2 + the keyword -> plan.fused = 1 with the flag; supports_dp_step stays False; without the keyword, and
    with one channel, the plan's bits are what they were."""
    for fused in (1, 2):
        eng = model(3).engine(fused=fused, fused_channels=True)
        assert bits(eng) == (1, FLAG) and eng.supports_dp_step is False
        assert bits(model(3).engine(fused=fused)) == (fused, 0)
    for fused in (1, 2):
        assert bits(model(1).engine(fused=fused, fused_channels=True)) == bits(model(1).engine(fused=fused)) == (fused, 0)


def test_trainer_keyword(unbound):
    m = model()
    tr = pv.trainers.SVItrainer(m, fused_channels=True)
    assert tr.engine.fused_channels is True and bits(tr.engine) == (1, FLAG)
    tr = pv.trainers.SVItrainer(m)                                      # a later trainer without the keyword: back to the default
    assert tr.engine.fused_channels is False and bits(tr.engine) == (2, 0)
