"""
The engines' settings rules against a recorded table (tests/golden/engine_settings.json, made by
tests/golden/make_engine_settings.py on the commit before the rules became one list; cases: tests/_engine_settings_cases.py).
Every combination of the settings on eight iVAE-like models through model.engine(**kw), the semi-supervised and VED engines on a
smaller cross, and every single change through engine.configure(**kw) from every accepted state of three models: accepted and
what the plan then carries, or the refusal's type and full text.  No device: bind() is stubbed.

Where the replay may differ from the record, and only there:
  * a refused configure leaves lr / betas / eps and the workspace alone (the recorded engine had assigned them before it refused);
    what it must do instead is asserted here directly — the engine is the object it was;
  * a refusal's text may differ where two rules are broken at once: it is then the constructor's text for the same model and
    settings (configure checks in the constructor's order).  Counted and printed; jiVAE with kl="analytic" and particles / renyi.
"""
import functools
import json
import os

import pytest

from conftest import GOLDEN

import _engine_settings_cases as sc
from pyroved_amd.engine import IVAEEngine


@functools.lru_cache(maxsize=None)
def recorded():
    with open(os.path.join(GOLDEN, "engine_settings.json")) as f:
        data = json.load(f)
    assert data["axes"] == [[k, list(v)] for k, v in sc.AXES] and data["changes"] == list(sc.CHANGES)
    assert data["dec_kernels"] == list(sc.DEC_KERNELS)
    return sc.unpack(data)


@functools.lru_cache(maxsize=None)
def replayed():
    return json.loads(json.dumps(sc.record()))            # (through JSON: tuples become lists, as in the record)


def test_recorded_table_counts():
    flat = [o for v in recorded()["constructor"].values() for o in v]
    assert len(flat) == 4096 and sum(o[0] == "ok" for o in flat) == 420 and sum(o[0] == "ValueError" for o in flat) == 3676
    assert len({o[1] for o in flat if o[0] != "ok"}) == 30
    assert os.path.getsize(os.path.join(GOLDEN, "engine_settings.json")) < 100 << 10


@pytest.mark.parametrize("table", ("constructor", "small"))
def test_constructor_replay(table):
    want, got = recorded()[table], replayed()[table]
    assert sorted(want) == sorted(got)
    axes = sc.AXES if table == "constructor" else sc.SMALL_AXES
    for name in want:
        assert len(want[name]) == len(got[name]) == len(sc.cases(axes))
        for kw, w, g in zip(sc.cases(axes), want[name], got[name]):
            assert g == w, (name, kw)


def _configure_cases(name):
    """(constructor keywords of the start state, dec_kernel, change, recorded outcome, replayed outcome) of one model."""
    starts = [kw for kw, o in zip(sc.cases(), recorded()["constructor"][name]) if o[0] == "ok"]
    rows_w, rows_g = recorded()["configure"][name], replayed()["configure"][name]
    assert len(starts) == len(rows_w) == len(rows_g)
    for kw, row_w, row_g in zip(starts, rows_w, rows_g):
        combos = [(dk, ch) for dk in sc.DEC_KERNELS for ch in sc.CHANGES]
        assert len(combos) == len(row_w) == len(row_g)
        for (dk, ch), w, g in zip(combos, row_w, row_g):
            yield kw, dk, ch, w, g


def test_configure_replay():
    reordered = {}
    for name in sc.CONFIGURE_MODELS:
        by_kw = {sc.key(kw): o for kw, o in zip(sc.cases(), recorded()["constructor"][name])}
        for kw, dk, ch, w, g in _configure_cases(name):
            where = (name, kw, dk, ch)
            assert g[0] == w[0], where                                # accepted or refused, the exception's type
            if g[0] == "ok":
                assert g == w, where                                  # settings, optimizer settings, plan, workspace reset
                continue
            assert g[2] == w[2] == "kept" and g[4] == w[4], where      # the settings and the plan after a refusal
            assert g[3] == [1e-3, [0.9, 0.999], 1e-8] and g[5] is True, where     # (the record: lr assigned in 18, ws dropped in 1398)
            if g[1] != w[1]:                                          # the allowance: the constructor's text for the same settings
                assert g[1] == by_kw[sc.key(sc.target(kw, ch))][1], where
                reordered.setdefault((name, json.dumps(ch), w[1][:24], g[1][:14]), []).append(dk)
    for k, v in sorted(reordered.items()):
        print("refusal reordered (%d cases): %s" % (len(v), k,))
    assert all(name == "jivae" and '"kl": "analytic"' in ch for name, ch, _, _ in reordered)
    assert sum(len(v) for v in reordered.values()) == 36              # 6 accepted jiVAE states x 2 double changes x 3 dec_kernel


def _identity(eng):
    return [id(v) for v in (eng.lr, eng.betas, eng.adam_eps, eng.ws, eng._static, eng.pixel_weights)] + sc.settings_of(eng)


def test_refused_configure_changes_nothing_and_agrees_with_the_constructor(monkeypatch):
    """After every refused configure — with lr, betas and eps in the same call — the engine holds the objects it held; after an
    accepted one the static plan is rebuilt.  And configure into some settings from a valid state is refused if and only if the
    constructor refuses those settings (at the same dec_kernel), with the same text."""
    monkeypatch.setattr(IVAEEngine, "_static_plan", lambda self: object())
    n_refused = n_ok = 0
    with sc.unbound():
        for name in sc.CONFIGURE_MODELS:
            m, fresh = sc.MODELS[name](), sc.MODELS[name]()
            ctor = {}
            for kw, o in zip(sc.cases(), replayed()["constructor"][name]):
                if o[0] != "ok":
                    continue
                for dk in sc.DEC_KERNELS:
                    for ch in sc.CHANGES:
                        eng, _ = sc.construct(m, kw)
                        eng.flat, eng._static, eng.ws, eng.dec_kernel = object(), object(), sc.SENTINEL, dk     # ("bound")
                        before, static = _identity(eng), eng._static
                        tgt = sc.target(kw, ch)
                        if (sc.key(tgt), dk) not in ctor:
                            monkeypatch.setattr(IVAEEngine, "dec_kernel", dk)
                            ctor[sc.key(tgt), dk] = sc.construct(fresh, tgt)[1]
                            monkeypatch.setattr(IVAEEngine, "dec_kernel", 0)
                        want = ctor[sc.key(tgt), dk]
                        try:
                            eng.configure(**sc._kw(m, dict(ch, lr=3e-3, betas=(0.8, 0.99), eps=1e-7)))
                        except ValueError as e:
                            assert _identity(eng) == before, (name, kw, dk, ch)
                            assert want == ["ValueError", str(e)], (name, kw, dk, ch)
                            n_refused += 1
                        else:
                            assert want[0] == "ok" and want[1] == sc.plan_of(eng), (name, kw, dk, ch, want)
                            assert (eng.lr, eng.betas, eng.adam_eps) == (3e-3, (0.8, 0.99), 1e-7) and eng._static is not static
                            n_ok += 1
    assert n_refused > 1000 and n_ok > 1000, (n_refused, n_ok)
