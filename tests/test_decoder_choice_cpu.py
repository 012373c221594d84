"""
test_decoder_choice_cpu.py — the fused decoder kernels' selection, replayed against the record made before the one resolved
choice (pv_sdec_fused.h: PvDecChoice) replaced the per-question queries: tests/golden/decoder_choice_plans.json and
decoder_choice_table.json (tests/golden/make_decoder_choice.py; cases: tests/_decoder_choice_cases.py).  Every integer and every
string must be the recorded one.  Host-side queries only: no device.
"""
import json
import os

import pytest

import _decoder_choice_cases as dc

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _load(name):
    with open(os.path.join(GOLDEN, name)) as f:
        return json.load(f)


def test_plans_replay():
    """Sizes of every entry-point family, routing and weighted kernel names of ~10 000 plans on both sides of every size switch"""
    want = dc.unpack_plans(_load("decoder_choice_plans.json"))
    cases = dc.plan_cases()
    assert len(want) == len(cases)
    lib = dc.open_lib(dc.SHIPPED)
    bad = []
    for (label, p), w in zip(cases, want):
        got = dc.plan_record(lib, p)
        if got != w:
            bad.append((label, [(q, a, b) for q, a, b in zip(dc.QUERIES, got, w) if a != b]))
    assert not bad, "%d plans differ (query, now, recorded); the first: %r" % (len(bad), bad[:3])
    # the record is not vacuous: valid and refused plans, the fused route, folding and non-folding guides, misalignment mattering
    col = {q: [w[i] for w in want] for i, q in enumerate(dc.QUERIES)}
    assert min(col["ws_all"]) < 0 < max(col["ws_all"]) and 0 < sum(col["uses_fused"]) < len(want)
    assert sum(col["guide_folds_misaligned"]) == 0 < sum(col["guide_folds"]) < len(want)
    assert len(set(col["wname_shared_grads"])) >= 4


@pytest.mark.parametrize("config", list(dc.CONFIGS))
def test_choice_table_replay(config):
    """(fused, units, grads, sel) through pv_debug_decoder_choice, and the kernel names, in a fresh process per library build and
    setting of the experiments build's switches"""
    which = dc.CONFIGS[config][0]
    if which == "experiments" and not os.path.exists(dc.EXPERIMENTS):
        pytest.skip("the experiments library (make -C pyroved_amd/csrc experiments) is not built: its rows cannot be replayed")
    want = dc.unpack_tables(_load("decoder_choice_table.json"))[config]
    got = dc.table_of(config)
    rows = dc.table_rows()
    choice = want["choice"]
    assert len(choice) == len(rows) == len(got["choice"])
    bad = [(r, [(f, a, b) for f, a, b in zip(dc.FIELDS, g, w) if a != b]) for r, g, w in zip(rows, got["choice"], choice) if g != w]
    assert not bad, "%d rows (fused, units, grads, sel) differ (field, now, recorded); the first: %r" % (len(bad), bad[:5])
    assert got["names"] == want["names"]
    assert got["fold_names"] == want["fold_names"]
