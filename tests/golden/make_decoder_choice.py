#!/usr/bin/env python
"""
make_decoder_choice.py — records tests/golden/decoder_choice_plans.json and tests/golden/decoder_choice_table.json: what the
library answers about the fused decoder kernels' selection (tests/_decoder_choice_cases.py).  tests/test_decoder_choice_cpu.py
replays both.

The files are a record of the selection AS IT WAS on the commit before the resolved choice (pv_sdec_fused.h: PvDecChoice) replaced
the per-question queries: they were made from a worktree of that commit, not from this tree —
    git worktree add --detach ../parent <that commit>
    make -C ../parent/pyroved_amd/csrc all experiments
    python tests/golden/make_decoder_choice.py --tree ../parent
The plans go through entry points whose signatures the change left alone, so that is all they need.  The table goes through
pv_debug_decoder_choice, which that commit does not have: the recording used a THROWAWAY hook of the same name and output,
appended to the worktree's pv_sdec_fused_bf16.hip before the make above and never committed.  It filled the fields from the old
queries — sel_valid from pv_sdec_fused_sel_valid; waves, rec_fmt, park_bytes (parks: != 0) and weighted from
pv_sdec_fused_bf16_waves / _record_fmt / _park_bytes / _weighted_ok; img_mode, img_scale, img_qswap from
pv_sdec_fused_bf16_prep_args on a PvFused holding units and sel; hosts_guide from pv_sdec_fused_fold_ok's selection half
(!x3 && fb_use_w8) — and family, prec, x3_waves, ds from fb_x3_kind / fb_use_w8 exactly as pv_sdec_fused_bf16_launch turned them
into a launch (x3_waves 0 where the kind is no wave count its launcher accepts; prec -1, x3_waves 0, ds 0 where the family has none).
Without --tree the script records this tree: a changed selection then shows up as a changed file, to be committed on purpose.
No device is needed.
"""
import argparse
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import _decoder_choice_cases as dc  # noqa: E402


def dump(name, data):
    path = os.path.join(HERE, name)
    with open(path, "w") as f:
        json.dump(data, f, separators=(",", ":"))
        f.write("\n")
    return os.path.getsize(path)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tree", default=None, help="record the libraries of this checkout instead of this tree's")
    a = ap.parse_args()
    pkg = os.path.join(os.path.abspath(a.tree), "pyroved_amd") if a.tree else dc.PKG
    libs = {"shipped": os.path.join(pkg, "libpyroved_amd.so"), "experiments": os.path.join(pkg, "libpyroved_amd_exp.so")}
    records = dc.plans(libs["shipped"])
    data = dc.pack_plans(records)
    assert dc.unpack_plans(data) == records
    n = dump("decoder_choice_plans.json", data)
    print("plans: %d, %d distinct size rows, %d bytes" % (len(records), len(data["sizes"]), n))
    tables = {config: dc.table_of(config, libs) for config in dc.CONFIGS}
    data = dc.pack_tables(tables)
    assert dc.unpack_tables(data) == tables
    n = dump("decoder_choice_table.json", data)
    print("table: %d configurations x %d rows, %d bytes" % (len(tables), len(dc.table_rows()), n))


if __name__ == "__main__":
    main()
