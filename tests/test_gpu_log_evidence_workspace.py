"""
The workspace contract (tests/_ws_contract.py: exact size, any prior content, no stray writes) for the held-out log-evidence:
pv_ivae_evidence_workspace_bytes / pv_ivae_evidence_accumulate through engine.log_evidence_chunk.

One cell = two chunks of P particles into one state and the finish, run by the kit's run_cell: twice on the engine's own evidence
workspace (which must hold exactly what the query says), then on a workspace of exactly the queried size between two guard
regions filled with zeros, with 0xFF bytes (NaN as fp32) and with seeded noise.  log p^, ESS and the state must have the same
bits in all runs and be finite, and the guards must stay as they were.  The evidence layout is the multi-particle forward layout
(pv_plan.hip: carve with Layout::ev), so the regions whose content is an index or a flag are the ones the kit's docstring
lists; the forward-only fused launches sum no slot they did not write.
The cells: the three forward kernels on 8x8 `rts`, the vanilla decoder (pv_lik_elem per particle), the Poisson model with three
channels (the per-image normaliser, the layered multi-channel kernels), class conditioning.
"""
import ctypes as C

import pytest
import torch

from pyroved_amd import _abi
from _judge import cpu_threads_16                           # noqa: F401  (autouse fixture)
from _ws_contract import Run, run_cell
import _evidence_kit as ek

pytestmark = pytest.mark.gpu

CELLS = [("8x8_rts_b6_p3", 0), ("8x8_rts_b6_p3", 2), ("8x8_rts_b6_p3", 3), ("8x8_none_b6_p3", 0), ("8x8_r_c3_poisson_b6_p3", 0),
         ("8x8_rt_cdim3_b6_p3", 2)]


def evidence_query(eng, batch, P):
    def q():
        ws = eng.ws
        p = eng._plan(batch, 1.0, what=2)
        eng.ws = ws
        return _abi.lib().pv_ivae_evidence_workspace_bytes(C.byref(p), P)
    return q


@pytest.mark.parametrize("name,fused", CELLS)
def test_evidence_workspace_contract(gpu_device, name, fused):
    def make():
        model, cfg, x, y, _, b, P = ek.make(name, "cuda")
        eps = ek.make(name, "cpu", particles=2 * P)[4]
        eng = model.engine(fused=fused)
        eng._ev_ws = eng._ev_need = None
        outs = dict(log_ev=torch.empty(b, device="cuda"), ess=torch.empty(b, device="cuda"), state=torch.empty(b, 4, device="cuda"))

        def call(inp):
            e = inp["eps"]
            st = eng.log_evidence_chunk(inp["x"], e[:P * b], inp.get("y"), outs["state"], first=True)
            st = eng.log_evidence_chunk(inp["x"], e[P * b:], inp.get("y"), st, first=False)
            ev, ess = eng.log_evidence_finish(st, 2 * P, True)
            outs["log_ev"].copy_(ev)
            outs["ess"].copy_(ess)

        def judge(snap):
            ref, bar = ek.reference_for(fused, model, cfg, x, eps, y, b, 2 * P)
            ek.check("%s fused=%d exact workspace, noise fill" % (name, fused), snap["out.log_ev"].cpu(), snap["out.ess"].cpu(), ref, bar)

        inputs = dict(x=x.cuda(), eps=eps.cuda())
        if y is not None:
            inputs["y"] = y.cuda()
        return Run(eng, {"_ev_ws": evidence_query(eng, b, P)}, inputs, call, outs=outs, judge=judge)
    need, secs = run_cell("%s fused=%d" % (name, fused), make)
    print("%s fused=%d: evidence workspace %d bytes, %.2f s" % (name, fused, need["_ev_ws"], secs))
