"""
The step's objective as one descriptor — pv_ivae_objective and pv_ivae_objective_workspace_bytes / _loss_and_grads / _step in the
C ABI — where no GPU is needed: for every plan x descriptor pair the unified query answers what the matching old query answers
(sizes and PV_EINVAL alike), the two unified calls refuse a plan without buffers with the old calls' code, the combinations no
kernel path exists for are PV_EINVAL from all three functions, and the header, the ctypes mirror and the unchanged v17 plan agree.
Host arithmetic and refusals return before any HIP call.  Plans are tests/_plan_kit.py's: 784 positions x ch observations, batch 16.
"""
import ctypes as C
import os
import re
import subprocess
import tempfile

from conftest import ROOT

from pyroved_amd import _abi
from _plan_kit import PLAN_FIELDS, _plan, _small_plan, _vanilla_plan

EINVAL = -1
ALPHA = 0.5
KEEP = C.create_string_buffer(64)                 # a host address for pointers that no refused call may touch
HOST = C.addressof(KEEP)
ELBO, RENYI = _abi.PV_BOUND_ELBO, _abi.PV_BOUND_RENYI
NONE, SHARED, PER_IMAGE = _abi.PV_OBS_W_NONE, _abi.PV_OBS_W_SHARED, _abi.PV_OBS_W_PER_IMAGE


# ------------------------------------------------------------------------------- plans
def _conv_plan():
    p = _plan(0, 1)                                                 # Conv2d(1 -> 4, k 3) on 28 x 28
    p.n_pix, p.n_enc, p.n_enc_ops, p.enc_ndim = 784, 0, 1, 2
    p.enc_in_dim[0] = p.enc_in_dim[1] = 28
    op = _abi.pv_op()
    op.kind, op.cin, op.cout, op.ksize, op.act, op.w_off, op.b_off = _abi.OP["conv"], 1, 4, 3, _abi.ACT["lrelu"], 0, 36
    p.enc_ops[0] = op
    p.head.in_dim = 4 * 784
    return p


def _with(p, **fields):
    for k, v in fields.items():
        setattr(p, k, v)
    return p


def _dy_plan():
    p = _plan(0, 1)
    p.c_dim, p.fc_latent.in_dim = 1, 3
    p.enc[0].in_dim += 1
    p.dy = HOST
    return p


def plans():
    out = {}
    for fused in (0, 1, 2, 3):
        for ch in (1, 3):
            for tag, flags in (("", 0), ("+channels", _abi.PV_PLAN_FUSED_CHANNELS), ("+fast", _abi.PV_PLAN_FAST_WEIGHTS)):
                out["fused%d-ch%d%s" % (fused, ch, tag)] = _with(_plan(fused, ch), flags=flags)
    for fused in (2, 3):
        for dk in (1, 2):
            for tag, flags in (("", 0), ("+fast", _abi.PV_PLAN_FAST_WEIGHTS)):
                out["fused%d-dec_kernel%d%s" % (fused, dk, tag)] = _with(_plan(fused, 1), dec_kernel=dk, flags=flags)
    for fused in (0, 2, 3):
        out["fused%d-analytic" % fused] = _with(_plan(fused, 1), kl_mode=_abi.KL["analytic"])
    for fused in (0, 2):
        out["vanilla-fused%d" % fused] = _vanilla_plan(fused)
        out["jivae-fused%d" % fused] = _small_plan(discrete_dim=3, fused=fused)
    out["conv"] = _conv_plan()
    out["ext_encoder"] = _with(_plan(0, 1), ext_encoder=1)
    out["ext_decoder"] = _with(_plan(0, 1), ext_decoder=1)
    for field in ("row_w", "row_elbo", "class_onehot"):
        out[field] = _with(_plan(0, 1), **{field: HOST})
    out["dy"] = _dy_plan()
    return out


# ------------------------------------------------------------------------------- descriptors and the old entry points they name
def objective(P=1, bound=ELBO, alpha=0.0, kind=NONE, obs_w=None, weights_out=None):
    o = _abi.pv_ivae_objective()
    o.num_particles, o.bound, o.alpha, o.obs_w_kind, o.obs_w, o.weights_out = P, bound, alpha, kind, obs_w, weights_out
    return o


def descriptors():
    """{name: (descriptor or None, old query, old loss_and_grads(p, want_grads), old step)}"""
    L = _abi.lib()
    out = {"null": (None, lambda p: L.pv_ivae_workspace_bytes_for(p, 1), lambda p, g: L.pv_ivae_loss_and_grads(p, g, None),
                    lambda p: L.pv_ivae_step(p, None)),
           "plain": (objective(), lambda p: L.pv_ivae_workspace_bytes_for(p, 1), lambda p, g: L.pv_ivae_loss_and_grads(p, g, None),
                     lambda p: L.pv_ivae_step(p, None))}
    for P in (1, 3):
        out["particles%d" % P] = (objective(P), lambda p, P=P: L.pv_ivae_particles_workspace_bytes(p, P),
                                  lambda p, g, P=P: L.pv_ivae_particles_loss_and_grads(p, P, g, None),
                                  lambda p, P=P: L.pv_ivae_particles_step(p, P, None))
    for P in (1, 3, 1025):
        out["renyi%d" % P] = (objective(P, RENYI, ALPHA, weights_out=HOST), lambda p, P=P: L.pv_ivae_renyi_workspace_bytes(p, P),
                              lambda p, g, P=P: L.pv_ivae_renyi_loss_and_grads(p, P, ALPHA, g, HOST, None),
                              lambda p, P=P: L.pv_ivae_renyi_step(p, P, ALPHA, HOST, None))
    out["shared"] = (objective(kind=SHARED, obs_w=HOST), lambda p: L.pv_ivae_weighted_workspace_bytes(p),
                     lambda p, g: L.pv_ivae_weighted_loss_and_grads(p, HOST, g, None), lambda p: L.pv_ivae_weighted_step(p, HOST, None))
    out["per_image"] = (objective(kind=PER_IMAGE, obs_w=HOST), lambda p: L.pv_ivae_weighted_workspace_bytes(p),
                        lambda p, g: L.pv_ivae_weighted_images_loss_and_grads(p, HOST, g, None),
                        lambda p: L.pv_ivae_weighted_images_step(p, HOST, None))
    return out


def _ref(o):
    return None if o is None else C.byref(o)


# ------------------------------------------------------------------------------- 1, 2: the unified trio against the old functions
def test_unified_query_and_calls_answer_what_the_old_entry_points_answer():
    """Every plan x descriptor pair, collected and compared in one go: (query, loss only, loss and gradients, step).  The plans carry
    no buffers, so every call is refused before it touches a pointer — with the old call's own code."""
    L = _abi.lib()
    new, old = {}, {}
    for pname, p in plans().items():
        ref = C.byref(p)
        for dname, (o, q, lag, step) in descriptors().items():
            new[pname, dname] = (L.pv_ivae_objective_workspace_bytes(ref, _ref(o)),
                                 L.pv_ivae_objective_loss_and_grads(ref, _ref(o), 0, None),
                                 L.pv_ivae_objective_loss_and_grads(ref, _ref(o), 1, None),
                                 L.pv_ivae_objective_step(ref, _ref(o), None))
            old[pname, dname] = (q(ref), lag(ref, 0), lag(ref, 1), step(ref))
    assert new == old, {k: (new[k], old[k]) for k in new if new[k] != old[k]}
    assert all(v[1:] == (EINVAL, EINVAL, EINVAL) for v in new.values())
    # the table is not one answer repeated: sizes and refusals both occur, and the objectives' layouts differ where they should
    sizes = {k: v[0] for k, v in new.items()}
    assert sum(1 for s in sizes.values() if s > 0) > 100 and sum(1 for s in sizes.values() if s == EINVAL) > 100
    assert all(s > 0 or s == EINVAL for s in sizes.values())
    base = "fused2-ch1"
    assert sizes[base, "null"] == sizes[base, "plain"] == sizes[base, "particles1"] == sizes[base, "renyi1"]
    assert sizes[base, "null"] < sizes[base, "particles3"] < sizes[base, "renyi3"]
    assert sizes[base, "shared"] == sizes[base, "per_image"] == sizes["fused1-ch1", "null"] != sizes[base, "null"]
    assert sizes["fused3-ch1+fast", "shared"] > 0 and sizes["fused3-ch1", "shared"] == EINVAL
    assert sizes[base, "renyi1025"] == EINVAL and sizes["ext_decoder", "null"] > 0 and sizes["ext_decoder", "particles3"] == EINVAL


# ------------------------------------------------------------------------------- 3: what only the descriptor can spell
def test_combinations_without_a_kernel_path_are_refused():
    L = _abi.lib()

    def answers(p, o):
        ref = C.byref(p)
        return (L.pv_ivae_objective_workspace_bytes(ref, C.byref(o)), L.pv_ivae_objective_loss_and_grads(ref, C.byref(o), 0, None),
                L.pv_ivae_objective_loss_and_grads(ref, C.byref(o), 1, None), L.pv_ivae_objective_step(ref, C.byref(o), None))
    refused = (EINVAL,) * 4
    for fused in (0, 2):
        p = _plan(fused, 1)
        for kind in (SHARED, PER_IMAGE):
            assert answers(p, objective(3, kind=kind, obs_w=HOST)) == refused                       # weights with P = 3
            assert answers(p, objective(3, RENYI, ALPHA, kind=kind, obs_w=HOST)) == refused         # weights with the Renyi bound
            assert answers(p, objective(1, RENYI, ALPHA, kind=kind, obs_w=HOST)) == refused         # ... at one particle too
        assert answers(p, objective(weights_out=HOST)) == refused                                   # weights_out with the ELBO
        assert answers(p, objective(3, weights_out=HOST)) == refused
        assert answers(p, objective(kind=SHARED, obs_w=HOST, weights_out=HOST)) == refused
        assert answers(p, objective(bound=7)) == refused and answers(p, objective(bound=-1)) == refused
        assert answers(p, objective(kind=7, obs_w=HOST)) == refused and answers(p, objective(kind=-1, obs_w=HOST)) == refused
        assert answers(p, objective(0)) == refused and answers(p, objective(-2, RENYI, ALPHA)) == refused
        # weights without a pointer: the query does not read it and answers; the calls refuse
        for kind in (SHARED, PER_IMAGE):
            got = answers(p, objective(kind=kind))
            assert got[0] == L.pv_ivae_weighted_workspace_bytes(C.byref(p)) > 0 and got[1:] == refused[1:]
    # the query does not validate alpha, the calls do (with buffers or without: the descriptor comes first)
    p = _plan(2, 1)
    for alpha in (1.0, float("nan"), float("inf")):
        got = answers(p, objective(3, RENYI, alpha))
        assert got[0] == L.pv_ivae_renyi_workspace_bytes(C.byref(p), 3) > 0 and got[1:] == refused[1:]


# ------------------------------------------------------------------------------- 4: header, mirror, unchanged ABI
def test_header_mirror_and_unchanged_abi():
    src = open(os.path.join(ROOT, "include", "pyroved_amd.h")).read()
    lib = _abi.lib()
    for decl in ("int64_t pv_ivae_objective_workspace_bytes(const pv_ivae_plan* plan, const pv_ivae_objective* objective);",
                 "int pv_ivae_objective_loss_and_grads(const pv_ivae_plan* plan, const pv_ivae_objective* objective, int want_grads, "
                 "void* stream);",
                 "int pv_ivae_objective_step(const pv_ivae_plan* plan, const pv_ivae_objective* objective, void* stream);"):
        assert decl in src, decl
        name = re.search(r"(pv_\w+)\(", decl).group(1)
        assert name in _abi.SIGNATURES and getattr(lib, name) is not None
    body = re.search(r"typedef struct pv_ivae_objective \{(.*?)\} pv_ivae_objective;", src, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = [re.search(r"(\w+)\s*$", d.strip()).group(1) for d in body.split(";") if d.strip()]
    assert fields == [f[0] for f in _abi.pv_ivae_objective._fields_]
    for name, val in (("PV_BOUND_ELBO", ELBO), ("PV_BOUND_RENYI", RENYI), ("PV_OBS_W_NONE", NONE), ("PV_OBS_W_SHARED", SHARED),
                      ("PV_OBS_W_PER_IMAGE", PER_IMAGE)):
        assert int(re.search(r"#define\s+%s\s+(\d+)" % name, src).group(1)) == val, name
    probe = r'''
#include <stdio.h>
#include <stddef.h>
#include "pyroved_amd.h"
int main() {
  printf("%zu %zu %zu %zu %zu %zu %zu %zu %d\n", sizeof(pv_ivae_objective), offsetof(pv_ivae_objective, num_particles),
         offsetof(pv_ivae_objective, bound), offsetof(pv_ivae_objective, alpha), offsetof(pv_ivae_objective, obs_w_kind),
         offsetof(pv_ivae_objective, obs_w), offsetof(pv_ivae_objective, weights_out), sizeof(pv_ivae_plan), PV_ABI_VERSION);
  return 0; }'''
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "p.c"), "w").write(probe)
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), os.path.join(d, "p.c"), "-o", os.path.join(d, "p")])
        got = [int(v) for v in subprocess.check_output([os.path.join(d, "p")]).split()]
    O = _abi.pv_ivae_objective
    assert got == [C.sizeof(O), O.num_particles.offset, O.bound.offset, O.alpha.offset, O.obs_w_kind.offset, O.obs_w.offset,
                   O.weights_out.offset, 2824, 17]
    assert _abi.PV_ABI_VERSION == 17 and lib.pv_version() == 17 and C.sizeof(_abi.pv_ivae_plan) == 2824
    assert [f[0] for f in _abi.pv_ivae_plan._fields_] == PLAN_FIELDS
