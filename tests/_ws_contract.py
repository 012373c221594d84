"""
_ws_contract.py — the kit of the workspace-contract tests (tests/test_gpu_workspace_contract.py on the GPU,
tests/test_workspace_contract_cpu.py without one).

include/pyroved_amd.h promises three things about the caller-owned workspace of every entry point:
  size      what a pv_*_workspace_bytes* query returns is enough;
  refusal   a smaller workspace is PV_EWS;
  content   the workspace is scratch: on entry it may hold anything, and nothing is kept in it between calls — except inside the
            three documented pairs (pv_ivae_guide -> pv_ivae_guide_backward, pv_convnet_forward -> pv_convnet_backward, the label
            MLP's forward -> backward), where it must stay untouched from the first call to the second.
The engines allocate the workspace with torch.empty, and the caching allocator hands the same block back for the same shape: a
region a kernel reads without having written it holds zeros (a fresh block) or the right values of the previous identical call.
"A repeated call is bit-identical" cannot see that.  This kit can: one cell = one call sequence, run on the engine's own
workspace and then on a workspace of EXACTLY the queried size between two guard regions, filled with zeros, with 0xFF bytes
(NaN as fp32 and bf16, 0xFFFFFFFF as a flag word, 255 as a winner byte) and with seeded noise; every result must have the same
bits in all four runs, be finite, and leave the guards as they were.

Regions whose CONTENT is used as an index, a flag or a count (read from carve() in csrc/pv_plan.hip, vcarve() in pv_ved.hip,
ncarve() in pv_convnet.hip, mlp_carve() in pv_ss.hip and their consumers), and why any content is safe on entry:
  Layout::enc_flags (pv_plan.hip: carve; pv_encoder.hip: pv_enc_kernel)   the tiled one-launch encoder's per-tile flags.  A
            consumer waits for the launch's generation tag (enc_next_gen: a process-wide counter with a random start), never for
            "non-zero"; the producers store the tag after their tiles.  A stale word equals the tag with probability 2^-32 per
            word, and a consumer that gives up computes the tiles itself.  Written before read within one launch.
  the 1024 + 16 words behind enc_flags (PvEncFold::coop_flags)            read by the experiments build's shared first layer only
            (a hand-off tag taken as "the word's content + 1": any content); the shipped library never touches them.
  Layout::ccode / ccode2, VLayout / NLayout sc.code / sc.code2            the max-pool winner bytes of the fused convolution +
            pooling blocks (pv_convstack.h: stack_fwd writes one byte per pooled output, stack_bwd reads the same bytes under
            the same conditions).  Written by the forward of the same call — or, for pv_convnet_*, of the documented pair.
  Layout::cwt / chead_wt, VLayout / NLayout wt                           the tiled weight images (a table addressed by
            pvcs::wt_layout offsets computed on the host): every image a launch reads is written by the wt_prep launch of the
            same entry point.
  Layout::f_part_hz (+ the row-sum slots behind it), f_part              per-sample slots / per-workgroup records that the closing
            launch SUMS over all kmax slots: content, not an index, but the sum reads slots no workgroup wrote, so the unused
            ones must be zero-filled in the same call (pv_sdec_fused_bf16_prep_args: nzero4; pv_plan.hip: hipMemsetAsync for the
            f32 kernel) — the invariant this kit exists to check.
Everything else is fp32 data that a launch of the same call writes before another reads it.  No region holds a count: the
deferred weight-gradient list (PvFinishList) lives on the host.

Out of scope here: captured graphs (they bake the workspace pointer), the data-parallel one-call step, overruns shorter than a
region's 256-byte padding (they show only as reads), and any undersized workspace on the GPU (the CPU file checks PV_EWS).
"""
import ctypes as C
import time

import torch

from pyroved_amd import _abi

FILLS = ("zeros", "ones", "noise")
GUARD = 1 << 20                      # bytes on either side of the workspace: a condition of the test, not a measurement
INPUT_GUARD = 1 << 16                # floats of NaN behind every flushed input
_GUARD_PATTERN = {"zeros": 0xA5, "ones": 0x5A, "noise": None}      # (noise: seeded bytes from another seed than the fill's)
NOISE_SEED, GUARD_SEED = 1234, 4321


# ------------------------------------------------------------------------------- fills and guards
def _noise(n, seed, device):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, 256, (n,), generator=g, dtype=torch.uint8).to(device)


def fill_(t, fill):
    """Fills a uint8 tensor in place with one of FILLS."""
    if fill == "zeros":
        t.zero_()
    elif fill == "ones":
        t.fill_(0xFF)
    elif fill == "noise":
        t.copy_(_noise(t.numel(), NOISE_SEED, t.device))
    else:
        raise KeyError(fill)
    return t


class Guards:
    """The two guard regions around a workspace view and their saved copies."""

    def __init__(self, base, need, guard):
        self.base, self.need, self.guard = base, need, guard
        self.saved = (base[:guard].clone(), base[guard + need:].clone())

    @property
    def ptr(self):
        """address of the middle region (a view of zero bytes has no data_ptr of its own)"""
        return self.base.data_ptr() + self.guard

    def damage(self):
        """[(which guard, offset of the first changed byte relative to the workspace, number of changed bytes)]"""
        out = []
        for which, now, was, at in (("front", self.base[:self.guard], self.saved[0], -self.guard),
                                    ("back", self.base[self.guard + self.need:], self.saved[1], self.need)):
            bad = torch.nonzero(now != was).flatten()
            if bad.numel():
                out.append((which, at + int(bad[0]), int(bad.numel())))
        return out

    def __call__(self):
        d = self.damage()
        assert not d, "guard bytes changed (guard, first offset from the workspace's start, bytes): %s" % (d,)


def guarded(need, fill, guard=GUARD, device="cuda"):
    """One uint8 buffer of need + 2 guard bytes: (the middle view of exactly `need` bytes filled with `fill`, check).  check()
    compares both guards with their saved copies byte for byte.  `guard` is a multiple of 4096, so the view keeps the
    allocation's alignment."""
    assert guard % 4096 == 0 and need >= 0
    base = torch.empty(need + 2 * guard, dtype=torch.uint8, device=device)
    pat = _GUARD_PATTERN[fill]
    for sl, seed in ((slice(0, guard), GUARD_SEED), (slice(guard + need, None), GUARD_SEED + 1)):
        if pat is None:
            base[sl].copy_(_noise(guard, seed, device))
        else:
            base[sl].fill_(pat)
    view = base[guard:guard + need]
    fill_(view, fill)
    return view, Guards(base, need, guard)


def install(eng, view, attr="ws", need=None):
    """Sets eng.<attr> to the view: the engines rebuild plan.ws / plan.ws_bytes from the attribute on every call.  After any
    configure() (it resets ws).  A view shorter than `need` is refused here: an engine would quietly replace it."""
    need = view.numel() if need is None else need
    if view.dtype != torch.uint8 or view.dim() != 1 or view.numel() < need:
        raise ValueError("workspace view of %d bytes (%s), need %d" % (view.numel(), view.dtype, need))
    setattr(eng, attr, view)
    return view


def flush(t, device="cuda"):
    """A device copy of an input tensor with INPUT_GUARD NaNs directly behind its last element (behind its last 16 bytes where
    the tensor is no multiple of 16 bytes: the start keeps the allocation's alignment).  A read past the end reads NaN."""
    if t is None:
        return None
    t = t.to(torch.float32)
    n = t.numel()
    buf = torch.full((n + INPUT_GUARD,), float("nan"), dtype=torch.float32, device=device)
    buf[:n].copy_(t.reshape(-1))
    return buf[:n].view(t.shape)


def same_bits(a, b):
    """Bitwise equality of two fp32 tensors (two NaNs are equal only with the same payload)."""
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.numel() == 0:
        return True
    return bool(torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32)))


# ------------------------------------------------------------------------------- one cell
class Run:
    """What a cell's make() returns: the objects one call sequence works on.
      eng         the object that owns the workspace attribute(s): an engine, or a stand-in for a raw C-ABI sequence
      workspaces  {attribute: callable -> the bytes the matching workspace query returns for this call's plan}
      inputs      {name: tensor}: the call's inputs (host or device); the fill runs get flush()ed copies
      outs        {name: device tensor}: every output buffer the call is given; NaN-filled before every call
      call        call(inputs): the library call(s)
      grads       () -> {name: tensor}: the gradient tensors the call writes (per-tensor views), or None
      scalars     () -> tensor of the 4 loss scalars, or None
      state       () -> {name: tensor}: what a one-call step updates (parameters, m, v per tensor), or None
      poison      (): NaN into every gradient / scalar buffer the call must overwrite
      restore     (): puts back what a call changes (parameters, Adam moments, running statistics), before every call
      zero_grads  the gradients must be exactly zero after the call (step=True: the header's zero_grads)
      judge       judge(snapshot of the noise-fill run): a reference of the family's own, at the family's own bars
      writes_ws   the call is known to write its workspace (False: a problem too small to need its scratch); checked on the
                  0xFF fill, so that a cell whose plan never pointed at the installed view cannot pass"""

    def __init__(self, eng, workspaces, inputs, call, outs=None, grads=None, scalars=None, state=None, poison=None,
                 restore=None, zero_grads=False, judge=None, writes_ws=True):
        self.writes_ws = writes_ws
        self.eng, self.workspaces, self.inputs, self.call = eng, workspaces, inputs, call
        self.outs = outs or {}
        self.grads, self.scalars, self.state = grads, scalars, state
        self.poison, self.restore, self.zero_grads, self.judge = poison, restore, zero_grads, judge


def snapshot(run):
    """Clones of everything the call produced: the scalars, every gradient tensor, every output it was given, and after a one-call
    step every parameter, m and v — per tensor (the flat buffers' alignment padding is not under contract)."""
    snap = {}
    if run.scalars is not None:
        snap["scalars"] = run.scalars().detach().clone()
    if run.grads is not None:
        for k, v in run.grads().items():
            snap["grad." + k] = v.detach().clone()
    for k, v in run.outs.items():
        snap["out." + k] = v.detach().clone()
    if run.state is not None:
        for k, v in run.state().items():
            snap["state." + k] = v.detach().clone()
    return snap


def _sync(device):
    if torch.device(device).type == "cuda":
        torch.cuda.synchronize()


def _one_call(run, inputs, device="cuda"):
    if run.restore is not None:
        run.restore()
    if run.poison is not None:
        run.poison()
    for v in run.outs.values():
        v.fill_(float("nan"))
    _sync(device)
    run.call(inputs)
    _sync(device)
    return snapshot(run)


def differing(a, b):
    return [k for k in a if not same_bits(a[k], b[k])]


def non_finite(snap):
    return [k for k, v in snap.items() if not bool(torch.isfinite(v).all())]


def engine_views(eng):
    """{key: (offset, shape)} of the parameters (not the batch-norm running statistics) in the engine's flat buffers."""
    return {k: (eng._layout[k], v.shape) for k, v in eng._views.items()
            if not k.endswith((".running_mean", ".running_var"))}


def engine_run(eng, inputs, call, outs=None, workspaces=None, want_grads=True, scalars=True, step=False, extra_grads=None,
               judge=None):
    """A Run over an IVAEEngine-like object: gradients through grad_of, NaN into eng.grad (scalars included) before every call,
    parameters / moments / running statistics / step count put back before every call."""
    views = engine_views(eng)
    saved = dict(flat=eng.flat.clone(), m=eng.m.clone(), v=eng.v.clone(), t=eng.adam_t)

    def restore():
        eng.flat.copy_(saved["flat"])
        eng.m.copy_(saved["m"])
        eng.v.copy_(saved["v"])
        eng.adam_t = saved["t"]

    def grads():
        g = {k: eng.grad_of(k) for k in views}
        if extra_grads is not None:
            g.update(extra_grads())
        return g

    def state():
        out = {}
        for k, (o, shape) in views.items():
            n = int(torch.Size(shape).numel())
            for name, buf in (("p", eng.flat), ("m", eng.m), ("v", eng.v)):
                out["%s.%s" % (name, k)] = buf[o:o + n]
        return out

    return Run(eng, workspaces, inputs, call, outs=outs, grads=grads if want_grads else None,
               scalars=(lambda: eng.scalars) if scalars else None, state=state if step else None,
               poison=lambda: eng.grad.fill_(float("nan")), restore=restore, zero_grads=step, judge=judge)


def run_cell(name, make, report=None, device="cuda"):
    """One cell (see the module docstring).  Returns (need bytes per workspace, seconds).  device="cpu" serves the kit's own
    tests, which run plain torch in place of the library."""
    t0 = time.perf_counter()
    run = make()
    # 1. two ordinary calls on the engine's own workspace: the family must be deterministic before a fill can be blamed
    first = _one_call(run, run.inputs, device)
    second = _one_call(run, run.inputs, device)
    diff = differing(first, second)
    assert not diff, "%s: NON-DETERMINISTIC family — two ordinary calls differ in %s (no fill involved)" % (name, diff)
    bad = non_finite(first)
    assert not bad, "%s: the ordinary call left non-finite values in %s" % (name, bad)
    # 2. the engine allocates what the query says, not more
    need = {}
    for attr, query in run.workspaces.items():
        ws = getattr(run.eng, attr)
        assert ws is not None, "%s: the call did not allocate %s" % (name, attr)
        need[attr] = int(ws.numel())
        want = int(query())
        assert need[attr] == want, "%s: the engine holds %d bytes of %s, the workspace query says %d" % (name, need[attr], attr, want)
    # 3. exactly `need` bytes between two guards, any content
    snaps = {}
    for fill in FILLS:
        checks = []
        for attr, n in need.items():
            view, check = guarded(n, fill, device=device)
            install(run.eng, view, attr, n)
            checks.append((attr, view, check))
        flushed = {k: (flush(v, device) if torch.is_tensor(v) else v) for k, v in run.inputs.items()}
        snaps[fill] = _one_call(run, flushed, device)
        for attr, view, check in checks:
            assert getattr(run.eng, attr) is view, "%s: the engine replaced the installed %s (fill %s)" % (name, attr, fill)
            if fill == "ones" and run.writes_ws and view.numel():
                assert bool((view != 0xFF).any()), "%s: the call left the installed %s untouched — it ran on another one" % (name, attr)
            d = check.damage()
            assert not d, "%s, fill %s: %s guard bytes changed (guard, first offset from the workspace's start, bytes): %s" % (
                name, fill, attr, d)
        bad = non_finite(snaps[fill])
        assert not bad, "%s, fill %s: non-finite values in %s — a read of bytes the call never wrote" % (name, fill, bad)
    # 4. the same bits whatever the workspace held
    for fill in FILLS:
        diff = differing(first, snaps[fill])
        assert not diff, "%s: fill %s changes %s — a read of bytes the call never wrote" % (name, fill, diff)
    # 5. a one-call step leaves the gradients zeroed
    if run.zero_grads:
        for fill in FILLS:
            nz = [k for k, v in snaps[fill].items() if k.startswith("grad.") and bool((v != 0).any())]
            assert not nz, "%s, fill %s: gradients not zero after the one-call step: %s" % (name, fill, nz)
    if run.judge is not None:
        run.judge(snaps["noise"])
    _sync(device)
    secs = time.perf_counter() - t0
    if report is not None:
        report(name, need, secs)
    return need, secs


# ------------------------------------------------------------------------------- workspace queries, restated per engine call
def ivae_query(eng, batch, what=1, beta=1.0):
    """The query that belongs to the entry point an IVAEEngine call reaches (what: PV_WS_STEP 1, _ENCODE 2, _DECODE 3)."""
    lib = _abi.lib()

    def q():
        ws = eng.ws
        p = eng._plan(batch, beta, what) if what == 1 else eng._plan(batch, what=what)
        eng.ws = ws                                     # (_plan may not replace what is installed; keep it in any case)
        if what == 1:                                   # (the training step: the one query of the engine's objective)
            return lib.pv_ivae_objective_workspace_bytes(C.byref(p), C.byref(eng._objective))
        return lib.pv_ivae_workspace_bytes_for(C.byref(p), what)
    return q


def ved_query(eng, batch):
    def q():
        ws = eng.ws
        p = eng._plan(batch)
        eng.ws = ws
        return _abi.lib().pv_ved_workspace_bytes(C.byref(p))
    return q


def mlp_query(eng, batch):
    def q():
        plan = eng._mlp
        plan.batch = batch
        return _abi.lib().pv_mlp_workspace_bytes(C.byref(plan))
    return q
