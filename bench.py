#!/usr/bin/env python
"""
bench.py — throughput of the SVI training hot path on MI355X.

  python bench.py --gpus N --steps K --warmup W [--config C1..C5] [--strong] [--dump-outputs DIR] [--full [--repeats R]]
  (N > 1: launched by torch.distributed.run, one rank per GPU over RCCL)

A plain run measures the headline figure and nothing else: set-up, the untimed state-free pass, --warmup SVI steps,
PREROLL_PASSES gradient-only passes (no optimizer update: they keep the clocks up without moving the training state), then
ONE timed region of exactly --steps steps; `ms_per_step` is that region's time / --steps.  --dump-outputs DIR then writes
what the timed path computed in its last step as DIR/<name>.npy: every entry of the model's state_dict after the step
(`param.<key>`, float32), the step's four loss scalars (`loss_terms`: loss, and the three ELBO terms, float64) and the loss
of every timed step (`loss_per_step`, float64).  Data, noise and weights are seeded, and the number of optimizer steps is
--warmup + --steps, so the same arguments give the same inputs on every run.
--full adds everything below: the other precision leg, repeated and converged regions, kernel events and rooflines, the
CPU baseline, the trainer / inference legs and the side configs (N = 1), both scalings and the conv config (N > 1).

Headline workload (BASELINE.json configs[1], "C2"): iVAE, data_dim (28, 28), latent_dim 2, invariances ['r','t'],
Bernoulli likelihood, batch 256 PER GPU (weak scaling; --strong: 256 GLOBAL, sharded), bf16 as that config names it:
the decoder's hidden-layer contractions take bf16 operands on the MFMA with fp32 accumulation (ELBO within 1e-5 of
the fp32 oracle, gradients to ~1e-2 — mixed-precision training), everything else fp32.  The same run repeats the
measurement on the library's default fp32-class path ("bf16x3": hi+lo operands, 3 products — the 1e-4 parity mode for
gradients too) and reports it as `fp32_class`.  Synthetic data torch.rand(..., seed 0), model/trainer seed 1,
random-init weights.  A step = Trace_ELBO loss + gradients over one minibatch already resident in HBM + [one
all-reduce of the flat gradient when N > 1] + Adam.

--config selects another BASELINE.json configuration: C1 iVAE 28x28 ['r'] B=128, C3 jiVAE K=10 28x28
['r'] B=512, C4 iVAE 64x64 ['r','t','s'] + set_encoder(convEncoderNet) B=128/GPU, C5 VED 64x64 -> 128 B=256/GPU.
The default N=1 run also times C1, C3, C4, C5 (one short subprocess each: a case that follows a much larger one in the
same process inherits its freed device memory and can measure slower) and carries them in `configs`.

The timed region is EXACTLY --steps steps bracketed by barrier + synchronize, max over ranks; it is repeated
--repeats times inside the invocation (default 5) and `ms_per_step` / `value` are the MEDIAN region (all regions in
`ms_per_step_all`), so a 20-step run is not one 3 ms sample.

Round 3: timed regions are repeated until two successive ones agree to 1 % (the box is still warming up for the first few:
`regions_discarded` says how many were dropped, cap 40), THEN --repeats regions are measured; `roofline.kernel` is the name
rocprofv3 prints for the kernel the library dispatches (asked from the library), `roofline.traffic` comes from the committed
PMC pass of the same config (profiles/traffic.json); the conv-encoder / VED configs carry `roofline_conv` = the heaviest
kernel-3 convolution launch, event-timed inside the step; the default N = 1 run adds `C4fc` (fc encoder), a `trainer` leg
(SVItrainer.step over a CPU DataLoader: what a user of the reference API calls) and an `inference` leg (encode + decode);
N > 1 runs report `allreduce_ms` and both scalings (`value` = weak, `strong` = the config's batch sharded).

Prints ONE JSON line (rank 0).  Besides the contract fields it carries
  roofline     the dominant kernel (the fused decoder kernel) against the dense MFMA peak of the instruction it
               runs on, its duration measured with HIP events recorded on the launch stream inside the timed
               region (every 8th step: an event pair costs ~10 us of stream bubbles),
  cpu_baseline the CPU oracle (eager-torch restatement of the reference) timed on this host's cores
               on a bounded sample of the same workload (rank 0, N = 1 only): best thread count and a 1-thread leg,
  elbo         per-image loss of the first timed step next to the oracle's value on the same inputs.
"""
import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys
import time

import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

# test hook: PV_BENCH_FORCE_DIST=1 initialises the process group and takes the multi-rank code path (sync, collective, barriers,
# max-over-ranks timing) at WORLD_SIZE 1 — on a one-GPU box it is the only way the nccl (= RCCL) backend ever executes this file
FORCE_DIST = bool(os.environ.get("PV_BENCH_FORCE_DIST"))
COLLECTIVE = {"want": os.environ.get("PV_BENCH_COLLECTIVE", "native"), "used": None}
N_RING = 16                      # distinct resident minibatches (n = 16 * B) for the 28x28 configs
MFMA_F32_PEAK_TFLOPS = 157.3     # MI355X_MICROARCH.md: v_mfma_f32_* f32-in peak
MFMA_BF16_PEAK_TFLOPS = 2500.0   # MI355X_MICROARCH.md: dense bf16 MFMA peak
HBM_PEAK_GBS = 8000.0
DEC_FLOP_PER_PIXEL = 3 * (2 * 2 * 128 + 2 * 128 * 128 * 2 + 2 * 128)   # spatial decoder fwd+bwd: 3 * 66 304

# name -> workload.  flops_per_image: algorithmic fwd+bwd FLOPs of the whole step per image (measured
# with FlopCounterMode on the reference's modules).  dec_passes: decoder evaluations per image (K for jiVAE).
CONFIGS = {
    "C1": dict(kind="ivae", data_dim=(28, 28), inv=["r"], batch=128, flops_per_image=1.566e8, dec_passes=1, ring=16,
               desc="iVAE 28x28 invariances=['r'] latent_dim=2 bernoulli"),
    "C2": dict(kind="ivae", data_dim=(28, 28), inv=["r", "t"], batch=256, flops_per_image=1.566e8, dec_passes=1, ring=16,
               desc="iVAE 28x28 invariances=['r','t'] latent_dim=2 bernoulli"),
    "C3": dict(kind="jivae", data_dim=(28, 28), inv=["r"], batch=512, K=10, flops_per_image=1.56e9, dec_passes=10, ring=4,
               desc="jiVAE discrete_dim=10 latent_dim=2 invariances=['r'] 28x28 bernoulli, exact enumeration"),
    "C4": dict(kind="ivae_conv", data_dim=(64, 64), inv=["r", "t", "s"], batch=128, flops_per_image=1.50e9, dec_passes=1,
               ring=4, desc="iVAE 64x64 invariances=['r','t','s'] + set_encoder(convEncoderNet default stack)"),
    "C4fc": dict(kind="ivae", data_dim=(64, 64), inv=["r", "t", "s"], batch=128, flops_per_image=8.18e8, dec_passes=1, ring=4,
                 desc="iVAE 64x64 invariances=['r','t','s'] latent_dim=2 bernoulli, fc encoder (SURVEY 8d: C4's other reading)"),
    "C5": dict(kind="ved", data_dim=(64, 64), out_dim=(128,), batch=256, flops_per_image=7.09e8, dec_passes=0, ring=2,
               desc="VED im2spec 64x64 image -> 128-point spectrum, default conv stacks"),
}
# HBM bytes per launch of a config's dominant kernel, from the committed rocprofv3 PMC passes (scripts/gpu_prof_r6.sh writes
# profiles/traffic.json: FETCH_SIZE doubled per the guide's gfx950 correction + WRITE_SIZE, separate passes).  NOT collected by
# this run: `traffic_source` says where from.  Keys "<config>:<mode>" (decoder kernel) and "<config>:<mode>:conv".
TRAFFIC = {}
_traffic_file = os.path.join(ROOT, "profiles", "traffic.json")
if os.path.exists(_traffic_file):
    try:
        for k_, v_ in json.load(open(_traffic_file)).items():
            TRAFFIC[k_] = (int(v_["bytes"]), v_["source"])
    except Exception:
        pass

EV_EVERY = 8                     # (N > 1: the all-reduce's torch events, every EV_EVERY-th step)
EV_PER_REGION = 1                # decoder / conv launches carrying HIP events per timed region, taken mid-region (a launch with events
                                 # costs the stream ~11 us: profiles/r05ay_bench_region_timing.txt); the measured regions' samples are pooled
PREROLL_PASSES = 100            # (plain run) gradient-only passes in front of the one timed region, a fixed count: see --full's
                                 # preroll below for why a short region wants them
PREROLL_MS, PREROLL_MAX = 10.0, 100   # untimed steps enqueued right in front of every timed region's opening synchronisation: ~10 ms of
                                 # them (at most 100; counted from the first region's step time, the same on every rank).  A 20-step
                                 # region is 2 ms — after the idle gap between regions it ran at a colder GPU's clocks (decoder
                                 # launch 87.8 vs 85.6 us, step 0.1091 vs 0.1049 ms); a training run is not 20 steps long


class HipEvents:
    """Raw hipEvent_t pairs (the library records them on the stream it launches on)."""
    def __init__(self, n):
        self.hip = C.CDLL("libamdhip64.so.7")      # already loaded by torch: the same runtime instance
        self.hip.hipEventCreate.argtypes = [C.POINTER(C.c_void_p)]
        self.hip.hipEventElapsedTime.argtypes = [C.POINTER(C.c_float), C.c_void_p, C.c_void_p]
        self.pairs = []
        for _ in range(n):
            a, b = C.c_void_p(), C.c_void_p()
            assert self.hip.hipEventCreate(C.byref(a)) == 0 and self.hip.hipEventCreate(C.byref(b)) == 0
            self.pairs.append((a, b))

    def elapsed_ms(self):
        out = []
        for a, b in self.pairs:
            ms = C.c_float()
            if self.hip.hipEventElapsedTime(C.byref(ms), a, b) == 0:
                out.append(ms.value)
        return out


# --------------------------------------------------------------------------------------------- workloads
def make_model(pv, cfg, dev):
    if cfg["kind"] == "ivae":
        return pv.models.iVAE(cfg["data_dim"], 2, cfg["inv"], seed=1, device=dev)
    if cfg["kind"] == "jivae":
        return pv.models.jiVAE(cfg["data_dim"], 2, cfg["K"], cfg["inv"], seed=1, device=dev)
    if cfg["kind"] == "ivae_conv":
        m = pv.models.iVAE(cfg["data_dim"], 2, cfg["inv"], seed=1, device=dev)
        m.set_encoder(pv.nets.convEncoderNet(cfg["data_dim"], latent_dim=m.z_dim))
        return m
    if cfg["kind"] == "ved":
        return pv.models.VED(cfg["data_dim"], cfg["out_dim"], seed=1, device=dev)
    raise KeyError(cfg["kind"])


def make_oracle(cfg, state):
    from oracle import svi_oracle as orc
    if cfg["kind"] == "ved":
        oc = orc.VedConfig(input_dim=cfg["data_dim"], output_dim=cfg["out_dim"], latent_dim=2)
        return orc.VedOracle(state, oc), 2
    oc = orc.Config(data_dim=cfg["data_dim"], latent_dim=2, invariances=cfg["inv"], discrete_dim=cfg.get("K", 0),
                    conv_encoder=[(32,), (64, 64), (128, 128)] if cfg["kind"] == "ivae_conv" else None)
    return orc.SVIOracle(state, oc), oc.z_dim


def make_data(cfg, n, gen):
    """n samples of the workload: (x,) or (x, y)."""
    if cfg["kind"] == "ved":
        return (torch.rand(n, 1, *cfg["data_dim"], generator=gen), torch.rand(n, 1, *cfg["out_dim"], generator=gen))
    return (torch.rand(n, *cfg["data_dim"], generator=gen),)


def host_cpu_info():
    model, cores = "unknown", set()
    try:
        phys = core = None
        for line in open("/proc/cpuinfo"):
            if line.startswith("model name") and model == "unknown":
                model = line.split(":", 1)[1].strip()
            elif line.startswith("physical id"):
                phys = line.split(":", 1)[1].strip()
            elif line.startswith("core id"):
                core = line.split(":", 1)[1].strip()
            elif not line.strip():
                if phys is not None and core is not None:
                    cores.add((phys, core))
                phys = core = None
    except OSError:
        pass
    return model, (len(cores) or (os.cpu_count() or 1)), (os.cpu_count() or 1)


def cpu_baseline(name, cfg, budget_s=12.0):
    """The CPU oracle (a restatement of the reference's eager-torch path) on the same workload: the best of a few
    thread counts (eager torch does not scale to every hardware thread of a big host on (200704 x 128) operands) for
    ~budget_s seconds, and a 1-thread leg of a few steps."""
    import pyroved_amd as pv
    model_name, n_phys, n_logical = host_cpu_info()
    B = cfg["batch"]
    model = make_model(pv, cfg, "cpu")
    o, z_dim = make_oracle(cfg, model.state_dict())
    data = make_data(cfg, B, torch.Generator().manual_seed(0))
    torch.manual_seed(1)
    eps0 = torch.empty(B, z_dim).normal_()

    def one(eps=None):
        e = torch.empty(B, z_dim).normal_() if eps is None else eps
        return o.step(data[0], data[1], e) if cfg["kind"] == "ved" else o.step(data[0], e)
    torch.set_num_threads(min(16, n_logical))
    loss0 = one(eps0)                          # also the warm-up step
    best_t, best_n, probes = None, None, {}
    for nt in (8, 16, 32, 64, 128):
        if nt > n_logical:
            break
        torch.set_num_threads(nt)
        t0 = time.perf_counter()
        one()
        dt = time.perf_counter() - t0
        probes[nt] = dt
        if best_t is None or dt < best_t:
            best_t, best_n = dt, nt
        if dt > 2.5 * best_t:
            break
    if best_n is None:
        best_n = n_logical
    torch.set_num_threads(best_n)
    t0, n = time.perf_counter(), 0
    while True:
        one()
        n += 1
        el = time.perf_counter() - t0
        if (el > budget_s and n >= 3) or n >= 200:
            break
    torch.set_num_threads(1)
    t1, n1 = time.perf_counter(), 0
    while True:
        one()
        n1 += 1
        el1 = time.perf_counter() - t1
        if el1 > 4.0 or n1 >= 20:
            break
    # ... and every physical core (SURVEY 8d asked for this figure by name; on a 128-core host it is slower than 32 threads)
    torch.set_num_threads(n_phys)
    t2, n2 = time.perf_counter(), 0
    while True:
        one()
        n2 += 1
        el2 = time.perf_counter() - t2
        if el2 > 3.0 or n2 >= 10:
            break
    torch.set_num_threads(best_n)
    return dict(value=n * B / el, unit="images/s", cores=best_n, kind="port",
                sample="%d SVI steps of batch %d (%.1f s) of the same %s workload (%s), eager torch CPU oracle "
                       "(oracle/svi_oracle.py), %d threads = the fastest of the probed thread counts %s"
                       % (n, B, el, name, cfg["desc"], best_n, sorted(probes)),
                ms_per_step=1e3 * el / n, cpu_model=model_name, physical_cores=n_phys, logical_cpus=n_logical,
                thread_probe_ms={str(k): 1e3 * v for k, v in probes.items()},
                one_thread={"value": n1 * B / el1, "unit": "images/s", "cores": 1, "ms_per_step": 1e3 * el1 / n1,
                            "sample": "%d steps (%.1f s)" % (n1, el1)},
                all_physical_cores={"value": n2 * B / el2, "unit": "images/s", "cores": n_phys, "ms_per_step": 1e3 * el2 / n2,
                                    "sample": "%d steps (%.1f s)" % (n2, el2)}), loss0 / B


# --------------------------------------------------------------------------------------------- the timed run
MAX_REGIONS = 40                 # cap on warm-up regions + measured regions of one leg
CONVERGED = 0.01                 # two successive regions within 1 %: the box has stopped warming up


class TorchEvents:
    """torch events on the current stream around the collective (N > 1), every EV_EVERY-th step."""
    def __init__(self):
        self.pairs = []

    def pair(self):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        self.pairs.append((a, b))
        return a, b

    def elapsed_ms(self):
        return [a.elapsed_time(b) for a, b in self.pairs]


def _run(args, cfg, fused, pv, pvdist, td, dev, rank, world, B, attrs=None):
    """warm-up, regions of --steps steps until two successive ones agree to 1 %, then --repeats measured regions, on one
    decoder path.  -> dict(regions (max over ranks, seconds), discarded, kernel ms, conv-kernel ms + flops, all-reduce ms,
    per-step losses (cpu), engine, model)"""
    model = make_model(pv, cfg, dev)
    eng = model.engine(fused=fused)
    for k_, v_ in (attrs or {}).items():           # per-plan switches of the engine (e.g. enc_fold=False: the guide as its own launch)
        setattr(eng, k_, v_)
    if os.environ.get("PV_BENCH_CONV_X3") == "1":  # (A/B: the fp32-class convolutions with both operands split, rounds 2-4's form)
        eng.conv_x3 = True
    multi = world > 1 or FORCE_DIST                 # (FORCE_DIST: the multi-rank code path at world size 1 — test hook)
    comm = None
    if multi:
        pvdist.sync_replicas(eng)
        # the step's one collective: ncclAllReduce enqueued by the LIBRARY on the compute stream (pv_ivae_dp_step / pv_ved_dp_step,
        # ABI v16) on an RCCL communicator of this process; PV_BENCH_COLLECTIVE=torch: torch.distributed.all_reduce (its own
        # stream + two event hand-offs per step) — also what a gloo run (the one-GPU test hook) uses
        if COLLECTIVE["want"] == "native" and pvdist.native_available():
            try:
                comm = pvdist.native_comm(dev)
                COLLECTIVE["used"] = "rccl-native (%s)" % os.path.basename(comm.library)
            except Exception as e:                   # (a measurement harness must still produce its line: say so in it)
                COLLECTIVE["used"] = "torch.distributed (native communicator failed: %s)" % repr(e)[:200]
                comm = None
        else:
            COLLECTIVE["used"] = "torch.distributed"
    ring_n = cfg["ring"]
    gen = torch.Generator().manual_seed(0)
    # synthetic data, resident in HBM before the timed region.  Weak scaling: every rank owns B samples of each of the
    # ring's global minibatches of world*B; strong scaling: the global minibatch is B_global = world*B too (B = global/world)
    data = make_data(cfg, ring_n * world * B, gen)
    data = [t.view(ring_n, world, B, *t.shape[1:])[:, rank].contiguous().to(dev) for t in data]
    full = args.full
    R = max(1, args.repeats) if full else 1
    n_eps = args.warmup + (2 if full else 1) * args.steps    # noise ring (the first warmup + steps draws are the seeded stream)
    torch.manual_seed(1)
    eps_all = torch.empty(n_eps, world, B, model.z_dim).normal_()[:, rank].contiguous().to(dev)
    n_ev = max(1, min(EV_PER_REGION, args.steps)) if full else 0     # (plain run: no events in the timed region)
    ev_at = {min(args.steps - 1, int((2 * j_ + 1) * args.steps / (2 * n_ev))): j_ for j_ in range(n_ev)}   # step index -> sample slot
    events = HipEvents(n_ev * R)                        # one set per measured region (warm-up regions re-record set 0)
    conv = cfg["kind"] in ("ved", "ivae_conv")
    cevents = HipEvents(n_ev * R) if conv else None
    preroll_env = os.environ.get("PV_BENCH_PREROLL")            # (experiments: a fixed count)
    preroll_n = [int(preroll_env) if (preroll_env is not None and full) else 0]   # set after the first region (its step time is the estimate)
    cflops = C.c_double(0.0)
    arev = TorchEvents()
    hist = torch.zeros(n_eps, 4, device=dev)
    ved = cfg["kind"] == "ved"
    one_call = not multi and not args.two_call and getattr(eng, "supports_step", False)

    def reduce_(t):
        if comm is not None:
            comm.allreduce_sum_(t)
        else:
            pvdist.allreduce_sum_(t)

    def step(i, ev=None, cev=None, ar=None):
        eng.events = ev if ev is not None else (None, None)
        eng.conv_events = (cev[0], cev[1], cflops) if cev is not None else None
        k = i % n_eps
        x = data[0][i % ring_n]
        if ar is not None:
            ar = arev.pair()
        if multi and comm is not None and not ar:
            # the data-parallel step as ONE library call: shard gradients -> ncclAllReduce([grads | 4 scalars]) -> Adam + history
            if ved:
                eng.loss_and_grads(x, eps_all[k], 1.0, data[1][i % ring_n], step=True, comm=comm, hist_out=hist[k])
            else:
                eng.loss_and_grads(x, eps_all[k], step=True, comm=comm, hist_out=hist[k])
        elif multi:
            # (torch.distributed's collective, or a sampled step of the native one: the same three enqueues on the same stream as
            #  three calls, with events around the collective)
            if ved:
                eng.loss_and_grads(x, eps_all[k], 1.0, data[1][i % ring_n])
            else:
                eng.loss_and_grads(x, eps_all[k])
            if ar: ar[0].record()
            reduce_(eng.grad)                         # gradients + the 4 loss scalars in one collective
            if ar: ar[1].record()
            if hasattr(eng, "adam_step_hist"):
                eng.adam_step_hist(hist[k])           # Adam + the history write in one launch; no host sync anywhere
            else:
                hist[k].copy_(eng.scalars)
                eng.adam_step()
        elif ved:
            eng.loss_and_grads(x, eps_all[k], 1.0, data[1][i % ring_n], scalars_out=hist[k])
            eng.adam_step()
        elif one_call:
            # single process: SVI.step as ONE library call (pv_ivae_step: ELBO + gradients + Adam; bit-identical to
            # the two calls, tests/test_gpu_parity.py)
            eng.loss_and_grads(x, eps_all[k], scalars_out=hist[k], step=True)
        else:
            eng.loss_and_grads(x, eps_all[k], scalars_out=hist[k])
            eng.adam_step()

    def free_pass():
        if ved:
            eng.loss_and_grads(data[0][0], eps_all[0], 1.0, data[1][0])
        else:
            eng.loss_and_grads(data[0][0], eps_all[0])

    # one untimed, state-free pass first (gradients only, no optimizer update, no collective on real data): module
    # loading and first-launch costs never land in a timed region, whatever --warmup is
    free_pass()
    if multi:
        reduce_(torch.zeros_like(eng.grad))
    for i in range(args.warmup):
        step(i)
    torch.cuda.synchronize()
    losses_head = hist[:, 0].cpu().clone()             # (steps 0 .. warmup-1 of the seeded stream; later slots are reused)

    first_after = {"t": None}                           # loss of the first step after the warm-up (= step 0 when --warmup 0)

    def note_first(i):
        if first_after["t"] is None:
            first_after["t"] = hist[i % n_eps, 0].clone()

    def region(base, slot=0):
        for i in range(preroll_n[0]):                   # (untimed; the noise ring wraps, the optimizer state moves on)
            step(base + i)
            note_first(base + i)
        if multi:
            td.barrier()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i in range(args.steps):
            sample = i in ev_at
            j = slot * n_ev + ev_at.get(i, 0)
            step(base + i, events.pairs[j] if sample else None, cevents.pairs[j] if (sample and conv) else None,
                 True if (i % EV_EVERY == 0 and multi and full) else None)
            note_first(base + i)
        if multi:
            td.barrier()
        torch.cuda.synchronize()
        t = torch.tensor([time.perf_counter() - t0], device=dev, dtype=torch.float64)
        if multi:
            td.all_reduce(t, op=td.ReduceOp.MAX)
        return t.item()

    if not full:
        # the plain run: the fixed preroll, then exactly --steps timed steps
        for _ in range(PREROLL_PASSES):
            free_pass()
        t = region(args.warmup)
        losses_first = hist[:, 0].cpu().clone()
        base = args.warmup + args.steps
        return dict(regions=[t], discarded=0, all_regions=[t], kms=[], cms=[], conv_flops=0.0, ar_ms=[],
                    losses_head=losses_head, losses_first=losses_first, first_after_warmup=first_after["t"].item(),
                    preroll=PREROLL_PASSES, ev_samples_per_region=0, last_loss=hist[(base - 1) % n_eps, 0].item(),
                    outputs=_outputs(args, model, hist, base, n_eps), eng=eng, model=model)
    all_regions, base = [], args.warmup
    first = region(base)
    if preroll_env is None:                             # (max over ranks already: the same count everywhere)
        preroll_n[0] = max(0, min(PREROLL_MAX, int(PREROLL_MS * 1e-3 / max(first / args.steps, 1e-9) + 0.999)))
    losses_first = hist[:, 0].cpu().clone()            # slot `warmup` = the first timed step
    all_regions.append(first)
    base += args.steps
    # warm-up regions: until two successive ones agree (decided on the max-over-ranks time, identical on every rank)
    while len(all_regions) < MAX_REGIONS - R:
        r = region(base)
        base += args.steps
        all_regions.append(r)
        if abs(all_regions[-1] - all_regions[-2]) <= CONVERGED * all_regions[-1]:
            break
    discarded = len(all_regions) - 1                   # the last converged region is the first measured one
    regions = [all_regions[-1]]
    arev.pairs.clear()
    for k_ in range(R - 1):
        regions.append(region(base, k_ + 1))
        base += args.steps
    torch.cuda.synchronize()
    return dict(regions=regions, discarded=discarded, all_regions=all_regions + regions[1:],
                kms=events.elapsed_ms() if not ved else [], cms=cevents.elapsed_ms() if conv else [],
                conv_flops=cflops.value, ar_ms=arev.elapsed_ms(), losses_head=losses_head, losses_first=losses_first,
                first_after_warmup=first_after["t"].item(), preroll=preroll_n[0], ev_samples_per_region=n_ev,
                last_loss=hist[(base - 1) % n_eps, 0].item(), outputs=_outputs(args, model, hist, base, n_eps),
                eng=eng, model=model)


DUMP_MAX_BYTES = 64 << 20        # --dump-outputs: at most this much in all
DUMP_SAMPLE = 1 << 20            # an array of more elements is written as a fixed, seeded sample of this many


def _outputs(args, model, hist, base, n_eps):
    """(--dump-outputs) what the caller of the timed path holds after its last step (step index base - 1): name -> numpy array."""
    if not args.dump_outputs:
        return None
    import numpy as np
    torch.cuda.synchronize()
    slots = [(base - args.steps + i) % n_eps for i in range(args.steps)]
    out = {"loss_per_step": hist[slots, 0].double().cpu().numpy(),
           "loss_terms": hist[(base - 1) % n_eps].double().cpu().numpy()}
    for k, v in model.state_dict().items():
        a = v.detach().cpu()
        a = (a.float() if a.is_floating_point() else a.double()).numpy()
        if a.size > DUMP_SAMPLE:
            idx = np.sort(np.random.default_rng(0).choice(a.size, DUMP_SAMPLE, replace=False))
            a = a.reshape(-1)[idx]
        out["param." + k] = a
    return out


def write_outputs(d, arrays):
    import numpy as np
    total = sum(a.nbytes for a in arrays.values())
    if total > DUMP_MAX_BYTES:
        raise SystemExit("--dump-outputs: %d bytes, over the %d-byte cap" % (total, DUMP_MAX_BYTES))
    os.makedirs(d, exist_ok=True)
    for k, a in arrays.items():
        np.save(os.path.join(d, k + ".npy"), a)


def _kernel_name(fused, units, grads=1, lik=0, fold=False):
    """The name rocprofv3 prints for the decoder kernel the library dispatches (a debug export of the library)."""
    from pyroved_amd import _abi
    lib = C.CDLL(_abi.LIB_PATH)
    if fold:
        lib.pv_debug_decoder_kernel_name_fold.restype = C.c_char_p
        lib.pv_debug_decoder_kernel_name_fold.argtypes = [C.c_int, C.c_int]
        return lib.pv_debug_decoder_kernel_name_fold(grads, lik).decode()
    lib.pv_debug_decoder_kernel_name.restype = C.c_char_p
    lib.pv_debug_decoder_kernel_name.argtypes = [C.c_int, C.c_int64, C.c_int, C.c_int]
    return lib.pv_debug_decoder_kernel_name(fused, units, grads, lik).decode()


def _paths(cfg, mode, B, n_pix, fold=False):
    """(kernel name, flops per launch, peak TF, dtype label, arithmetic description) of the dominant decoder kernel."""
    passes = max(cfg["dec_passes"], 1)
    dec_fl = DEC_FLOP_PER_PIXEL * n_pix * passes * B
    units = B * n_pix * passes // 16
    if mode == 2:
        kn = _kernel_name(2, units)
        # round 4: training launches of the fp32-class path run an fp16 build from 16 384 rows up (last template argument of
        # pv_sdec_fused_bf16_kernel: 8 = H231, 2 = H221, 1 = the bf16 three-product kernel; pv_sdec_fused_bf16.hip)
        prec = kn.split(",")[-1].split(">")[0].strip() if "pv_sdec_fused_bf16_kernel" in kn else "1"
        if prec == "8":
            return (kn, dec_fl, MFMA_BF16_PEAK_TFLOPS, "f16w2",
                    "f16 MFMA: weights as two exact power-of-two-scaled fp16 pieces, activations one piece (forward 2 products, "
                    "dgrad 3 with dL/dpre split, wgrad 1; fp32 accumulate; fp32 elsewhere): every gradient within 1e-4 of the oracle")
        if prec == "2":
            return (kn, dec_fl, MFMA_BF16_PEAK_TFLOPS, "f16w2",
                    "f16 MFMA: weights as two exact power-of-two-scaled fp16 pieces, activations and dL/dpre one piece (forward 2 "
                    "products, dgrad 2, wgrad 1; fp32 accumulate; fp32 elsewhere); selected from 524 288 decoder rows up")
        return (kn, dec_fl, MFMA_BF16_PEAK_TFLOPS, "bf16x3",
                "bf16 split-precision MFMA (hi+lo, 3 products, fp32 accumulate; fp32 elsewhere)")
    if mode == 3:
        return (_kernel_name(3, units, fold=fold), dec_fl, MFMA_BF16_PEAK_TFLOPS, "bf16",
                "bf16 MFMA operands for the hidden-layer contractions (fp32 accumulate; fp32 elsewhere)"
                + ("; the guide (fc encoder, sample, split) runs in the decoder launch's prologue in fp32" if fold else ""))
    if mode == 1:
        return (_kernel_name(1, units), dec_fl, MFMA_F32_PEAK_TFLOPS, "f32", "fp32 (f32-input MFMA)")
    return ("pv_gemm_kernel<NT> (decoder hidden layer fwd, M=B*N, K=N=128)", 2.0 * B * n_pix * 128 * 128 * passes,
            MFMA_F32_PEAK_TFLOPS, "f32", "fp32 (f32-input MFMA)")


def _traffic(key, B, cfg):
    tr = TRAFFIC.get(key) if B == cfg["batch"] else None
    return (tr[0] if tr else None,
            (tr[1] + " (committed rocprofv3 --pmc pass of this config, not collected by this run)") if tr else None)


def measure(args, name, cfg, fused, ctx, attrs=None):
    """One decoder path of one config -> dict of numbers."""
    pv, pvdist, td, dev, rank, world, B = ctx
    r = _run(args, cfg, fused, pv, pvdist, td, dev, rank, world, B, attrs)
    regions, eng = r["regions"], r["eng"]
    med = statistics.median(regions)
    n_pix = 1
    for d in cfg["data_dim"]:
        n_pix *= d
    ved = cfg["kind"] == "ved"
    out = {"regions_s": regions, "median_s": med, "ms_per_step": 1e3 * med / args.steps,
           "ms_per_step_all": [1e3 * v / args.steps for v in regions],
           "regions_discarded": r["discarded"],
           "ms_per_step_warming": [1e3 * v / args.steps for v in r["all_regions"][:r["discarded"]]],
           "value": args.steps * B * world / med,
           "loss_per_image_step0": (r["losses_head"][0].item() if args.warmup > 0 else r["first_after_warmup"]) / (B * world),
           "preroll_steps": r["preroll"], "kernel_event_samples_per_region": r["ev_samples_per_region"],
           "loss_per_image_first_timed_step": r["losses_first"][args.warmup].item() / (B * world),
           "loss_per_image_last_step": r["last_loss"] / (B * world), "outputs": r["outputs"]}
    if (world > 1 or FORCE_DIST) and r["ar_ms"]:
        out["collective"] = COLLECTIVE["used"]
        out["allreduce_ms"] = sum(r["ar_ms"]) / len(r["ar_ms"])
        out["allreduce_ms_samples"] = len(r["ar_ms"])
        # one bucket, issued after the step's last gradient launch and followed by Adam: nothing runs beside it on this rank,
        # so the collective's whole duration is exposed (why a second bucket would not pay)
        out["allreduce_exposed_ms"] = out["allreduce_ms"]
    step_tf = out["value"] / world * cfg["flops_per_image"] / 1e12
    out["step_algorithmic_tflops"] = step_tf
    conv_roof = None
    if r["cms"] and r["conv_flops"] > 0:
        # the heaviest kernel-3 convolution launch of the encoder's forward (64 -> 64 channels at 32x32 in the default stack,
        # max-pool in its epilogue), event-timed inside the step: split operands, three matrix instructions per multiply-add
        c_avg = sum(r["cms"]) / len(r["cms"])
        c_tf = r["conv_flops"] / (c_avg * 1e-3) / 1e12
        bf = fused == 3
        tb, ts = _traffic("%s:%d:conv" % (name, fused), B, cfg)
        conv_roof = {"bound": "mfma", "achieved": c_tf, "peak": MFMA_BF16_PEAK_TFLOPS, "unit": "TFLOP/s",
                     "frac": c_tf / MFMA_BF16_PEAK_TFLOPS, "traffic": tb, "traffic_source": ts,
                     "kernel": "void pv_conv3_sp_kernel<%d, 4, true>(ConvSp)" % (1 if bf else 2),
                     "what": "heaviest kernel-3 convolution of the encoder forward (most multiply-adds), with its max-pool "
                             "epilogue; " + ("ONE fp16 piece per operand (power-of-two scaled per staged tile), one product per "
                                             "multiply-add: the throughput precision" if bf else
                                             "operands split in two fp16 pieces (exact power-of-two scaling), 3 products per "
                                             "multiply-add"),
                     "kernel_ms": c_avg, "kernel_ms_samples": len(r["cms"]), "flops_per_launch": r["conv_flops"],
                     "mfma_products_per_mac": 1 if bf else 3,
                     "frac_of_split_operand_peak": (1 if bf else 3) * c_tf / MFMA_BF16_PEAK_TFLOPS}
    if ved:
        # both precisions run the 2-D k3 convolutions on the 16x16x32 f16 matrix-core instruction (pv_conv_sp.hip): fp32-class =
        # two fp16 pieces with exact power-of-two scaling per staged tile, three products (~2^-22 per product); throughput
        # (round 4; SVItrainer(precision="bf16")) = ONE fp16 piece per operand, one product
        bf = fused == 3
        out.update(dtype="f16" if bf else "f16x3", path="conv-f16" if bf else "conv-f16x3",
                   arith=("2-D k3 convolutions on the f16 MFMA with ONE fp16 piece per operand (power-of-two scaled per staged "
                          "tile), one product per multiply-add (fp32 accumulate); 1-D convolutions on the f32-input MFMA; fp32 "
                          "elsewhere" if bf else
                          "2-D k3 convolutions on the f16 MFMA, operands as fp16 pieces with exact power-of-two scaling per staged "
                          "tile: FORWARD both operands two pieces, three products (3e-7 relative l2 vs float64: its outputs pick "
                          "max-pool winners); INPUT GRADIENT the same three products (round 6: one-piece dL/dy accumulated down the "
                          "chain to 1.6e-4 under equal forward decisions); WEIGHT GRADIENT one piece per operand, one product "
                          "(5..8e-5 on its own tensor) — every gradient within 1e-4 of float64 under the HIP forward's own "
                          "decisions, three draws (fp32 accumulate); 1-D convolutions on the f32-input MFMA; fp32 elsewhere"))
        out["roofline"] = conv_roof if conv_roof else {"bound": "mfma", "achieved": 0.0, "peak": MFMA_BF16_PEAK_TFLOPS,
                                                       "unit": "TFLOP/s", "frac": 0.0, "traffic": None, "kernel": "n/a"}
        out["roofline_step"] = {"bound": "mfma", "scope": "step", "achieved": step_tf, "peak": MFMA_BF16_PEAK_TFLOPS,
                                "unit": "TFLOP/s", "frac": step_tf / MFMA_BF16_PEAK_TFLOPS,
                                "flops_per_step": cfg["flops_per_image"] * B}
        return out
    mode = fused if eng.uses_fused(B) else 0
    fold = False
    if mode == 3 and hasattr(eng, "_plan"):
        try:
            from pyroved_amd import _abi
            fold = bool(_abi.lib().pv_ivae_guide_folds(C.byref(eng._plan(B))))
        except Exception:
            fold = False
    kname, fl, peak, dtype, arith = _paths(cfg, mode, B, n_pix, fold)
    out["guide_folded"] = fold
    kms = r["kms"]
    k_avg = sum(kms) / max(len(kms), 1)
    achieved = fl / (k_avg * 1e-3) / 1e12 if k_avg > 0 else 0.0
    tb, ts = _traffic("%s:%d" % (name, mode), B, cfg)
    out.update(dtype=dtype, arith=arith, path={0: "layered", 1: "fused-f32", 2: "fused-" + dtype, 3: "fused-bf16"}[mode],
               roofline={"bound": "mfma", "achieved": achieved, "peak": peak, "unit": "TFLOP/s", "frac": achieved / peak,
                         "traffic": tb, "traffic_source": ts,
                         "kernel": kname, "kernel_ms": k_avg, "kernel_ms_samples": len(kms), "flops_per_launch": fl})
    if conv_roof:
        out["roofline_conv"] = conv_roof
    return out


def sub_config(name, args):
    """Times another config in its own process (N = 1) and returns its compact record."""
    cmd = [sys.executable, os.path.abspath(__file__), "--config", name, "--steps", str(args.sub_steps), "--warmup", "10",
           "--full", "--repeats", "3", "--no-cpu-baseline", "--no-configs"]
    try:
        p = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
        line = [l for l in p.stdout.splitlines() if l.startswith("{")][-1]
        d = json.loads(line)
        rec = {"config": name, "workload": d["config"]["workload"], "n_gpus": 1, "dtype": d["dtype"],
               "ms_per_step": d["ms_per_step"], "ms_per_step_all": d["ms_per_step_all"],
               "regions_discarded": d.get("regions_discarded"), "value": d["value"],
               "unit": d["unit"], "roofline": d["roofline"], "step_algorithmic_tflops": d.get("step_algorithmic_tflops"),
               "loss_per_image_step0": d["elbo"]["loss_per_image_step0"]}
        for k in ("roofline_conv", "roofline_step", "fp32_class", "throughput_precision"):
            if k in d:
                rec[k] = d[k]
        return rec
    except Exception as e:       # a failed side measurement must not take the headline line down
        return {"config": name, "error": repr(e)[:300]}


def trainer_leg(pv, dev):
    """What a user of the reference API calls: SVItrainer.step(train_loader) with a CPU DataLoader handed over
    (trainers/svi.py:139-162), images/s INCLUDING the feed — 61 440 images of the headline model, batch 256, one warm-up
    epoch (uploads the dataset, builds the engine), then 3 timed epochs; both precisions."""
    n, B, epochs = 61440, 256, 3
    x = torch.rand(n, 28, 28, generator=torch.Generator().manual_seed(0))
    out = {"images": n, "batch": B, "epochs": epochs, "unit": "images/s",
           "what": "SVItrainer.step(init_dataloader(x, batch_size=256)) on iVAE 28x28 ['r','t']: shuffling DataLoader's order "
                   "and the CPU generator's noise stream reproduced, dataset resident on the device after the first epoch"}
    for precision in ("bf16", "fp32"):
        model = pv.models.iVAE((28, 28), 2, ["r", "t"], seed=1, device=dev)
        loader = pv.utils.init_dataloader(x, batch_size=B)
        tr = pv.trainers.SVItrainer(model, seed=1, precision=precision)
        tr.step(loader)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(epochs):
            tr.step(loader)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        out[precision] = {"value": n * epochs / dt, "ms_per_step": 1e3 * dt / (epochs * (n // B)),
                          "loss_per_image_last_epoch": tr.loss_history["training_loss"][-1]}
        del tr, model
    return out


def inference_leg(pv, dev):
    """encode() and decode() of the headline model through the reference API (models/base.py:121-171): 65 536 samples in
    loader batches of 4096, results on the CPU as the API returns them (one device -> host copy per call), and the kernels'
    own rate (inputs and outputs on the device).  decode runs the fused decoder kernel forward-only at fp32-class
    precision (split-precision MFMA); encode the fc encoder's GEMM kernels."""
    n, bs = 65536, 4096
    model = pv.models.iVAE((28, 28), 2, ["r", "t"], seed=1, device=dev)
    x = torch.rand(n, 28, 28, generator=torch.Generator().manual_seed(0))
    z = torch.randn(n, 2, generator=torch.Generator().manual_seed(1))
    model.encode(x[:bs], batch_size=bs); model.decode(z[:bs], batch_size=bs)           # warm-up
    out = {"samples": n, "batch_size": bs, "unit": "images/s"}
    for what, fn in (("encode_api", lambda: model.encode(x, batch_size=bs)), ("decode_api", lambda: model.decode(z, batch_size=bs))):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out[what] = n / (time.perf_counter() - t0)
    eng = model.engine()
    xg, zg = x[:32768].to(dev), z[:32768].to(dev)
    for what, fn in (("encode_device", lambda: eng.encode(xg)), ("decode_device", lambda: eng.decode(zg))):
        fn()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(5):
            fn()
        torch.cuda.synchronize()
        out[what] = 5 * 32768 / (time.perf_counter() - t0)
    from pyroved_amd import _abi
    out["decode_workspace_bytes_b32768"] = int(_abi.lib().pv_ivae_workspace_bytes_for(C.byref(eng._plan(32768, what=3)), 3))
    out["decode_kernel"] = _kernel_name(2, 32768 * 784 // 16, grads=0)
    return out


def headline(args, name, cfg, leg, world, B):
    """The result line's contract fields (a plain run prints these alone)."""
    return {
        "metric": "images/sec (SVI step)", "value": leg["value"], "unit": "images/s", "n_gpus": world,
        "steps": args.steps, "warmup": args.warmup, "ms_per_step": leg["ms_per_step"],
        "higher_is_better": True, "scaling": "strong" if args.strong else "weak", "vs_baseline": None,
        "dtype": leg["dtype"], "data": "synthetic",
        "config": {"workload": "%s %s, batch %d per GPU (global %d), %s, SVI step = ELBO+grads+%sAdam"
                               % (name, cfg["desc"], B, B * world, leg["arith"], "allreduce+" if world > 1 else ""),
                   "parallelism": "dp%d" % world, "path": leg["path"], "baseline_config": name},
        "elbo": {k: leg[k] for k in ("loss_per_image_first_timed_step", "loss_per_image_last_step", "loss_per_image_step0")},
        "timing": {"preroll_passes": PREROLL_PASSES,
                   "note": "one timed region of exactly --steps steps after --warmup steps and preroll_passes gradient-only "
                           "passes; --full for the repeated regions, the other precision, rooflines and the side measurements"},
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--full", action="store_true",
                    help="everything besides the headline figure: the other precision leg, repeated regions, rooflines, the CPU "
                         "baseline, the trainer / inference legs, the side configs (N = 1), both scalings (N > 1)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write what the timed path computed in its last step to DIR/<name>.npy")
    ap.add_argument("--repeats", type=int, default=5, help="(--full) timed regions of --steps steps; the median is reported")
    ap.add_argument("--config", default="C2", choices=sorted(CONFIGS))
    ap.add_argument("--no-legs", action="store_true", help="skip the trainer / inference legs of the default N=1 run")
    ap.add_argument("--strong", action="store_true", help="strong scaling: the config's batch is the GLOBAL batch, sharded")
    ap.add_argument("--fused", type=int, default=None,
                    help="lead path: 0 layered, 1 fused f32 MFMA, 2 fp32-class (every gradient to 1e-4: the reference's precision), "
                         "3 throughput precision (bf16 / one fp16 piece).  Default: 3 for C2 (BASELINE configs[1] names bf16), "
                         "2 for every other config (BASELINE names no dtype there and the reference is fp32 end to end)")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-alt", action="store_true", help="skip the second leg (the fp32-class path)")
    ap.add_argument("--no-configs", action="store_true", help="skip the side measurements of C1, C3, C4, C5")
    ap.add_argument("--sub-steps", type=int, default=40)
    ap.add_argument("--batch", type=int, default=None, help="per-GPU batch override (weak) / global batch (--strong)")
    ap.add_argument("--two-call", action="store_true", help="N=1: pv_ivae_loss_and_grads + pv_adam_step instead of pv_ivae_step")
    args = ap.parse_args()

    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if args.gpus > 1 and world != args.gpus:
        raise SystemExit("--gpus %d needs torch.distributed.run with --nproc-per-node %d" % (args.gpus, args.gpus))
    # test hook (one-GPU boxes): PV_BENCH_BACKEND=gloo PV_BENCH_ONE_DEVICE=1 runs all ranks on cuda:0 over gloo, to
    # exercise the multi-rank code path end to end where no second GPU exists; the numbers then mean nothing
    backend = os.environ.get("PV_BENCH_BACKEND", "nccl")
    if os.environ.get("PV_BENCH_ONE_DEVICE"):
        local_rank = 0
    torch.cuda.set_device(local_rank)
    dev = torch.device("cuda", local_rank)
    import torch.distributed as td
    if world > 1 or FORCE_DIST:
        if FORCE_DIST:
            os.environ.setdefault("MASTER_ADDR", "127.0.0.1"); os.environ.setdefault("MASTER_PORT", "29533")
            os.environ.setdefault("RANK", "0"); os.environ.setdefault("WORLD_SIZE", "1")
        if backend == "nccl":
            td.init_process_group("nccl", device_id=dev)
        else:
            td.init_process_group(backend)

    import pyroved_amd as pv
    from pyroved_amd import dist as pvdist

    name = args.config
    cfg = CONFIGS[name]
    b_cfg = args.batch if args.batch is not None else cfg["batch"]
    if args.strong:
        if b_cfg % world:
            raise SystemExit("--strong: the global batch %d is not divisible by %d ranks" % (b_cfg, world))
        B = b_cfg // world
    else:
        B = b_cfg
    ctx = (pv, pvdist, td, dev, rank, world, B)

    if args.fused is None:
        args.fused = int(os.environ.get("PV_BENCH_FUSED", "3" if name == "C2" else "2"))
    main_leg = measure(args, name, cfg, args.fused, ctx)
    outputs = main_leg.pop("outputs")
    if outputs is not None and rank == 0:
        write_outputs(args.dump_outputs, outputs)
    if not args.full:
        if rank == 0:
            print(json.dumps(headline(args, name, cfg, main_leg, world, B)))
            sys.stdout.flush()
        if world > 1 or FORCE_DIST:
            pvdist.close_native()
            td.destroy_process_group()
        return
    alt = None
    if args.fused in (2, 3) and not args.no_alt:
        alt = measure(args, name, cfg, 5 - args.fused, ctx)      # the same workload on the other precision
    unfolded = None
    if main_leg.get("guide_folded") and not args.no_alt:
        # the decoder launch hosts the guide: its duration is no longer the decoder's alone.
        # The same workload with the guide as its own launch gives the decoder-only kernel time / fraction next to it
        unfolded = measure(args, name, cfg, args.fused, ctx, attrs={"enc_fold": False})
    # which leg is the fp32-class one (the reference's precision: what C1 / C3 / C4 / C5 lead with) and which the throughput one
    fp32_leg = main_leg if args.fused == 2 else (alt if args.fused == 3 else None)
    alt_key = "fp32_class" if args.fused == 3 else "throughput_precision"
    strong = None
    if world > 1 and not args.strong and b_cfg % world == 0 and not args.no_alt:
        # N > 1: the other scaling too — the config's batch as the GLOBAL batch, sharded (at batch 256 / 28x28 this is
        # latency-bound by design: 32 images per GPU at N = 8; DESIGN.md section 6 has the expected curve)
        strong = measure(args, name, cfg, args.fused, (pv, pvdist, td, dev, rank, world, b_cfg // world))
    c5w = None
    if (world > 1 or FORCE_DIST) and name == "C2" and not args.strong and args.batch is None and not args.no_alt:
        # N > 1: the conv config too (weak scaling, 256 images per GPU) — its 0.75 ms step hides the all-reduce's latency far
        # better than C2's 0.12 ms, so it is the config whose curve can reach the >= 6x target
        try:
            c5w = measure(args, "C5", CONFIGS["C5"], 2, (pv, pvdist, td, dev, rank, world, CONFIGS["C5"]["batch"]))
        except Exception as e:                   # (must not take the headline line down)
            c5w = {"error": repr(e)[:300]}
    if rank == 0:
        out = headline(args, name, cfg, main_leg, world, B)
        del out["elbo"], out["timing"]
        out.update({
            "repeats": len(main_leg["regions_s"]), "ms_per_step_all": main_leg["ms_per_step_all"],
            "regions_discarded": main_leg["regions_discarded"], "ms_per_step_warming": main_leg["ms_per_step_warming"],
            "timing": {"preroll_steps": main_leg["preroll_steps"],
                       "kernel_event_samples_per_region": main_leg["kernel_event_samples_per_region"],
                       "note": "every timed region (exactly --steps steps between two synchronisations) is preceded by "
                               "preroll_steps untimed steps (~10 ms of them, at most 100; none before the first, discarded region) enqueued "
                               "back to back: after the idle gap between regions a 2 ms region ran at a colder GPU's clocks (step 0.1091 vs 0.1049 ms, profiles/r05ay_*); launches "
                               "carrying HIP events cost the stream ~11 us each, so one launch per region (mid-region) is sampled and "
                               "the measured regions' samples pooled"},
            "ms_per_step_spread": (max(main_leg["ms_per_step_all"]) - min(main_leg["ms_per_step_all"])),
            "roofline": main_leg["roofline"],
            "step_algorithmic_tflops": main_leg.get("step_algorithmic_tflops"),
            "elbo": {k: main_leg[k] for k in ("loss_per_image_first_timed_step", "loss_per_image_last_step",
                                              "loss_per_image_step0")},
        })
        for k in ("roofline_conv", "roofline_step", "allreduce_ms", "allreduce_ms_samples", "allreduce_exposed_ms", "collective"):
            if k in main_leg:
                out[k] = main_leg[k]
        # driver-visible scalars inside `roofline` (a key the driver's record keeps): the step-level fraction of the lead leg and
        # the fp32-class leg's step time / kernel fraction / step fraction, whichever leg that is
        out["roofline"] = dict(out["roofline"])
        out["roofline"]["step_frac"] = main_leg["step_algorithmic_tflops"] / MFMA_BF16_PEAK_TFLOPS
        if unfolded is not None:
            out["roofline"]["note"] = ("this launch also runs the guide (fc encoder, sample, split, fc_latent: fp32 matrix-vector "
                                       "products, no matrix-core work) and, since round 6, every image's latent backward + encoder "
                                       "input-gradient chain in its epilogue; decoder_only_* = the same workload with the guide and "
                                       "the latent backward in launches of their own (PV_PLAN_NO_ENC_FOLD)")
            out["roofline"]["decoder_only_kernel"] = unfolded["roofline"].get("kernel")
            out["roofline"]["decoder_only_kernel_ms"] = unfolded["roofline"].get("kernel_ms")
            out["roofline"]["decoder_only_frac"] = unfolded["roofline"].get("frac")
            out["unfolded"] = {"ms_per_step": unfolded["ms_per_step"], "value": unfolded["value"], "unit": "images/s",
                               "launches": "pv_enc_kernel, pv_sdec_w8_kernel, pv_latent_bwd_reduce_kernel, pv_wgrad_small_kernel"}
        if fp32_leg is not None:
            out["roofline"]["fp32_class_ms"] = fp32_leg["ms_per_step"]
            out["roofline"]["fp32_class_frac"] = fp32_leg["roofline"]["frac"]
            out["roofline"]["fp32_class_step_frac"] = fp32_leg["step_algorithmic_tflops"] / MFMA_BF16_PEAK_TFLOPS
        if alt is not None:
            out[alt_key] = {"path": alt["path"], "dtype": alt["dtype"], "value": alt["value"], "unit": "images/s",
                                 "ms_per_step": alt["ms_per_step"], "ms_per_step_all": alt["ms_per_step_all"],
                                 "regions_discarded": alt["regions_discarded"],
                                 "kernel": alt["roofline"].get("kernel"),
                                 "kernel_ms": alt["roofline"].get("kernel_ms"), "roofline_frac": alt["roofline"]["frac"],
                                 "roofline_traffic": alt["roofline"].get("traffic"),
                                 "loss_per_image_step0": alt["loss_per_image_step0"]}
            if "roofline_conv" in alt:
                out[alt_key]["roofline_conv"] = alt["roofline_conv"]
            if "allreduce_ms" in alt:
                out[alt_key]["allreduce_ms"] = alt["allreduce_ms"]
        if strong is not None:
            out["strong"] = {"scaling": "strong", "global_batch": b_cfg, "batch_per_gpu": b_cfg // world,
                             "value": strong["value"], "unit": "images/s", "ms_per_step": strong["ms_per_step"],
                             "ms_per_step_all": strong["ms_per_step_all"], "allreduce_ms": strong.get("allreduce_ms"),
                             "kernel_ms": strong["roofline"].get("kernel_ms"),
                             "note": "latency-bound by design at this size (launch chain + one all-reduce per step vs a few "
                                     "microseconds of decoder work per GPU): weak scaling is the curve that can reach the "
                                     ">= 6x target"}
        if c5w is not None:
            out["c5_weak"] = c5w if "error" in c5w else {
                "config": "C5", "scaling": "weak", "batch_per_gpu": CONFIGS["C5"]["batch"], "value": c5w["value"],
                "unit": "images/s", "ms_per_step": c5w["ms_per_step"], "ms_per_step_all": c5w["ms_per_step_all"],
                "allreduce_ms": c5w.get("allreduce_ms"), "dtype": c5w["dtype"]}
        if world > 1:
            # what DESIGN.md section 6 expects on 8 GPUs of one node (no hardware run before round 4): the driver computes the
            # measured x from its own per-N runs; these are the predictions to hold them against
            out["expected_x8"] = {"c2_weak": "5.1-5.9 (one ncclAllReduce of 0.6 MB, ~30-50 us, enqueued by the library between the last "
                                             "gradient launch and the Adam launch of a 0.098 ms step: latency-bound on xGMI; 6x needs <= 32 us "
                                             "for collective + Adam)",
                                  "c2_fp32_class_weak": "6.1-6.6 (0.175 ms step)",
                                  "c5_weak": "~7.4 (2.3 MB per 0.76-0.80 ms step)", "c2_strong": "1.1-1.3 (latency-bound by design)"}
        if world == 1 and not args.no_cpu_baseline:
            cb, loss0 = cpu_baseline(name, cfg)
            out["cpu_baseline"] = cb
            out["elbo"]["oracle_loss_per_image_step0"] = loss0
            if B == cfg["batch"]:
                out["elbo"]["rel_err_step0"] = abs(out["elbo"]["loss_per_image_step0"] - loss0) / abs(loss0)
        default_run = world == 1 and name == "C2" and not args.strong and args.batch is None
        if default_run and not args.no_legs:
            del main_leg, alt
            torch.cuda.empty_cache()
            try:
                out["trainer"] = trainer_leg(pv, dev)
            except Exception as e:
                out["trainer"] = {"error": repr(e)[:300]}
            try:
                out["inference"] = inference_leg(pv, dev)
            except Exception as e:
                out["inference"] = {"error": repr(e)[:300]}
        if default_run and not args.no_configs:
            # release this process's device memory first, then one short process per side config
            main_leg = alt = None
            torch.cuda.empty_cache()
            out["configs"] = [sub_config(c, args) for c in ("C1", "C3", "C4", "C4fc", "C5")]
            #  the per-config headline scalars also INSIDE `roofline`, the one object the driver's record
            # keeps whole: ms per step, the arithmetic the leg computes in, the dominant kernel's and the step's fraction of peak
            rc = {}
            for c in out["configs"]:
                if isinstance(c, dict) and "ms_per_step" in c:
                    rl = c.get("roofline") or {}
                    rc[str(c["config"])] = {
                        "ms_per_step": round(c["ms_per_step"], 5), "dtype": c.get("dtype"), "images_s": round(c["value"]),
                        "kernel": rl.get("kernel"), "kernel_ms": rl.get("kernel_ms"), "frac": rl.get("frac"),
                        "step_frac": (c.get("roofline_step") or {}).get("frac", rl.get("step_frac")),
                        "conv_frac": (c.get("roofline_conv") or {}).get("frac"),
                        "throughput_ms_per_step": (c.get("throughput_precision") or {}).get("ms_per_step")}
            out["roofline"]["configs"] = rc
        # the side legs' headline scalars at the FRONT of the line (the driver's record keeps the known keys and the last 2 000
        # characters) and once more as a short line on stderr, which ends the captured output
        summ = {}
        if "fp32_class" in out:
            summ.update(fp32_class_ms=round(out["fp32_class"]["ms_per_step"], 5), fp32_class_images_s=round(out["fp32_class"]["value"]),
                        fp32_class_kernel_ms=out["fp32_class"].get("kernel_ms"), fp32_class_frac=out["fp32_class"].get("roofline_frac"))
        elif fp32_leg is not None:
            summ.update(fp32_class_ms=round(fp32_leg["ms_per_step"], 5), fp32_class_images_s=round(fp32_leg["value"]),
                        fp32_class_kernel_ms=fp32_leg["roofline"].get("kernel_ms"), fp32_class_frac=fp32_leg["roofline"]["frac"])
        summ["step_frac"] = round(out["roofline"]["step_frac"], 4)
        tr, inf = out.get("trainer") or {}, out.get("inference") or {}
        if isinstance(tr.get("bf16"), dict):
            summ["trainer_images_s"] = round(tr["bf16"]["value"])
        if isinstance(tr.get("fp32"), dict):
            summ["trainer_fp32_class_images_s"] = round(tr["fp32"]["value"])
        for k_src, k_dst in (("decode_device", "decode_images_s"), ("encode_device", "encode_images_s"),
                             ("decode_api", "decode_api_images_s"), ("encode_api", "encode_api_images_s")):
            if isinstance(inf.get(k_src), (int, float)):
                summ[k_dst] = round(inf[k_src])
        for c in out.get("configs") or []:
            if isinstance(c, dict) and "ms_per_step" in c and "config" in c:
                # (side configs lead with the fp32-class leg: `<config>_ms` IS the reference-precision step)
                summ["%s_ms" % str(c["config"]).lower()] = round(c["ms_per_step"], 4)
                if isinstance(c.get("throughput_precision"), dict) and "ms_per_step" in c["throughput_precision"]:
                    summ["%s_throughput_ms" % str(c["config"]).lower()] = round(c["throughput_precision"]["ms_per_step"], 4)
        front = ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline",
                 "dtype", "data")
        ordered = {k: out[k] for k in front}
        ordered["summary"] = summ
        ordered.update({k: v for k, v in out.items() if k not in front})
        print(json.dumps(ordered))
        sys.stdout.flush()
        print("BENCH-SUMMARY " + json.dumps({"value": round(out["value"]), "ms_per_step": round(out["ms_per_step"], 5),
                                             "kernel_ms": out["roofline"].get("kernel_ms"), "frac": out["roofline"].get("frac"),
                                             **summ}), file=sys.stderr)
    if world > 1 or FORCE_DIST:
        pvdist.close_native()                       # (the library's RCCL communicators first: nothing of ours outlives the group)
        td.destroy_process_group()


if __name__ == "__main__":
    main()
