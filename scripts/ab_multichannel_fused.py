"""The multi-channel SVI step on the fused f32 decoder kernel (model.engine(fused_channels=True): pv_sdec_fused_mc_kernel<true, C>)
against the layer-by-layer step a multi-channel model otherwise runs — scripts/ab_multichannel.py's method: every arm in one
process, alternating regions after a warm-up, ~10 ms of untimed steps in front of every timed region; ms per step, median and
spread over the regions.  iVAE 28x28 ['r','t'] at batch 256, loss + gradients + Adam in one library call (step=True).

Arms, per C in --channels (default 2,3,4,8): this library layered (fused = 0) and this library with fused_channels=True; with
--parent-lib PATH (a libpyroved_amd.so built from the parent commit) the layered arm on that library as well — the arm the
fused one has to beat, and, next to this library's layered arm (the same launches), the alternation's own noise.  The last arm
is C = 1 at fused = 1: pv_sdec_fused_kernel<true>, the kernel the multi-channel one is a sibling of.

  python scripts/ab_multichannel_fused.py [--steps 200] [--regions 7] [--parent-lib PATH] [--out profiles/multichannel_fused_ab.txt]

Kernel durations come from a separate, short run under `rocprofv3 --kernel-trace --stats` (tracing only, no counters:
--steps 50 --regions 1): pv_sdec_fused_mc_kernel<true, C> next to pv_sdec_fused_kernel<true> on the same 200 704 rows, and
pv_sdec_fused_mc_reduce_out_kernel; scripts/kstats.py prints them.
"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pyroved_amd as pv  # noqa: E402
from pyroved_amd import _abi  # noqa: E402
from ab_multichannel import DIMS, INV, BATCH, load_library, region  # noqa: E402


def make_arm(channels, handle, **engine_kw):
    model = pv.models.iVAE(DIMS, 2, INV, seed=1, device="cuda", **({} if channels == 1 else {"channels": channels}))
    eng = model.engine(**engine_kw)
    g = torch.Generator().manual_seed(0)
    shape = DIMS if channels == 1 else DIMS + (channels,)
    x = torch.rand(BATCH, *shape, generator=g).cuda()
    eps = torch.randn(BATCH, model.z_dim, generator=g).cuda()

    def step():
        _abi._lib = handle
        eng.loss_and_grads(x, eps, step=True)
    return step, eng


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--regions", type=int, default=7)
    ap.add_argument("--channels", default="2,3,4,8")
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this measurement needs the GPU"
    own = _abi.lib()
    parent = load_library(args.parent_lib) if args.parent_lib else None
    arms = []                                          # (name, C, kind, step, engine)
    for c in (int(v) for v in args.channels.split(",")):
        if parent is not None:
            arms.append(("parent C=%d layered" % c, c, "parent") + make_arm(c, parent, fused=0))
        arms.append(("this   C=%d layered" % c, c, "layered") + make_arm(c, own, fused=0))
        step, eng = make_arm(c, own, fused_channels=True)
        assert eng.uses_fused(BATCH), "C = %d does not run the fused kernel" % c
        arms.append(("this   C=%d fused_channels" % c, c, "fused", step, eng))
    arms.append(("this   C=1 fused=1", 1, "base") + make_arm(1, own, fused=1))
    lines = ["# python scripts/ab_multichannel_fused.py --steps %d --regions %d%s   (%s)"
             % (args.steps, args.regions, " --parent-lib <parent commit's library>" if args.parent_lib else "", torch.cuda.get_device_name(0)),
             "# iVAE 28x28 rt, B = 256: ms per SVI step (loss + gradients + Adam, one library call); median [min .. max] over %d "
             "alternating regions" % args.regions]
    for arm in arms:
        for _ in range(30):
            arm[3]()
    torch.cuda.synchronize()
    est = region(arms[0][3], 20, 0)
    preroll = max(1, min(400, int(10.0 / max(est, 1e-3))))
    times = [[] for _ in arms]
    for _ in range(args.regions):
        for i, arm in enumerate(arms):
            times[i].append(region(arm[3], args.steps, preroll))
    med = [statistics.median(t) for t in times]
    ref = {}                                           # per C: the arm to beat (the parent's layered step, else this library's)
    for (name, c, kind, _, _), m in zip(arms, med):
        if kind == "parent" or (kind == "layered" and c not in ref):
            ref[c] = m
    for (name, c, kind, _, eng), t, m in zip(arms, times, med):
        rel = "x %.3f of %s C=%d layered" % (m / ref[c], "parent" if parent is not None else "this", c) if c in ref else ""
        lines.append("%-26s %.4f [%.4f .. %.4f]   %-34s loss %.1f" % (name, m, min(t), max(t), rel, eng.scalars[0].item()))
    _abi._lib = own
    text = "\n".join(lines) + "\n"
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)
    print(text)


if __name__ == "__main__":
    main()
