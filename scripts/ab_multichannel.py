"""The multi-channel SVI step, iVAE(..., channels=C), against the single-channel step of the same model (scripts/ab_poisson.py's
method: every arm in one process, alternating regions after a warm-up, ~10 ms of untimed steps in front of every timed region;
ms per step, median and spread over the regions).  iVAE 28x28 ['r','t'] at batch 256 on the layer-by-layer kernels (fused = 0,
the path a multi-channel model runs whatever it asks for), loss + gradients + Adam in one library call.

Arms: this library at C = 1, 2, 3, 4 — C = 1 runs pv_out_lik_kernel, C > 1 the pv_out_lik_mc_kernel<C> instance; only that launch
and the element counts of x / loc / the encoder's first layer differ from the C = 1 step.  With --parent-lib PATH (a
libpyroved_amd.so built from the parent commit) a further arm runs the same C = 1 model on that library: the two C = 1 arms
enqueue the same launches, so their difference is the alternation's own noise.  The last arm is C = 1 on the fused decoder
(fused = 2, the default): what a multi-channel model pays today for having no fused kernel.

  python scripts/ab_multichannel.py [--steps 200] [--regions 7] [--parent-lib PATH] [--out profiles/multichannel_ab.txt]

Under `rocprofv3 --kernel-trace --stats` (a short run: --steps 50 --regions 1 --channels 1,3) the kernel statistics give
pv_out_lik_kernel and pv_out_lik_mc_kernel<3> on the same 200 704 rows; scripts/kstats.py prints them.
"""
import argparse
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import pyroved_amd as pv  # noqa: E402
from pyroved_amd import _abi  # noqa: E402

DIMS, INV, BATCH = (28, 28), ["r", "t"], 256


def load_library(path):
    """A second library handle next to the package's own (the binding keeps ONE handle: an arm swaps its own in)."""
    own, own_path = _abi.lib(), _abi.LIB_PATH
    _abi._lib, _abi.LIB_PATH = None, path
    try:
        return _abi.lib()
    finally:
        _abi._lib, _abi.LIB_PATH = own, own_path


def make_arm(channels, fused, handle):
    model = pv.models.iVAE(DIMS, 2, INV, seed=1, device="cuda", **({} if channels == 1 else {"channels": channels}))
    eng = model.engine(fused=fused)
    g = torch.Generator().manual_seed(0)
    shape = DIMS if channels == 1 else DIMS + (channels,)
    x = torch.rand(BATCH, *shape, generator=g).cuda()
    eps = torch.randn(BATCH, model.z_dim, generator=g).cuda()

    def step():
        _abi._lib = handle
        eng.loss_and_grads(x, eps, step=True)
    return step, eng


def region(step, steps, preroll):
    for _ in range(preroll):
        step()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        step()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0) / steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--regions", type=int, default=7)
    ap.add_argument("--channels", default="1,2,3,4")
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this measurement needs the GPU"
    own = _abi.lib()
    arms = []
    if args.parent_lib:
        arms.append(("parent C=1 layered",) + make_arm(1, 0, load_library(args.parent_lib)))
    for c in (int(v) for v in args.channels.split(",")):
        arms.append(("this   C=%d layered" % c,) + make_arm(c, 0, own))
    arms.append(("this   C=1 fused=2",) + make_arm(1, 2, own))
    lines = ["# python scripts/ab_multichannel.py --steps %d --regions %d%s   (%s)"
             % (args.steps, args.regions, " --parent-lib <parent commit's library>" if args.parent_lib else "", torch.cuda.get_device_name(0)),
             "# iVAE 28x28 rt, B = 256: ms per SVI step (loss + gradients + Adam, one library call); median [min .. max] over %d "
             "alternating regions" % args.regions]
    for _, step, _ in arms:
        for _ in range(30):
            step()
    torch.cuda.synchronize()
    est = region(arms[0][1], 20, 0)
    preroll = max(1, min(400, int(10.0 / max(est, 1e-3))))
    times = [[] for _ in arms]
    for _ in range(args.regions):
        for i, (_, step, _) in enumerate(arms):
            times[i].append(region(step, args.steps, preroll))
    base = None
    for (name, _, eng), t in zip(arms, times):
        med = statistics.median(t)
        if name.startswith("this   C=1 layered"):
            base = med
    for (name, _, eng), t in zip(arms, times):
        med = statistics.median(t)
        lines.append("%-20s %.4f [%.4f .. %.4f]   x %.3f of this C=1 layered   loss %.1f"
                     % (name, med, min(t), max(t), med / base if base else float("nan"), eng.scalars[0].item()))
    _abi._lib = own
    text = "\n".join(lines) + "\n"
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)
    print(text)


if __name__ == "__main__":
    main()
