"""The SVI step of a model whose positions are no multiple of 16 on the tail form of the fused f32 decoder kernel
(model.engine(fused_any_size=True): pv_sdec_fused_mc_tail_kernel<true, C, 0>) against what such a model runs without the keyword
and against the neighbouring size on the same kernel family — scripts/ab_multichannel.py's method: every arm in one process,
alternating regions after a warm-up, ~10 ms of untimed steps in front of every timed region; ms per step, median and spread over
the regions.  iVAE ['r','t'] at batch 256, loss + gradients + Adam in one library call (step=True).

Arms, per C in --channels (default 1,3; C > 1 with fused_channels=True):
  (a) 27 x 27 with fused_any_size=True              729 positions: 46 units per sample, the last with 9 valid rows
  (b) 27 x 27 without it                            the layer-by-layer step, which is what such a model runs otherwise
  (c) 28 x 28 at fused=1 without it                 784 positions: 49 units per sample on pv_sdec_fused_kernel / _mc_kernel
Two conditions, both checked here and printed with the table:
  (a) <= (c) + the run-to-run spread   (a) walks 46 units per sample against 49 and does the same work per unit; the spread is
                                       the larger of the two arms' (max - min) over the regions
  (a) < (b)                            the reason the keyword exists

  python scripts/ab_any_size.py [--steps 200] [--regions 7] [--channels 1,3] [--out profiles/any_size_ab.txt]

Kernel durations come from separate, short runs under `rocprofv3 --kernel-trace --stats --output-format csv` (tracing only), one arm per process so
that the launches the arms share (the generic encoder's) are not mixed: --arms a (or c) --channels 1 --steps 50 --regions 1;
scripts/kstats.py prints them.  With --arms the two conditions are not evaluated.
"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pyroved_amd as pv  # noqa: E402
from ab_multichannel import INV, BATCH, region  # noqa: E402


def make_arm(dims, channels, **engine_kw):
    model = pv.models.iVAE(dims, 2, INV, seed=1, device="cuda", **({} if channels == 1 else {"channels": channels}))
    eng = model.engine(**engine_kw)
    g = torch.Generator().manual_seed(0)
    shape = dims if channels == 1 else dims + (channels,)
    x = torch.rand(BATCH, *shape, generator=g).cuda()
    eps = torch.randn(BATCH, model.z_dim, generator=g).cuda()

    def step():
        eng.loss_and_grads(x, eps, step=True)
    return step, eng


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--regions", type=int, default=7)
    ap.add_argument("--channels", default="1,3")
    ap.add_argument("--out", default=None)
    ap.add_argument("--arms", default="abc", help="a subset of the arms, for a profiling run (no conditions are evaluated)")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this measurement needs the GPU"
    arms = []                                          # (name, C, kind, step, engine)
    for c in (int(v) for v in args.channels.split(",")):
        ch = dict(fused_channels=True) if c > 1 else {}
        step, eng = make_arm((27, 27), c, fused_any_size=True, **ch)
        assert eng.uses_fused(BATCH), "C = %d, 27 x 27: fused_any_size does not run the fused kernel" % c
        arms.append(("(a) C=%d 27x27 fused_any_size" % c, c, "a", step, eng))
        step, eng = make_arm((27, 27), c, **ch)
        assert not eng.uses_fused(BATCH)
        arms.append(("(b) C=%d 27x27 layered" % c, c, "b", step, eng))
        step, eng = make_arm((28, 28), c, fused=1, **ch)
        assert eng.uses_fused(BATCH)
        arms.append(("(c) C=%d 28x28 fused=1" % c, c, "c", step, eng))
    arms = [arm for arm in arms if arm[2] in args.arms]
    lines = ["# python scripts/ab_any_size.py --steps %d --regions %d --channels %s   (%s)"
             % (args.steps, args.regions, args.channels, torch.cuda.get_device_name(0)),
             "# iVAE rt, B = 256: ms per SVI step (loss + gradients + Adam, one library call); median [min .. max] over %d "
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
    by = {(c, kind): t for (_, c, kind, _, _), t in zip(arms, times)}
    for (name, c, kind, _, eng), t in zip(arms, times):
        lines.append("%-30s %.4f [%.4f .. %.4f]   loss %.1f" % (name, statistics.median(t), min(t), max(t), eng.scalars[0].item()))
    ok = True
    for c in sorted({c for _, c, _, _, _ in arms} if set("abc") <= set(args.arms) else ()):
        a, b, cc = (by[(c, k)] for k in "abc")
        ma, mb, mc_ = (statistics.median(t) for t in (a, b, cc))
        spread = max(max(a) - min(a), max(cc) - min(cc))
        c1, c2 = ma <= mc_ + spread, ma < mb
        ok = ok and c1 and c2
        lines.append("C=%d: (a) / (c) = %.3f, (a) - (c) = %+.4f ms against a spread of %.4f ms: %s;   (a) / (b) = %.3f: %s"
                     % (c, ma / mc_, ma - mc_, spread, "holds" if c1 else "DOES NOT HOLD", ma / mb, "faster" if c2 else "NOT FASTER"))
    text = "\n".join(lines) + "\n"
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)
    print(text)
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
