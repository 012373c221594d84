"""The weighted SVI step on the bf16-class decoder kernels (fast_weights=True: the weighted instances of the 4-wave fused kernel,
PV_PLAN_FAST_WEIGHTS) against the weighted step as it runs without the keyword (the weighted fused f32 kernel) and the unweighted
steps next to them — scripts/ab_image_weights.py's method: every arm in one process, alternating regions after a warm-up, ~10 ms
of untimed steps in front of every timed region; ms per step, median and spread over the regions.  iVAE 28x28 ['r','t'] at batch
256, loss + gradients + Adam in one library call (step=True).  The weights are a circular aperture (r^2 <= 1 on the grid), for
the per-image arms the same aperture repeated for every image.

Arms:
  the weighted step without the keyword (fused f32 kernel) on the parent commit's library (--parent-lib PATH): the baseline;
  the same on this library (must sit inside the spread of the parent's: nothing existing moved);
  fast_weights on the x3 route (fused = 2) and on the plain-bf16 route (fused = 3), shared weights;
  the unweighted default step (fused = 2) and the unweighted bf16 step (fused = 3);
  both fast_weights routes again with per-image weights.
A route is worth shipping where its arm is below the baseline by more than twice the two arms' spread.

  python scripts/ab_fast_weights.py [--steps 200] [--regions 7] [--parent-lib PATH] [--out profiles/fast_weights_ab.txt]
"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from pyroved_amd import _abi  # noqa: E402
from ab_multichannel import BATCH, region  # noqa: E402
from ab_pixel_weights import load_parent  # noqa: E402
from ab_image_weights import make_arm  # noqa: E402

WEIGHTED = "weighted shared (fused f32 kernel)"
ARMS = [                                             # (name, weights, engine keywords, the decoder kernel's name contains)
    ("fast_weights x3 shared", "shared", dict(fused=2, fast_weights=True), "bf16_wt_kernel<true, 0, 1>"),
    ("fast_weights bf16 shared", "shared", dict(fused=3, fast_weights=True), "bf16_wt_kernel<true, 0, 0>"),
    ("unweighted default (fused=2)", None, dict(fused=2), None),
    ("unweighted bf16 (fused=3)", None, dict(fused=3), None),
    ("fast_weights x3 per-image", "images", dict(fused=2, fast_weights=True), "bf16_wt_kernel<true, 0, 1>"),
    ("fast_weights bf16 per-image", "images", dict(fused=3, fast_weights=True), "bf16_wt_kernel<true, 0, 0>"),
]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--regions", type=int, default=7)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this measurement needs the GPU"
    own = _abi.lib()
    parent = load_parent(args.parent_lib) if args.parent_lib else None
    arms = []                                          # (name, reference arm's name or None, step, engine)
    if parent is not None:
        arms.append(("parent " + WEIGHTED, None) + make_arm(1, parent, "shared"))
    base = ("parent " if parent is not None else "this   ") + WEIGHTED
    step, eng = make_arm(1, own, "shared")
    assert "pv_sdec_fused_mc_kernel<true, 1, 1>" in _abi.weighted_decoder_kernel_name(eng._plan(BATCH), 0, 1)
    arms.append(("this   " + WEIGHTED, base if parent is not None else None, step, eng))
    for name, weights, kw, kernel in ARMS:
        step, eng = make_arm(1, own, weights, **dict(kw))
        if kernel:
            got = _abi.weighted_decoder_kernel_name(eng._plan(BATCH), weights == "images", 1)
            assert kernel in got, (name, got)
        arms.append(("this   " + name, base, step, eng))
    lines = ["# python scripts/ab_fast_weights.py --steps %d --regions %d%s   (%s)"
             % (args.steps, args.regions, " --parent-lib <parent commit's library>" if parent is not None else "",
                torch.cuda.get_device_name(0)),
             "# iVAE 28x28 rt, B = 256, weights: circular aperture (per-image: repeated for every image): ms per SVI step (loss + "
             "gradients + Adam, one library call); median [min .. max] (spread %% of the median) over %d alternating regions" % args.regions]
    for arm in arms:
        for _ in range(30):
            arm[2]()
    torch.cuda.synchronize()
    est = region(arms[0][2], 20, 0)
    preroll = max(1, min(400, int(10.0 / max(est, 1e-3))))
    times = [[] for _ in arms]
    for _ in range(args.regions):
        for i, arm in enumerate(arms):
            times[i].append(region(arm[2], args.steps, preroll))
    med = {arm[0]: statistics.median(t) for arm, t in zip(arms, times)}
    spread = {arm[0]: max(t) - min(t) for arm, t in zip(arms, times)}
    for (name, ref, _, eng), t in zip(arms, times):
        m = med[name]
        rel = ""
        if ref:
            d, s2 = m - med[ref], 2.0 * max(spread[name], spread[ref])
            where = "inside" if abs(d) <= s2 else ("BELOW" if d < 0 else "ABOVE")
            rel = "x %.4f (%+.2f us; twice the two arms' spread %.2f us: %s) of [%s]" % (m / med[ref], 1e3 * d, 1e3 * s2, where, ref.strip())
        lines.append("%-52s %.4f [%.4f .. %.4f] (%.2f %%)   %-112s loss %.1f"
                     % (name, m, min(t), max(t), 100.0 * spread[name] / m, rel, eng.scalars[0].item()))
    _abi._lib = own
    text = "\n".join(lines) + "\n"
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)
    print(text)


if __name__ == "__main__":
    main()
