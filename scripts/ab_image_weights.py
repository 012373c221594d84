"""The SVI step with per-IMAGE observation weights (model.engine(image_weights=True): pv_ivae_weighted_images_step) against the
shared-weight steps next to it (pixel_weights=w: pv_ivae_weighted_step) — scripts/ab_pixel_weights.py's method: every arm in one
process, alternating regions after a warm-up, ~10 ms of untimed steps in front of every timed region; ms per step, median and
spread over the regions.  iVAE 28x28 ['r','t'] at batch 256, loss + gradients + Adam in one library call (step=True).  The
weights are a circular aperture (r^2 <= 1 on the grid), for the per-image arms the same aperture repeated for every image — the
same arithmetic, plus one stream of B N C floats.

Arms, each on this library and — the first four, with --parent-lib PATH (a libpyroved_amd.so built from the parent commit) — on
that library, the same launches (the pair shows that nothing existing moved, and the measurement's own noise):
  the default unweighted step (fused = 2);
  shared-weight C = 1 (the weighted fused f32 kernel);
  shared-weight C = 3 with fused_channels;
  shared-weight layered (C = 1, fused = 0);
  per-image C = 1, C = 3 fused_channels and layered — this library only.

  python scripts/ab_image_weights.py [--steps 200] [--regions 7] [--parent-lib PATH] [--out profiles/image_weights_ab.txt]
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
from ab_multichannel import DIMS, INV, BATCH, region  # noqa: E402
from ab_pixel_weights import load_parent, aperture  # noqa: E402


def make_arm(channels, handle, weights=None, **engine_kw):
    """weights: None, "shared" (pixel_weights = the aperture) or "images" (image_weights = the aperture repeated per image)."""
    model = pv.models.iVAE(DIMS, 2, INV, seed=1, device="cuda", **({} if channels == 1 else {"channels": channels}))
    call_kw = {}
    if weights == "shared":
        engine_kw["pixel_weights"] = aperture(channels)
    elif weights == "images":
        engine_kw["image_weights"] = True
        a = aperture(channels)
        call_kw["image_weights"] = a.unsqueeze(0).expand(BATCH, *a.shape).reshape(BATCH, -1).contiguous().cuda()
    eng = model.engine(**engine_kw)
    g = torch.Generator().manual_seed(0)
    shape = DIMS if channels == 1 else DIMS + (channels,)
    x = torch.rand(BATCH, *shape, generator=g).cuda()
    eps = torch.randn(BATCH, model.z_dim, generator=g).cuda()

    def step():
        _abi._lib = handle
        eng.loss_and_grads(x, eps, step=True, **call_kw)
    return step, eng


SHARED_ARMS = [                                      # (name, channels, weights, engine keywords, uses_fused expected)
    ("C=1 default (fused=2)", 1, None, {}, True),
    ("C=1 shared (fused)", 1, "shared", {}, True),
    ("C=3 fused_channels shared", 3, "shared", {"fused_channels": True}, True),
    ("C=1 shared layered", 1, "shared", {"fused": 0}, False),
]
IMAGE_ARMS = [                                       # (name, the shared arm it is compared with, channels, engine keywords, fused)
    ("C=1 per-image (fused)", "C=1 shared (fused)", 1, {}, True),
    ("C=3 fused_channels per-image", "C=3 fused_channels shared", 3, {"fused_channels": True}, True),
    ("C=1 per-image layered", "C=1 shared layered", 1, {"fused": 0}, False),
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
    for name, ch, weights, kw, fused in SHARED_ARMS:
        if parent is not None:
            arms.append(("parent " + name, None) + make_arm(ch, parent, weights, **dict(kw)))
        step, eng = make_arm(ch, own, weights, **dict(kw))
        assert eng.uses_fused(BATCH) is fused, name
        arms.append(("this   " + name, "parent " + name if parent is not None else None, step, eng))
    for name, ref, ch, kw, fused in IMAGE_ARMS:
        step, eng = make_arm(ch, own, "images", **dict(kw))
        assert eng.uses_fused(BATCH) is fused, name
        arms.append(("this   " + name, "this   " + ref, step, eng))
    lines = ["# python scripts/ab_image_weights.py --steps %d --regions %d%s   (%s)"
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
            rel = "x %.4f (%+.2f us; twice the two arms' spread %.2f us: %s) of [%s]" \
                  % (m / med[ref], 1e3 * d, 1e3 * s2, "inside" if abs(d) <= s2 else "OUTSIDE", ref.strip())
        lines.append("%-40s %.4f [%.4f .. %.4f] (%.2f %%)   %-100s loss %.1f"
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
