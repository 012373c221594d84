"""The SVI step with per-observation weights (model.engine(pixel_weights=w): pv_ivae_weighted_step) against the unweighted steps
next to it — scripts/ab_multichannel.py's method: every arm in one process, alternating regions after a warm-up, ~10 ms of
untimed steps in front of every timed region; ms per step, median and spread over the regions.  iVAE 28x28 ['r','t'] at batch
256, loss + gradients + Adam in one library call (step=True).  The weights are a circular aperture (r^2 <= 1 on the grid).

Arms:
  the default unweighted step (fused = 2) on this library — and, with --parent-lib PATH (a libpyroved_amd.so built from the
      parent commit), on that library: the same launches, so the pair shows that the default objective did not move (and, the
      two alternating, the measurement's own noise);
  C = 1 weighted (the weighted fused f32 kernel, pv_sdec_fused_mc_kernel<true, 1, true>) against the unweighted fused = 1 step
      (pv_sdec_fused_kernel<true>) and the unweighted default (the fp16-piece kernel a weighted model leaves), and against the
      weighted layered step (fused = 0);
  C = 3 fused_channels weighted against unweighted.

  python scripts/ab_pixel_weights.py [--steps 200] [--regions 7] [--parent-lib PATH] [--out profiles/pixel_weights_ab.txt]
"""
import argparse
import ctypes as C
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pyroved_amd as pv  # noqa: E402
from pyroved_amd import _abi  # noqa: E402
from ab_multichannel import DIMS, INV, BATCH, region  # noqa: E402


def load_parent(path):
    """The parent commit's library next to the package's own: it lacks the pv_ivae_weighted_* symbols the binding insists on, so
    it is bound here, symbol by symbol, with what it has."""
    handle = C.CDLL(path)
    for name, (res, args) in _abi.SIGNATURES.items():
        fn = getattr(handle, name, None)
        if fn is not None:
            fn.restype, fn.argtypes = res, args
    assert handle.pv_version() == _abi.PV_ABI_VERSION
    return handle


def aperture(channels):
    mesh = torch.meshgrid(*[torch.linspace(-1.0, 1.0, d) for d in DIMS], indexing="ij")
    w = (sum(m ** 2 for m in mesh) <= 1.0).to(torch.float32)
    return w if channels == 1 else w.unsqueeze(-1).expand(*DIMS, channels).contiguous()


def make_arm(channels, handle, weighted=False, **engine_kw):
    model = pv.models.iVAE(DIMS, 2, INV, seed=1, device="cuda", **({} if channels == 1 else {"channels": channels}))
    if weighted:
        engine_kw["pixel_weights"] = aperture(channels)
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
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this measurement needs the GPU"
    own = _abi.lib()
    arms = []                                          # (name, reference arm's name or None, step, engine)
    if args.parent_lib:
        arms.append(("parent C=1 default (fused=2)", None) + make_arm(1, load_parent(args.parent_lib)))
    arms.append(("this   C=1 default (fused=2)", "parent C=1 default (fused=2)" if args.parent_lib else None) + make_arm(1, own))
    arms.append(("this   C=1 fused=1", "this   C=1 default (fused=2)") + make_arm(1, own, fused=1))
    step, eng = make_arm(1, own, weighted=True)
    assert eng.uses_fused(BATCH), "the weighted one-channel step does not run the fused kernel"
    arms.append(("this   C=1 weighted (fused)", "this   C=1 fused=1", step, eng))
    arms.append(("this   C=1 weighted layered", "this   C=1 weighted (fused)") + make_arm(1, own, weighted=True, fused=0))
    arms.append(("this   C=3 fused_channels", None) + make_arm(3, own, fused_channels=True))
    step, eng = make_arm(3, own, weighted=True, fused_channels=True)
    assert eng.uses_fused(BATCH), "the weighted three-channel step does not run the fused kernel"
    arms.append(("this   C=3 fused_channels weighted", "this   C=3 fused_channels", step, eng))
    lines = ["# python scripts/ab_pixel_weights.py --steps %d --regions %d%s   (%s)"
             % (args.steps, args.regions, " --parent-lib <parent commit's library>" if args.parent_lib else "", torch.cuda.get_device_name(0)),
             "# iVAE 28x28 rt, B = 256, weights: circular aperture: ms per SVI step (loss + gradients + Adam, one library call); "
             "median [min .. max] over %d alternating regions" % args.regions]
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
    for (name, ref, _, eng), t in zip(arms, times):
        m = med[name]
        rel = "x %.3f (%+.1f us) of [%s]" % (m / med[ref], 1e3 * (m - med[ref]), ref.strip()) if ref else ""
        lines.append("%-36s %.4f [%.4f .. %.4f]   %-62s loss %.1f" % (name, m, min(t), max(t), rel, eng.scalars[0].item()))
    if "this   C=1 weighted (fused)" in med:
        lines.append("# weighted C=1 against the default unweighted step: x %.3f"
                     % (med["this   C=1 weighted (fused)"] / med["this   C=1 default (fused=2)"]))
    _abi._lib = own
    text = "\n".join(lines) + "\n"
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)
    print(text)


if __name__ == "__main__":
    main()
