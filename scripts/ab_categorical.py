"""The categorical likelihood's step, iVAE(..., channels=C, sampler_d="categorical", sigmoid_d=False), against the Bernoulli step of
the same multi-channel model on the same build — and the multi-channel Bernoulli step on this library against the parent commit's
(scripts/ab_multichannel.py's method: every arm in one process, alternating regions after a warm-up, ~10 ms of untimed steps in
front of every timed region; ms per step, median and spread over the regions).  iVAE 28x28 ['r','t'] at batch 256, loss +
gradients + Adam in one library call (step=True), on the layer-by-layer kernels (fused = 0) and on the fused f32 decoder kernel
(fused_channels=True).

  1. cost of the likelihood: categorical against Bernoulli at C = 3 and C = 8, both routes (this library);
  2. nothing else moved (with --parent-lib PATH, a libpyroved_amd.so built from the parent commit): the Bernoulli C = 3 step of
     both routes on the parent library and on this one, two engines each (A and B, interleaved: the difference between the two
     engines of one library is the null, what the alternation and the buffers' placement make of identical launches); and one
     gradient call of both libraries from identical parameters, whose four scalars and flat gradient must be the same bits.

  python scripts/ab_categorical.py [--steps 200] [--regions 7] [--parent-lib PATH] [--out profiles/categorical_ab.txt]
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
ROUTES = {"layered": dict(fused=0), "fused_channels": dict(fused_channels=True)}


def load_library(path):
    """A second library handle next to the package's own (the binding keeps ONE handle: an arm swaps its own in)."""
    own, own_path = _abi.lib(), _abi.LIB_PATH
    _abi._lib, _abi.LIB_PATH = None, path
    try:
        return _abi.lib()
    finally:
        _abi._lib, _abi.LIB_PATH = own, own_path


def make_arm(channels, route, kind, handle):
    kw = dict(sampler_d="categorical", sigmoid_d=False) if kind == "categorical" else {}
    model = pv.models.iVAE(DIMS, 2, INV, seed=1, device="cuda", channels=channels, **kw)
    _abi._lib = handle
    eng = model.engine(**ROUTES[route])
    g = torch.Generator().manual_seed(0)
    # the same label maps for both likelihoods: one-hot rows are legal Bernoulli observations too
    x = pv.utils.onehot_channels(torch.rand(BATCH, *DIMS, channels, generator=g).argmax(-1), channels).cuda()
    eps = torch.randn(BATCH, model.z_dim, generator=g).cuda()

    def step():
        _abi._lib = handle
        eng.loss_and_grads(x, eps, step=True)

    def grads():
        _abi._lib = handle
        eng.loss_and_grads(x, eps)
        torch.cuda.synchronize()
        return eng.scalars.clone(), eng.grad[:eng.n_flat].clone()
    return step, eng, grads


def region(step, steps, preroll):
    for _ in range(preroll):
        step()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        step()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0) / steps


def measure(arms, steps, regions):
    for _, step, _, _ in arms:
        for _ in range(30):
            step()
    torch.cuda.synchronize()
    est = region(arms[0][1], 20, 0)
    preroll = max(1, min(400, int(10.0 / max(est, 1e-3))))
    times = [[] for _ in arms]
    for _ in range(regions):
        for i, (_, step, _, _) in enumerate(arms):
            times[i].append(region(step, steps, preroll))
    return times


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--regions", type=int, default=7)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this measurement needs the GPU"
    own = _abi.lib()
    lines = ["# python scripts/ab_categorical.py --steps %d --regions %d%s   (%s)"
             % (args.steps, args.regions, " --parent-lib <parent commit's library>" if args.parent_lib else "", torch.cuda.get_device_name(0)),
             "# iVAE 28x28 rt, B = 256: ms per SVI step (loss + gradients + Adam, one library call); median [min .. max] over %d "
             "alternating regions" % args.regions,
             "# 1. categorical against Bernoulli, this library"]
    for channels in (3, 8):
        for route in ROUTES:
            arms = [("%-14s C=%d %-11s" % (route, channels, kind),) + make_arm(channels, route, kind, own)
                    for kind in ("bernoulli", "categorical")]
            t = measure(arms, args.steps, args.regions)
            med = [statistics.median(v) for v in t]
            for (name, _, eng, _), v, m in zip(arms, t, med):
                lines.append("%s %.4f [%.4f .. %.4f]   x %.3f of the Bernoulli step   spread %.4f   loss %.1f"
                             % (name, m, min(v), max(v), m / med[0], max(v) - min(v), eng.scalars[0].item()))
    if args.parent_lib:
        parent = load_library(args.parent_lib)
        lines.append("# 2. the multi-channel Bernoulli step, C = 3: the parent commit's library and this one, two engines each (A - B of a library: the null)")
        for route in ROUTES:
            # two engines a library, interleaved: A against B of one library enqueues the same launches from different buffers
            arms = [("%-14s parent A" % route,) + make_arm(3, route, "bernoulli", parent),
                    ("%-14s this   A" % route,) + make_arm(3, route, "bernoulli", own),
                    ("%-14s parent B" % route,) + make_arm(3, route, "bernoulli", parent),
                    ("%-14s this   B" % route,) + make_arm(3, route, "bernoulli", own)]
            t = measure(arms, args.steps, args.regions)
            med = [statistics.median(v) for v in t]
            for (name, _, _, _), v, m in zip(arms, t, med):
                lines.append("%s %.4f [%.4f .. %.4f]   %+.2f %% against parent A" % (name, m, min(v), max(v), 100.0 * (m / med[0] - 1.0)))
            pm, tm = 0.5 * (med[0] + med[2]), 0.5 * (med[1] + med[3])
            lines.append("%-14s null, parent B - parent A %+.2f %%; null, this B - this A %+.2f %%; this - parent (means of the two) %+.2f %%"
                         % (route, 100.0 * (med[2] / med[0] - 1.0), 100.0 * (med[3] / med[1] - 1.0), 100.0 * (tm / pm - 1.0)))
            # fresh models: one gradient call on each library from identical parameters
            (_, _, ga), (_, _, gb) = make_arm(3, route, "bernoulli", parent), make_arm(3, route, "bernoulli", own)
            (sa, fa), (sb, fb) = ga(), gb()
            same = torch.equal(sa, sb) and torch.equal(fa, fb)
            lines.append("%-14s scalars and flat gradient (%d floats) of the two libraries bit-identical: %s" % (route, fa.numel(), same))
            assert same, "the Bernoulli multi-channel step changed (%s)" % route
    _abi._lib = own
    text = "\n".join(lines) + "\n"
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)
    print(text)


if __name__ == "__main__":
    main()
