"""The Poisson (log link) SVI step against the Bernoulli step of the same model (scripts/ab_particles.py's method: both arms in
one process, alternating regions after a warm-up, ~10 ms of untimed steps in front of every timed region; ms per step, median
and spread over the regions).  iVAE 28x28 ['r','t'] at batch 256 (the benchmark's shape) and 128, both decoder precisions, loss +
gradients + Adam in one library call.  The Poisson arm trains on counts, the Bernoulli arm on uniform values: the kernels do
the same work whatever the data holds.

  python scripts/ab_poisson.py [--steps 200] [--regions 7] [--out profiles/poisson_ab.txt]

Under `rocprofv3 --kernel-trace --stats` (a short run: --steps 50 --regions 1) the kernel statistics give the decoder launch
of each arm (fp32-class: the Poisson arm runs the bf16 three-product build, the Bernoulli arm the fp16 one) and the normaliser's
two launches (pv_poisson_lognorm_part_kernel, then pv_poisson_lognorm_kernel) on their own; scripts/kstats.py prints them.
"""
import argparse
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import pyroved_amd as pv  # noqa: E402

DIMS, INV = (28, 28), ["r", "t"]


def make_arm(batch, fused, poisson):
    kw = dict(sampler_d="poisson_log", sigmoid_d=False) if poisson else {}
    model = pv.models.iVAE(DIMS, 2, INV, seed=1, device="cuda", **kw)
    eng = model.engine(fused=fused)
    g = torch.Generator().manual_seed(0)
    x = torch.rand(batch, *DIMS, generator=g)
    if poisson:
        x = torch.poisson(1.0 + 2.0 * x, generator=g)
    eps = torch.randn(batch, model.z_dim, generator=g).cuda()
    x = x.cuda()
    return lambda: eng.loss_and_grads(x, eps, step=True), eng


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
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this measurement needs the GPU"
    lines = ["# python scripts/ab_poisson.py --steps %d --regions %d   (%s)" % (args.steps, args.regions, torch.cuda.get_device_name(0)),
             "# ms per SVI step (loss + gradients + Adam, one library call); median [min .. max] over %d alternating regions"
             % args.regions]
    for fused, prec in ((3, "bf16"), (2, "fp32-class")):
        for batch in (256, 128):
            poi, eng_p = make_arm(batch, fused, True)
            ber, eng_b = make_arm(batch, fused, False)
            for step in (poi, ber):
                for _ in range(30):
                    step()
            torch.cuda.synchronize()
            est = region(poi, 20, 0)
            preroll = max(1, min(400, int(10.0 / max(est, 1e-3))))
            t_p, t_b = [], []
            for _ in range(args.regions):
                t_p.append(region(poi, args.steps, preroll))
                t_b.append(region(ber, args.steps, preroll))
            mp_, mb = statistics.median(t_p), statistics.median(t_b)
            lines.append("%-10s B=%3d   poisson_log %.4f [%.4f .. %.4f]   bernoulli %.4f [%.4f .. %.4f]   poisson - bernoulli = %+.1f us "
                         "(x %.3f)   loss %.1f / %.1f" % (prec, batch, mp_, min(t_p), max(t_p), mb, min(t_b), max(t_b),
                                                          1e3 * (mp_ - mb), mp_ / mb, eng_p.scalars[0].item(), eng_b.scalars[0].item()))
            print(lines[-1], flush=True)
    text = "\n".join(lines) + "\n"
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)
    print(text)


if __name__ == "__main__":
    main()
