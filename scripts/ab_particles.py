"""The multi-particle SVI step (engine(particles=P): one encoder pass over B images, P decoder samples per image) against the
only thing a user could do before it: the one-particle step on the minibatch repeated P times (P*B images through the encoder,
a loss P times too large).  iVAE 28x28 ['r','t'], both decoder precisions, loss + gradients + Adam in one library call:
  (a) B = 64,  P = 4   (256 decoder samples; the emulation's batch of 256 hosts its guide in the bf16 decoder launch)
  (b) B = 256, P = 2   (512 decoder samples: neither arm's guide folds)
Both arms live in the same process and alternate, region by region, after a warm-up of every shape and ~10 ms of untimed
steps in front of every timed region (as bench.py does); the figure is ms per step, median and spread over the regions.
--renyi ALPHA adds a third arm to every row, alternating with the other two: the importance-weighted bound of that order over
the same P samples (engine(particles=P, renyi=ALPHA)), timed against the P-particle ELBO step — on the fused decoder it runs
the decoder forward twice.

  python scripts/ab_particles.py [--steps 200] [--regions 7] [--renyi 0.0] [--out profiles/particles_ab.txt]
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


def make_arm(batch, particles, fused, repeat, renyi=None):
    """repeat > 1: the emulation — `batch` images repeated `repeat` times, one particle."""
    model = pv.models.iVAE(DIMS, 2, INV, seed=1, device="cuda")
    eng = model.engine(fused=fused, particles=particles, renyi=renyi)
    g = torch.Generator().manual_seed(0)
    x = torch.rand(batch, *DIMS, generator=g)
    eps = torch.randn(max(particles, repeat) * batch, model.z_dim, generator=g).cuda()
    x = (x.repeat(repeat, 1, 1) if repeat > 1 else x).cuda()
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
    ap.add_argument("--renyi", type=float, default=None, help="order alpha of the importance-weighted bound: adds its arm")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this measurement needs the GPU"
    lines = ["# python scripts/ab_particles.py --steps %d --regions %d%s   (%s)"
             % (args.steps, args.regions, "" if args.renyi is None else " --renyi %g" % args.renyi, torch.cuda.get_device_name(0)),
             "# ms per SVI step (loss + gradients + Adam, one library call); median [min .. max] over %d alternating regions"
             % args.regions]
    for fused, prec in ((3, "bf16"), (2, "fp32-class")):
        for batch, P in ((64, 4), (256, 2)):
            new, eng_new = make_arm(batch, P, fused, 1)
            old, eng_old = make_arm(batch, 1, fused, P)
            ren, eng_ren = make_arm(batch, P, fused, 1, args.renyi) if args.renyi is not None else (None, None)
            for step in (new, old, ren):                    # warm-up of every shape
                if step is None:
                    continue
                for _ in range(30):
                    step()
            torch.cuda.synchronize()
            est = region(new, 20, 0)
            preroll = max(1, min(400, int(10.0 / max(est, 1e-3))))
            t_new, t_old, t_ren = [], [], []
            for _ in range(args.regions):
                t_new.append(region(new, args.steps, preroll))
                t_old.append(region(old, args.steps, preroll))
                if ren is not None:
                    t_ren.append(region(ren, args.steps, preroll))
            mn, mo = statistics.median(t_new), statistics.median(t_old)
            lines.append("%-10s B=%3d P=%d   particles %.4f [%.4f .. %.4f]   repeated batch (B=%d, P=1) %.4f [%.4f .. %.4f]   "
                         "particles / repeated = %.3f   loss %.3f vs %.3f / %d"
                         % (prec, batch, P, mn, min(t_new), max(t_new), batch * P, mo, min(t_old), max(t_old), mn / mo,
                            eng_new.scalars[0].item(), eng_old.scalars[0].item(), P))
            print(lines[-1], flush=True)
            if ren is not None:
                mr = statistics.median(t_ren)
                lines.append("%-10s B=%3d P=%d   renyi(alpha=%g) %.4f [%.4f .. %.4f]   renyi / particles = %.3f   loss %.3f"
                             % (prec, batch, P, args.renyi, mr, min(t_ren), max(t_ren), mr / mn, eng_ren.scalars[0].item()))
                print(lines[-1], flush=True)
    text = "\n".join(lines) + "\n"
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)
    print(text)


if __name__ == "__main__":
    main()
