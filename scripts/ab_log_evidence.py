"""What the held-out log-evidence costs: one chunk of P particles (engine.log_evidence_chunk -> pv_ivae_evidence_accumulate)
against the call that runs the same launches, the forward-only importance-weighted bound
engine(particles=P, renyi=0.0).loss_and_grads(want_grads=False), on the same inputs.  iVAE 28x28 ['r','t'], B = 256, P = 16, both
decoder precisions (fused 2 and 3).  The evidence call replaces the bound's weights + per-image loss + scalars launches by the
log-weights and the state update, so the two should be equal within the spread of the alternating regions.
Both arms alternate region by region in one process after a warm-up and ~10 ms of untimed calls in front of every timed region
(as bench.py and scripts/ab_particles.py do); the figure is ms per call, median and spread over the regions.
A second table gives the throughput of the whole estimate, model.log_evidence with K = 1024 samples in chunks (the default
chunk, 16 and 64), as image-samples per second (images x K / wall time; the host loop, the eps draws on the CPU generator, their
upload and the final copy included).

  python scripts/ab_log_evidence.py [--steps 100] [--regions 7] [--out profiles/log_evidence_ab.txt]
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


def make_arms(batch, P, fused):
    g = torch.Generator().manual_seed(0)
    x = torch.rand(batch, *DIMS, generator=g).cuda()
    ev_model = pv.models.iVAE(DIMS, 2, INV, seed=1, device="cuda")
    re_model = pv.models.iVAE(DIMS, 2, INV, seed=1, device="cuda")
    eps = torch.randn(P * batch, ev_model.z_dim, generator=g).cuda()
    ev_eng = ev_model.engine(fused=fused)
    re_eng = re_model.engine(fused=fused, particles=P, renyi=0.0)
    state = torch.empty(batch, 4, device="cuda")
    return (lambda: ev_eng.log_evidence_chunk(x, eps, None, state, True)), (lambda: re_eng.loss_and_grads(x, eps, want_grads=False)), \
        ev_eng, re_eng, state


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
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--regions", type=int, default=7)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this measurement needs the GPU"
    batch, P = 256, 16
    lines = ["# python scripts/ab_log_evidence.py --steps %d --regions %d   (%s)" % (args.steps, args.regions, torch.cuda.get_device_name(0)),
             "# ms per call, 28x28 ['r','t'], B = %d, P = %d; median [min .. max] over %d alternating regions" % (batch, P, args.regions)]
    for fused, prec in ((3, "bf16"), (2, "fp32-class")):
        ev, ren, ev_eng, re_eng, state = make_arms(batch, P, fused)
        for step in (ev, ren):
            for _ in range(20):
                step()
        torch.cuda.synchronize()
        preroll = max(1, min(400, int(10.0 / max(region(ev, 10, 0), 1e-3))))
        t_ev, t_re = [], []
        for _ in range(args.regions):
            t_ev.append(region(ev, args.steps, preroll))
            t_re.append(region(ren, args.steps, preroll))
        me, mr = statistics.median(t_ev), statistics.median(t_re)
        lp, _ = ev_eng.log_evidence_finish(state, P)
        lines.append("%-10s evidence chunk %.4f [%.4f .. %.4f]   renyi(alpha=0) forward only %.4f [%.4f .. %.4f]   evidence / renyi = %.3f   "
                     "sum log p^ %.3f vs -loss %.3f   workspace %.1f MB vs %.1f MB"
                     % (prec, me, min(t_ev), max(t_ev), mr, min(t_re), max(t_re), me / mr, lp.double().sum().item(),
                        -re_eng.scalars[0].item(), ev_eng._ev_ws.numel() / 2 ** 20, re_eng.ws.numel() / 2 ** 20))
        print(lines[-1], flush=True)
    lines.append("# model.log_evidence, K = 1024 samples per image, 256 images in one batch: image-samples per second (wall time of the call)")
    K = 1024
    for fused, prec in ((3, "bf16"), (2, "fp32-class")):
        model = pv.models.iVAE(DIMS, 2, INV, seed=1, device="cuda")
        model.engine(fused=fused)
        x = torch.rand(batch, *DIMS, generator=torch.Generator().manual_seed(0))
        default = model._evidence_chunk(K, batch, model._evidence_positions())
        for chunk in (default, 16, 64):
            torch.manual_seed(0)
            model.log_evidence(x, num_samples=2 * chunk, chunk=chunk, batch_size=batch)             # warm-up
            ts = []
            for _ in range(3):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                lp, ess = model.log_evidence(x, num_samples=K, chunk=chunk, batch_size=batch, return_ess=True)
                ts.append(time.perf_counter() - t0)
            t = statistics.median(ts)
            lines.append("%-10s K=%d in chunks of %2d%s: %.3f s [%.3f .. %.3f]   %.3e image-samples/s   mean log p^ %.3f   mean ESS %.1f   "
                         "workspace %.0f MB" % (prec, K, chunk, " (default)" if chunk == default else "", t, min(ts), max(ts),
                                                batch * K / t, lp.mean().item(), ess.mean().item(), model.engine()._ev_ws.numel() / 2 ** 20))
            print(lines[-1], flush=True)
    text = "\n".join(lines) + "\n"
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)
    print(text)


if __name__ == "__main__":
    main()
