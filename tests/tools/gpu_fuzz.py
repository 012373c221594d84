"""Randomised parity sweep on the GPU: random iVAE / jiVAE / ssiVAE / ss_reg_iVAE configurations (data shapes incl. odd and
1-D, invariance sets, widths, activations, samplers, conditioning, batch sizes incl. 1 and non-multiples of 16, decoder
paths) against the CPU oracle from identical parameters: loss to 2e-5, every gradient tensor to a relative-L2 bar.
Prints one line per case and a summary; exit code 1 on any failure.    python tests/tools/gpu_fuzz.py [n_cases] [seed]"""
import os, sys, random, traceback
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import numpy as np, torch
import pyroved_amd as pv
from oracle import svi_oracle as orc
from _judge import rel_l2

n_cases = int(sys.argv[1]) if len(sys.argv) > 1 else 60
rng = random.Random(int(sys.argv[2]) if len(sys.argv) > 2 else 0)


def case():
    one_d = rng.random() < 0.2
    if one_d:
        data_dim = (rng.choice([16, 24, 32, 40]),)
        inv = rng.choice([None, ["t"]])
    else:
        data_dim = rng.choice([(8, 8), (12, 20), (16, 16), (7, 9), (28, 28), (16, 8)])
        inv = rng.choice([None, ["r"], ["t"], ["s"], ["r", "t"], ["r", "s"], ["t", "s"], ["r", "t", "s"]])
    family = rng.choice(os.environ.get("FAMILIES", "ivae,ivae,ivae,jivae,jivae,sscls,ssreg,ved").split(","))
    wide = rng.random() < 0.6                      # default widths (fused decoder / compact encoder) or custom ones
    hid = [128, 128] if wide else rng.choice([[64, 64], [32, 48], [128, 64, 32], [16]])
    act = "tanh" if rng.random() < 0.6 else rng.choice(["relu", "lrelu", "softplus"])
    sampler = rng.choice(["bernoulli", "bernoulli", "gaussian"])
    b = rng.choice([1, 2, 5, 7, 16, 19, 33])
    return dict(family=family, data_dim=data_dim, inv=inv, hid=hid, act=act, sampler=sampler, b=b,
                latent=rng.choice([2, 2, 3]), c_dim=rng.choice([0, 0, 2, 3]), K=rng.choice([2, 3, 5]),
                fused=rng.choice([0, 1, 2, 2]), beta=rng.choice([1.0, 1.0, 2.5]))


FORCE_FUSED = os.environ.get("FORCE_FUSED")        # e.g. 3: the mixed-precision mode everywhere (bars widened to 5e-2 / 5e-4)


def run(c):
    if FORCE_FUSED is not None:
        c["fused"] = int(FORCE_FUSED)
    g = torch.Generator().manual_seed(rng.randrange(1 << 30))
    dd, inv, hid = c["data_dim"], c["inv"], c["hid"]
    kw = dict(hidden_dim_e=hid, hidden_dim_d=hid, activation=c["act"], sampler_d=c["sampler"], seed=rng.randrange(100),
              device="cuda")
    b, fam = c["b"], c["family"]
    x = torch.rand(b, *dd, generator=g)
    base = dict(data_dim=dd, latent_dim=c["latent"], invariances=inv, n_hidden_e=len(hid), n_hidden_d=len(hid),
                activation=c["act"], sampler=c["sampler"])
    tol = 2e-4
    if fam == "ivae":
        model = pv.models.iVAE(dd, c["latent"], inv, c_dim=c["c_dim"], **kw)
        cfg = orc.Config(c_dim=c["c_dim"], **base)
        eng = model.engine(fused=c["fused"])
        o = orc.SVIOracle({k: v.cpu() for k, v in model.state_dict().items()}, cfg)
        y = None
        if c["c_dim"]:
            y = torch.zeros(b, c["c_dim"]); y[torch.arange(b), torch.randint(0, c["c_dim"], (b,), generator=g)] = 1.0
        eps = torch.randn(b, cfg.z_dim, generator=g)
        eng.loss_and_grads(x.cuda(), eps.cuda(), c["beta"], None if y is None else y.cuda())
        loss = eng.scalars[0].item()
        ref = o.step(x, eps, c["beta"], y)
        grads = o.last_grads
    elif fam == "jivae":
        model = pv.models.jiVAE(dd, c["latent"], c["K"], inv, **kw)
        cfg = orc.Config(discrete_dim=c["K"], **base)
        eng = model.engine(fused=c["fused"])
        eps = torch.randn(b, cfg.z_dim, generator=g)
        eng.loss_and_grads(x.cuda(), eps.cuda(), c["beta"])
        o = orc.SVIOracle({k: v.cpu() for k, v in model.state_dict().items()}, cfg)
        loss = eng.scalars[0].item()
        ref = o.step(x, eps, c["beta"])
        grads = o.last_grads
        tol = 6e-3                                   # class-logit cancellation (see tests: jivae_grad_tol)
    elif fam == "ved":
        import warnings; warnings.filterwarnings("ignore")
        in_dim = rng.choice([(16, 16), (12, 20), (32,), (16, 8), (24,)])
        out_dim = rng.choice([(16,), (32,), (8, 12), (16, 16)])
        chans = lambda: rng.choice([4, 8, 16, 32])
        c1, c2, c3 = chans(), chans(), chans()
        # (a last encoder block with a single conv is inconsistent in the reference itself: its pooling rule then
        #  disagrees with the feature size convEncoderNet computes — not generated)
        he = rng.choice([[(c1,), (c2, c2)], [(c1, c1), (c2, c2)], [(c1,), (c2,), (c3, c3)]])
        hd = rng.choice([[(c2, c2), (c1,)], [(c3,), (c2, c2)], [(c2,), (c1,)]])
        bn = rng.random() < 0.4
        act = rng.choice(["lrelu", "relu", "tanh"])
        model = pv.models.VED(in_dim, out_dim, latent_dim=c["latent"], hidden_dim_e=he, hidden_dim_d=hd, activation=act,
                              batchnorm=bn, sampler_d=c["sampler"], seed=rng.randrange(100), device="cuda")
        vcfg = orc.VedConfig(input_dim=in_dim, output_dim=out_dim, latent_dim=c["latent"], hidden_dim_e=he, hidden_dim_d=hd,
                             activation=act, batchnorm=bn, sampler=c["sampler"])
        b = max(b, 2) if bn else b
        eng = model.engine(fused=c["fused"])
        o = orc.VedOracle({k: v.cpu() for k, v in model.state_dict().items()}, vcfg)
        xv = torch.rand(b, 1, *in_dim, generator=g); yv = torch.rand(b, 1, *out_dim, generator=g)
        eps = torch.randn(b, c["latent"], generator=g)
        eng.loss_and_grads(xv.cuda(), eps.cuda(), c["beta"], yv.cuda())
        loss = eng.scalars[0].item()
        ref = o.step(xv, yv, eps, c["beta"])
        grads = o.last_grads
        if act in ("relu", "lrelu"):
            # kinked activations: a pre-activation within rounding of 0 flips its gate; the fp64 oracle tells such a
            # tie (the fp32 ORACLE is then off by as much) from a real error
            o64 = orc.VedOracle({k: v.cpu() for k, v in model.state_dict().items()}, vcfg, dtype=torch.float64)
            o64.step(xv, yv, eps, c["beta"])
            c["_tie"] = {k: rel_l2(grads[k], o64.last_grads[k]) for k in grads}
        c["data_dim"] = in_dim; c["hid"] = "%s%s" % (he, "+bn" if bn else ""); c["act"] = act; c["b"] = b
        tol = 3e-2 if c["fused"] == 3 else (2e-3 if bn else 3e-4)
    else:
        task = "classification" if fam == "sscls" else "regression"
        dim = c["K"] if fam == "sscls" else rng.choice([1, 2])
        ctor = pv.models.ssiVAE if fam == "sscls" else pv.models.ss_reg_iVAE
        kw2 = dict(kw); he = kw2.pop("hidden_dim_e"); hd = kw2.pop("hidden_dim_d")
        model = ctor(dd, c["latent"], dim, inv, hidden_dim_e=he, hidden_dim_d=hd, **kw2)
        cfg = orc.Config(c_dim=dim, **base)
        eng = model.engine(lr=5e-4, fused=c["fused"])
        o = orc.SSOracle({k: v.cpu() for k, v in model.state_dict().items()}, cfg, task)
        labeled = rng.random() < 0.4
        xf = x.reshape(b, -1)
        ys = None
        if labeled:
            ys = torch.randn(b, dim, generator=g) if task == "regression" else torch.eye(dim)[torch.randint(0, dim, (b,), generator=g)]
        eps = torch.randn((dim, b, cfg.z_dim) if (task == "classification" and not labeled) else (b, cfg.z_dim), generator=g)
        eps_y = torch.randn(b, dim, generator=g) if (task == "regression" and not labeled) else None
        lt = eng.elbo_loss_and_grads(xf.cuda(), eps.cuda(), None if ys is None else ys.cuda(),
                                     None if eps_y is None else eps_y.cuda(), c["beta"])
        loss = lt.item()
        out = orc.ss_elbo(o.p, cfg, task, xf, eps, ys, eps_y, c["beta"], 0.5, o.grid)
        out["loss"].backward()
        ref = out["loss"].item()
        grads = {k: (torch.zeros_like(v) if v.grad is None else v.grad) for k, v in o.p.items()}
        tol = 3e-3
    msg, ties = [], []
    ltol = 3e-5
    if c["fused"] == 3:
        tol, ltol = max(tol, 5e-2), 5e-4
    if abs(loss - ref) > ltol * abs(ref) + 1e-4:
        msg.append("loss %.6f vs %.6f" % (loss, ref))
    gmax = max(v.abs().max().item() for v in grads.values())
    for k, gr in grads.items():
        gq = eng.grad_of(k)
        if gr.abs().max().item() < 1e-6 * gmax:
            if (gq.cpu() - gr).abs().max().item() > 1e-5 * gmax:
                msg.append("%s (tiny) abs %.1e" % (k, (gq.cpu() - gr).abs().max().item()))
            continue
        e = rel_l2(gq, gr)
        if not e < tol:
            tie = c.get("_tie", {}).get(k, 0.0)
            if tie > 0.25 * e:
                ties.append("%s %.1e (fp32 oracle vs fp64: %.1e)" % (k, e, tie))
            else:
                msg.append("%s %.1e" % (k, e))
    if ties and not msg:
        return "ok (activation tie: " + "; ".join(ties[:2]) + ")"
    return "ok" if not msg else "FAIL " + "; ".join(msg[:4])


bad = 0
for i in range(n_cases):
    c = case()
    try:
        res = run(c)
    except Exception as e:                               # noqa: BLE001
        res = "ERROR " + "".join(traceback.format_exception_only(type(e), e)).strip()[:160]
    if not (res.startswith("ok") or res.startswith("skip")):
        bad += 1
    print("%3d %-6s %-9s inv=%-6s hid=%-14s %-8s %-9s b=%-3d c=%d K=%d fused=%d beta=%.1f -> %s" % (
        i, c["family"], "x".join(map(str, c["data_dim"])), "".join(c["inv"] or ["-"]), str(c["hid"]), c["act"], c["sampler"], c["b"],
        c["c_dim"], c["K"], c["fused"], c["beta"], res), flush=True)
print("failures: %d of %d" % (bad, n_cases))
sys.exit(1 if bad else 0)
