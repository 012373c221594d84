"""
_bf16_judge.py — the judge of the bf16 throughput step (fused = 3) against the reference that rounds where the kernel rounds
(oracle/bf16_plan.py), and its ceilings.  tests/test_gpu_bf16_emulated.py states the method; the particle, Renyi, Poisson and
partition-edge tests reuse it as it is.
"""
from _judge import rel_l2

# ceilings (the issue's paper estimate) — per-case bars are set from measurement, at most 4x the worst value seen
GRAD_CEIL, LOSS_CEIL, LOC_CEIL = 1e-3, 1e-5, 1e-4
SELF_CHECK = 10.0                          # a tensor more than 1e-3 from float64 lies at least 10x closer to the emulation
DECODE_BAR = 1.2e-6                        # model.decode vs float64: measured 2.42e-7 / 3.05e-7 (fp32-class build)
LIK = {"bernoulli": 0, "gaussian": 1, "continuous_bernoulli": 2}


def judge(case_name, eng, ref_out, ref_g, f64_out, f64_g, zl, zs, grad_bar, loss_bar, factor=10.0):
    """loss, z_loc / z_scale (1e-5) and every gradient tensor against the emulation, printed next to their distance from
    float64; returns the rows (quantity, vs emulation, vs float64)"""
    loss = eng.scalars[0].item()
    rows = []
    le = abs(loss - ref_out["loss"].item()) / abs(ref_out["loss"].item())
    rows.append(("loss", le, abs(loss - f64_out["loss"].item()) / abs(f64_out["loss"].item())))
    rows.append(("z_loc", rel_l2(zl, ref_out["z_loc"].detach()), rel_l2(zl, f64_out["z_loc"].detach())))
    rows.append(("z_scale", rel_l2(zs, ref_out["z_scale"].detach()), rel_l2(zs, f64_out["z_scale"].detach())))
    for key in ref_g:
        g = eng.grad_of(key)
        rows.append((key, rel_l2(g, ref_g[key]), rel_l2(g, f64_g[key])))
    print("\n[bf16-emulated] %s" % case_name)
    for key, e_em, e_64 in rows:
        print("  %-42s vs emulated %.3e   vs float64 %.3e" % (key, e_em, e_64))
    assert le < loss_bar, "%s: loss %.3e from the emulation (bar %.1e)" % (case_name, le, loss_bar)
    for key, e_em, e_64 in rows[1:]:
        bar = 1e-5 if key.startswith("z_") else grad_bar
        assert e_em < bar, "%s: %s %.3e from the emulation (bar %.1e)" % (case_name, key, e_em, bar)
        if e_64 > 1e-3:   # the emulation must explain the error, not just sit under a lucky bar
            assert e_em * factor <= e_64, "%s: %s %.3e from the emulation, %.3e from float64" % (case_name, key, e_em, e_64)
    return rows
