"""
_decoder_choice_cases.py — what tests/golden/make_decoder_choice.py records and tests/test_decoder_choice_cpu.py replays: which
fused decoder kernel a launch runs and everything the host derives from that decision (pv_sdec_fused.h: PvDecChoice).

Two records, both made of host-side queries that dereference nothing and need no device (pv_sdec_fused_grid answers for 256 CUs):
  plans  pv_ivae_plan structs through the public size and routing queries (workspace bytes of every entry-point family, uses_fused,
         guide_folds, the weighted route and its kernel names);
  table  the grid (fused, units, grads, sel) through pv_debug_decoder_choice and the kernel-name hooks — once per library build and,
         for the experiments build, once per setting of its environment switches (read once per process: a fresh one each).

Run as a program it prints one table as JSON: `python _decoder_choice_cases.py LIBRARY` — the fresh process of a row of CONFIGS.
That path imports ctypes alone.
"""
import ctypes as C
import json
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
PKG = os.path.join(os.path.dirname(HERE), "pyroved_amd")
SHIPPED, EXPERIMENTS = os.path.join(PKG, "libpyroved_amd.so"), os.path.join(PKG, "libpyroved_amd_exp.so")

# ------------------------------------------------------------------------------- the choice table
FUSED = (1, 2, 3)
# both sides of every switch of the size rule on 256 CUs: the H231 build (1024), the 8-wave kernels (6 x 256), the H221 build
# (32768), the row cap (2^26 units = 2^30 rows)
UNITS = (1, 255, 256, 1023, 1024, 1535, 1536, 1537, 32767, 32768, 2 ** 26 - 1, 2 ** 26, 2 ** 27)
# every dec_kernel pv_sdec_fused_sel_valid accepts in either build, and three it accepts in none
SELS = (0, 1, 2, 21, 28, 4, 8, 23, 31, 33, 26, 27, 29, 41, 48, 3, 5, 99)
LIKS = (0, 1, 2, 3)
FIELDS = ("sel_valid", "family", "prec", "x3_waves", "ds", "waves", "rec_fmt", "parks", "park_bytes", "img_mode", "img_scale_bits",
          "img_qswap", "weighted", "hosts_guide")
# name -> (library, environment of the fresh process)
CONFIGS = {"shipped": ("shipped", {}), "experiments": ("experiments", {})}
CONFIGS.update({"PV_W8=%s" % v: ("experiments", {"PV_W8": v}) for v in ("0", "1")})
CONFIGS.update({"PV_X3_KERNEL=%s" % v: ("experiments", {"PV_X3_KERNEL": v}) for v in ("o", "4", "8", "h221", "h231", "w221", "w231")})
SWITCHES = ("PV_W8", "PV_X3_KERNEL", "PV_FD_ABLATE", "PV_QSWAP")


def table(lib_path):
    """{"choice": [[14 integers] per (fused, units, grads, sel)], "names": [name per (fused, units, grads, lik)], "fold_names": ...}"""
    lib = C.CDLL(lib_path)
    lib.pv_debug_decoder_choice.restype = C.c_int
    lib.pv_debug_decoder_choice.argtypes = [C.c_int, C.c_int64, C.c_int, C.c_int, C.POINTER(C.c_int64)]
    lib.pv_debug_decoder_kernel_name.restype = C.c_char_p
    lib.pv_debug_decoder_kernel_name.argtypes = [C.c_int, C.c_int64, C.c_int, C.c_int]
    lib.pv_debug_decoder_kernel_name_fold.restype = C.c_char_p
    lib.pv_debug_decoder_kernel_name_fold.argtypes = [C.c_int, C.c_int]
    out = (C.c_int64 * len(FIELDS))()
    choice = []
    for fused in FUSED:
        for units in UNITS:
            for grads in (0, 1):
                for sel in SELS:
                    assert lib.pv_debug_decoder_choice(fused, units, grads, sel, out) == 0
                    choice.append(list(out))
    names = [lib.pv_debug_decoder_kernel_name(fused, units, grads, lik).decode()
             for fused in FUSED for units in UNITS for grads in (0, 1) for lik in LIKS]
    fold = [lib.pv_debug_decoder_kernel_name_fold(grads, lik).decode() for grads in (0, 1) for lik in LIKS]
    return {"choice": choice, "names": names, "fold_names": fold}


def table_rows():
    return [(fused, units, grads, sel) for fused in FUSED for units in UNITS for grads in (0, 1) for sel in SELS]


def table_of(config, libs=None):
    """The table of one row of CONFIGS from a fresh process (libs: {"shipped": path, "experiments": path}, default this tree's)."""
    which, extra = CONFIGS[config]
    path = (libs or {"shipped": SHIPPED, "experiments": EXPERIMENTS})[which]
    env = {k: v for k, v in os.environ.items() if k not in SWITCHES}
    env.update(extra)
    out = subprocess.run([sys.executable, os.path.abspath(__file__), path], env=env, check=True, stdout=subprocess.PIPE).stdout
    return json.loads(out)


# ------------------------------------------------------------------------------- the plans
DEC_KERNELS = (0, 1, 2, 21, 28, 7)                   # (7: valid in no mode)
PLAN_LIKS = ("bernoulli", "gaussian", "continuous_bernoulli", "poisson_log")
PLAN_FLAGS = (0, 512, 16)                            # none, PV_PLAN_FAST_WEIGHTS, PV_PLAN_NO_ENC_FOLD
# batches that put units = batch * positions / 16 on both sides of 256 (the grid), 1024, 1536 and 32768
SHAPES = (((16,), (255, 256, 257, 1023, 1024, 1535, 1536, 1537)),
          ((8, 8), (255, 256, 383, 384, 385)),
          ((28, 28), (6, 256, 257, 669)))
# fake addresses of (params, x) for pv_ivae_guide_folds, which looks at their alignment: a 16-aligned pair and a misaligned one
ADDRESSES = ((0x10000, 0x20000), (0x10004, 0x20008))
QUERIES = ("ws_all", "ws_step", "ws_encode", "ws_decode", "obj_elbo_1", "obj_renyi_1", "obj_elbo_3", "obj_renyi_3", "evidence_1",
           "evidence_4", "weighted_ws", "uses_fused", "guide_folds", "guide_folds_misaligned", "weighted_uses_fused",
           "wname_shared_fwd", "wname_shared_grads", "wname_image_fwd", "wname_image_grads")


def plan_cases():
    """[(label, plan)]: the fc-encoder iVAE on the fused architecture (tests/_plan_kit.py) over fused x dec_kernel x likelihood x
    flags x c_dim x (shape, batch), jiVAE K = 3 at a few of them, and one vanilla-decoder plan"""
    import _plan_kit as kit
    from pyroved_amd import _abi

    def make(shape, batch, fused, dk, lik, flags, c_dim, K=0):
        p = kit._small_plan(discrete_dim=K, fused=fused)
        n = 1
        for d in shape:
            n *= d
        p.batch, p.n_pix, p.coord_dim, p.c_dim = batch, n, len(shape), c_dim
        p.has_r = 1 if len(shape) == 2 else 0
        p.z_dim = p.latent_dim + p.has_r + len(shape)
        p.enc[0].in_dim = n + c_dim
        p.head.out_dim = 2 * p.z_dim + K
        p.fc_coord.in_dim = len(shape)
        p.fc_latent.in_dim = p.latent_dim + c_dim + K
        p.lik, p.sigmoid_out, p.decoder_sig = _abi.LIK[lik], 0 if lik == "poisson_log" else 1, 0.5
        p.dec_kernel, p.flags = dk, flags
        return p

    cases = []
    for shape, batches in SHAPES:
        for batch in batches:
            for fused in (0, 1, 2, 3):
                for dk in DEC_KERNELS:
                    for lik in PLAN_LIKS:
                        for flags in PLAN_FLAGS:
                            for c_dim in (0, 2):
                                key = (shape, batch, fused, dk, lik, flags, c_dim)
                                cases.append((key, make(*key)))
    for shape, batch in (((16,), 256), ((8, 8), 384), ((28, 28), 6)):
        for fused in (0, 1, 2, 3):
            for dk in (0, 1, 28):
                cases.append(((shape, batch, fused, dk, "jiVAE K=3"), make(shape, batch, fused, dk, "bernoulli", 0, 0, K=3)))
    for fused in (0, 2, 3):
        cases.append(("vanilla f%d" % fused, kit._vanilla_plan(fused)))
    return cases


def plan_record(lib, p):
    """What the library answers for one plan, in the order of QUERIES (lib: a CDLL with _abi.SIGNATURES applied)"""
    from pyroved_amd import _abi
    ref = C.byref(p)
    p.params, p.x = ADDRESSES[0]
    rec = [lib.pv_ivae_workspace_bytes_for(ref, what) for what in (0, 1, 2, 3)]
    for P in (1, 3):
        for bound in (_abi.PV_BOUND_ELBO, _abi.PV_BOUND_RENYI):
            o = _abi.pv_ivae_objective()
            o.num_particles, o.bound, o.alpha = P, bound, 0.5
            rec.append(lib.pv_ivae_objective_workspace_bytes(ref, C.byref(o)))
    rec += [lib.pv_ivae_evidence_workspace_bytes(ref, P) for P in (1, 4)]
    rec += [lib.pv_ivae_weighted_workspace_bytes(ref), lib.pv_ivae_uses_fused(ref), lib.pv_ivae_guide_folds(ref)]
    p.params, p.x = ADDRESSES[1]
    rec.append(lib.pv_ivae_guide_folds(ref))
    p.params, p.x = ADDRESSES[0]
    rec.append(lib.pv_ivae_weighted_uses_fused(ref))
    fn = lib.pv_debug_weighted_decoder_kernel_name
    fn.restype, fn.argtypes = C.c_char_p, [C.POINTER(_abi.pv_ivae_plan), C.c_int, C.c_int]
    rec += [fn(ref, per_image, grads).decode() for per_image in (0, 1) for grads in (0, 1)]
    return rec


def open_lib(path):
    from pyroved_amd import _abi
    lib = C.CDLL(path)
    for name, (res, args) in _abi.SIGNATURES.items():
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = res, args
    return lib


def plans(lib_path=SHIPPED):
    lib = open_lib(lib_path)
    return [plan_record(lib, p) for _, p in plan_cases()]


# ------------------------------------------------------------------------------- the files' form
def pack(records, group):
    """[record] -> {"records": every distinct record once, "groups": every distinct run of `group` consecutive records once, as
    indices, "order": the runs in order, "tail": the records behind the last whole run}"""
    def intern(items):
        seen, index, out = [], {}, []
        for it in items:
            if it not in index:
                index[it] = len(seen)
                seen.append(it)
            out.append(index[it])
        return seen, out
    distinct, idx = intern([tuple(r) for r in records])
    n = len(idx) // group * group
    groups, order = intern([tuple(idx[i:i + group]) for i in range(0, n, group)])
    return {"records": distinct, "groups": groups, "order": order, "tail": idx[n:]}


def unpack(data):
    idx = [i for g in data["order"] for i in data["groups"][g]] + data["tail"]
    return [list(data["records"][i]) for i in idx]


# plans: the eleven sizes in units of the carver's 256-byte alignment (negative: an error code, kept), every distinct value once
# ("values_256") and every distinct row of eleven as indices into them ("sizes"); the eight routing answers, every distinct row once
# ("routes"); then the plans as (sizes row, routes row)
N_SIZES, PLAN_GROUP = 11, 24                       # (24: likelihood x flags x c_dim of one (shape, batch, fused, dec_kernel))


def pack_plans(records):
    assert all(v < 0 or v % 256 == 0 for r in records for v in r[:N_SIZES])
    values = sorted({v // 256 if v > 0 else v for r in records for v in r[:N_SIZES]})
    at = {v: i for i, v in enumerate(values)}
    sizes = pack([[at[v // 256 if v > 0 else v] for v in r[:N_SIZES]] for r in records], 1)
    routes = pack([r[N_SIZES:] for r in records], 1)
    first = lambda p: [p["groups"][g][0] for g in p["order"]]
    return {"values_256": values, "sizes": sizes["records"], "routes": routes["records"],
            "plans": pack(list(zip(first(sizes), first(routes))), PLAN_GROUP)}


def unpack_plans(data):
    size = [v * 256 if v > 0 else v for v in data["values_256"]]
    return [[size[i] for i in data["sizes"][s]] + list(data["routes"][t]) for s, t in unpack(data["plans"])]


# table: the configurations one behind the other; runs of one (fused, units, grads): 18 selections, 4 likelihoods, 8 fold names
def pack_tables(tables):
    cat = lambda key: [r for c in CONFIGS for r in tables[c][key]]
    return {"configs": list(CONFIGS), "choice": pack(cat("choice"), len(SELS)), "names": pack([[n] for n in cat("names")], len(LIKS)),
            "fold_names": pack([[n] for n in cat("fold_names")], 8)}


def unpack_tables(data):
    out = {c: {} for c in data["configs"]}
    for key, one in (("choice", list), ("names", lambda r: r[0]), ("fold_names", lambda r: r[0])):
        rows = [one(r) for r in unpack(data[key])]
        per = len(rows) // len(data["configs"])
        for i, c in enumerate(data["configs"]):
            out[c][key] = rows[i * per:(i + 1) * per]
    return out


if __name__ == "__main__":
    json.dump(table(sys.argv[1]), sys.stdout, separators=(",", ":"))
