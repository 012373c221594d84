#!/usr/bin/env python
"""Symbol-by-symbol comparison of a HIP source's gfx950 device assembly at two commits.

    python scripts/compare_kernel_asm.py [--source pv_sdec_fused_bf16.hip] [--base HEAD~1] [--keep DIR] [--define PV_EXPERIMENTS]
    python scripts/compare_kernel_asm.py --asm OLD.s NEW.s

Compiles pyroved_amd/csrc/<source> with `-S --cuda-device-only` under the Makefile's flags for that file — once from a
`git worktree` of the base commit, once from the working tree — and compares, for every function symbol of the base, the
text from its .type directive to its .size directive — the instructions and, for a kernel, the descriptor
(.amdhsa_kernel block: registers, scratch, LDS) the compiler emits in between — with the same symbol's in the new file.  Local labels
carry the function's ordinal in the translation unit (.LBB<fn>_<n>, .Lfunc_end<fn>, ...), which moves when functions are
added in front: the ordinal is normalised away, nothing else is.  Exit status 0 when every base symbol is present and
identical; symbols that exist only in the new file are listed, not compared.  Needs hipcc, no GPU.
"""
import argparse
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join("pyroved_amd", "csrc")


def makefile_flags(csrc_dir, stem):
    """CXXFLAGS + FLAGS_<stem> as pyroved_amd/csrc/Makefile spells them (ARCH = gfx950)."""
    text = open(os.path.join(csrc_dir, "Makefile")).read()

    def var(name):
        m = re.search(r"^%s\s*=\s*(.*)$" % re.escape(name), text, re.M)
        return m.group(1).strip() if m else ""

    flags = var("CXXFLAGS").replace("$(ARCH)", "gfx950") + " " + var("FLAGS_" + stem)
    return flags.split()


def compile_asm(csrc_dir, source, out, defines=()):
    stem = os.path.splitext(source)[0]
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    cmd = [hipcc] + makefile_flags(csrc_dir, stem) + ["-D" + d for d in defines] + ["-S", "--cuda-device-only", source, "-o", out]
    subprocess.check_call(cmd, cwd=csrc_dir, stderr=subprocess.DEVNULL)


_LOCAL = re.compile(r"\.L(BB|func_begin|func_end|tmp|JTI|CPI)(\d+)")


def _norm(line):
    line = line.split(";", 1)[0].rstrip()          # (comments carry nothing the assembler reads)
    return _LOCAL.sub(lambda m: ".L%s#" % m.group(1), line)


def symbols(path):
    """{name: normalised text} of every function (body and kernel descriptor) of an assembly file."""
    out = {}
    lines = open(path).read().splitlines()
    i, n = 0, len(lines)
    while i < n:
        m = re.match(r"\s*\.type\s+(\S+),@function", lines[i])
        if m:
            name, body = m.group(1), []
            i += 1
            while i < n and not re.match(r"\s*\.size\s+%s," % re.escape(name), lines[i]):
                t = _norm(lines[i])
                if t.strip():
                    body.append(t)
                i += 1
            out[name] = "\n".join(body)
        i += 1
    return out


def compare(old_s, new_s):
    a, b = symbols(old_s), symbols(new_s)
    missing = [k for k in a if k not in b]
    changed = [k for k in a if k in b and a[k] != b[k]]
    added = [k for k in b if k not in a]
    print("base symbols: %d   identical: %d   changed: %d   missing: %d   only in the new file: %d"
          % (len(a), len(a) - len(missing) - len(changed), len(changed), len(missing), len(added)))
    for k in changed:
        print("  CHANGED", k)
    for k in missing:
        print("  MISSING", k)
    for k in added:
        print("  new    ", k)
    return not missing and not changed


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--source", default="pv_sdec_fused_bf16.hip")
    ap.add_argument("--base", default="HEAD~1", help="commit to compare the working tree with")
    ap.add_argument("--keep", default=None, help="directory to leave the two .s files in")
    ap.add_argument("--define", action="append", default=[], metavar="NAME", help="compile both sides with -DNAME (the experiments build: PV_EXPERIMENTS)")
    ap.add_argument("--asm", nargs=2, metavar=("OLD.s", "NEW.s"), help="compare two assembly files already made")
    a = ap.parse_args()
    if a.asm:
        sys.exit(0 if compare(*a.asm) else 1)
    with tempfile.TemporaryDirectory() as tmp:
        keep = a.keep or tmp
        os.makedirs(keep, exist_ok=True)
        tree = os.path.join(tmp, "base")
        subprocess.check_call(["git", "-C", ROOT, "worktree", "add", "--detach", tree, a.base], stdout=subprocess.DEVNULL,
                              stderr=subprocess.DEVNULL)
        try:
            old_s, new_s = os.path.join(keep, "base.s"), os.path.join(keep, "new.s")
            compile_asm(os.path.join(tree, CSRC), a.source, old_s, a.define)
            compile_asm(os.path.join(ROOT, CSRC), a.source, new_s, a.define)
            ok = compare(old_s, new_s)
        finally:
            subprocess.call(["git", "-C", ROOT, "worktree", "remove", "--force", tree], stdout=subprocess.DEVNULL,
                            stderr=subprocess.DEVNULL)
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
