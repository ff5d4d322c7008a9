#!/usr/bin/env python3
"""Compare the gfx950 device code two source trees compile to.

    tools/codegen_compare.py PARENT_TREE BRANCH_TREE [file.hip ...]

Each tree is a checkout of this repository (a `git worktree` path serves as the parent).  Every csrc/*.hip of both trees is
compiled with the command its own Makefile would use for the object file (`make -n -B`, so per-file flags are the real ones),
with `-c` replaced by `--cuda-device-only -S`.  The `__hip_cuid_*` lines, which differ on every compile, are dropped.

Output: one line per file (`identical` = the whole device assembly matches line for line), then one line per kernel symbol:
`identical`, or both sides' resource tuple (vgpr_count, sgpr_count, LDS bytes, scratch bytes, occupancy, instructions, MFMAs).
Exit status 1 when a resource of any kernel differs (or a kernel exists on one side only), 0 otherwise.  A kernel whose
instructions were merely re-ordered or re-counted with equal resources is reported, not failed.

Reads compiler output only.  CPU only; not part of the pytest suite (a device compile takes seconds per file).
"""
import argparse
import os
import re
import shlex
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

CSRC = os.path.join("mnasnet_pytorch_amd", "csrc")
RESOURCES = ("vgpr", "lds", "scratch", "occupancy", "mfma")      # a difference in one of these fails the comparison


def compile_commands(tree):
    """{file.hip: argv} from the tree's own Makefile."""
    out = subprocess.run(["make", "-n", "-B", "-C", os.path.join(tree, CSRC), "all"], check=True, capture_output=True, text=True).stdout
    cmds = {}
    for line in out.splitlines():
        argv = shlex.split(line)
        if "-c" not in argv or "-o" not in argv:
            continue
        src = [a for a in argv if a.endswith(".hip")]
        if len(src) == 1:
            cmds[src[0]] = argv
    return cmds


def device_asm(tree, argv, src, outdir):
    dst = os.path.join(outdir, src[:-4] + ".s")
    o = argv.index("-o")
    cmd = argv[:o] + argv[o + 2:]
    cmd[cmd.index("-c"):cmd.index("-c") + 1] = ["--cuda-device-only", "-S"]
    subprocess.run(cmd + ["-o", dst], check=True, cwd=os.path.join(tree, CSRC))
    with open(dst) as f:
        return [l.rstrip() for l in f if "__hip_cuid_" not in l]


_LABEL = re.compile(r"^([A-Za-z_][\w$.]*):\s*; @")
# the ...ForWavesPerEU figures are the code object's .vgpr_count / .sgpr_count
_INFO = {"NumSGPRsForWavesPerEU": "sgpr", "NumVGPRsForWavesPerEU": "vgpr", "ScratchSize": "scratch", "Occupancy": "occupancy", "LDSByteSize": "lds"}
_INFO_RE = re.compile(r"^; (\w+): (\d+)")


def kernels(lines):
    """{symbol: {"body": [...], resources...}} for every .amdhsa_kernel of one assembly file."""
    funcs, cur, last = {}, None, None
    for l in lines:
        m = _LABEL.match(l)
        if m:
            cur = last = m.group(1)
            funcs[cur] = {"body": []}
        elif cur is not None:
            if l.startswith(".Lfunc_end"):
                cur = None
            else:
                funcs[cur]["body"].append(l)
        elif last is not None:
            m = _INFO_RE.match(l)
            if m and m.group(1) in _INFO:
                funcs[last].setdefault(_INFO[m.group(1)], int(m.group(2)))
    names = {l.split()[1] for l in lines if l.lstrip().startswith(".amdhsa_kernel ")}
    out = {}
    for n in names:
        f = funcs[n]
        ins = [b.split()[0] for b in f["body"] if b.startswith("\t") and b[1:2].isalpha()]
        f["insts"] = len(ins)
        f["mfma"] = sum(1 for i in ins if i.startswith("v_mfma"))
        out[n] = f
    return out


def demangle(names):
    try:
        r = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True)
        return dict(zip(names, r.stdout.splitlines()))
    except (OSError, subprocess.CalledProcessError):
        return {n: n for n in names}


def tup(k):
    return "vgpr %d sgpr %d lds %d scratch %d occ %d insts %d mfma %d" % tuple(
        k.get(x, -1) for x in ("vgpr", "sgpr", "lds", "scratch", "occupancy", "insts", "mfma"))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("parent")
    ap.add_argument("branch")
    ap.add_argument("files", nargs="*", help="restrict to these csrc file names")
    ap.add_argument("-j", "--jobs", type=int, default=16)
    a = ap.parse_args()
    jobs = max(1, min(16, a.jobs))
    cp, cb = compile_commands(a.parent), compile_commands(a.branch)
    files = sorted(set(cp) | set(cb))
    if a.files:
        files = [f for f in files if f in a.files]
    bad = 0
    with tempfile.TemporaryDirectory() as tmp, ThreadPoolExecutor(jobs) as pool:
        fut = {}
        for side, tree, cmds in (("parent", a.parent, cp), ("branch", a.branch, cb)):
            os.mkdir(os.path.join(tmp, side))
            for f in files:
                if f in cmds:
                    fut[side, f] = pool.submit(device_asm, tree, cmds[f], f, os.path.join(tmp, side))
        for f in files:
            if ("parent", f) not in fut or ("branch", f) not in fut:
                print("%s: only in %s" % (f, "parent" if ("parent", f) in fut else "branch"))
                continue
            lp, lb = fut["parent", f].result(), fut["branch", f].result()
            print("%s: %s" % (f, "identical" if lp == lb else "differs"))
            kp, kb = kernels(lp), kernels(lb)
            names = demangle(sorted(set(kp) | set(kb)))
            for n in sorted(names):
                if n not in kp or n not in kb:
                    print("  %s: only in %s" % (names[n], "parent" if n in kp else "branch"))
                    bad += 1
                    continue
                p, b = kp[n], kb[n]
                if p["body"] == b["body"] and all(p.get(r) == b.get(r) for r in RESOURCES):
                    print("  %s: identical" % names[n])
                    continue
                diff = [r for r in RESOURCES if p.get(r) != b.get(r)]
                print("  %s: %s\n      parent %s\n      branch %s" % (names[n], "RESOURCES DIFFER (%s)" % ", ".join(diff) if diff else "same resources",
                                                                    tup(p), tup(b)))
                bad += bool(diff)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
