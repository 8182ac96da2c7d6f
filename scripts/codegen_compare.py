#!/usr/bin/env python3
"""Per-kernel comparison of the gfx950 code two source trees generate (host only, no GPU).

    git archive --prefix=parent/ HEAD~1 | tar -x -C /tmp/cg
    python scripts/codegen_compare.py /tmp/cg/parent . --out /tmp/cg/out

Every ``csrc/*.hip`` of both trees is compiled with the build's HIP_FLAGS plus
``--cuda-device-only -S -Rpass-analysis=kernel-resource-usage``. The assembly is split by
kernel symbol; the ``__hip_cuid_*`` symbol and basic-block label numbers are normalised. Per
kernel it prints identical / differs, the instruction count and the compiler's resource table
(VGPRs, AGPRs, SGPRs, spills, scratch, LDS, occupancy), and whether the symbol lists are equal.
A listing that is newer than its source and headers is reused. Exit status 1 if the symbol
lists differ or a kernel that differs also changes a count."""
import argparse
import concurrent.futures as cf
import glob
import importlib.util
import os
import re
import subprocess
import sys

# harp_amd/ops/build.py by path: the flags are the build's own, and torch is not imported
_spec = importlib.util.spec_from_file_location(
    "harp_build", os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "harp_amd", "ops", "build.py"))
_build = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(_build)
CSRC, HIP_FLAGS, HIPCC = _build.CSRC, _build.HIP_FLAGS, _build.HIPCC

FIELDS = (("VGPRs", "vgpr"), ("AGPRs", "agpr"), ("TotalSGPRs", "sgpr"), ("VGPRs Spill", "vspill"), ("SGPRs Spill", "sspill"),
          ("ScratchSize [bytes/lane]", "scratch"), ("LDS Size [bytes/block]", "lds"), ("Occupancy [waves/SIMD]", "occ"))


def compile_one(tree, src, out):
    """csrc/<src> of `tree` -> (<out>/<src>.s, <out>/<src>.remarks)"""
    path = os.path.join(tree, "csrc", src)
    asm, rem = os.path.join(out, src + ".s"), os.path.join(out, src + ".remarks")
    deps = [path] + glob.glob(os.path.join(tree, "csrc", "*.h"))
    if not (os.path.exists(asm) and os.path.exists(rem) and all(os.path.getmtime(d) < os.path.getmtime(asm) for d in deps)):
        flags = ["-I" + os.path.join(tree, "csrc") if f == "-I" + CSRC else f for f in HIP_FLAGS]
        cmd = [HIPCC] + flags + ["--cuda-device-only", "-S", "-Rpass-analysis=kernel-resource-usage", path, "-o", asm]
        r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        if r.returncode != 0:
            raise RuntimeError(f"{' '.join(cmd)}\n{r.stdout}")
        open(rem, "w").write(r.stdout)
    return asm, rem


def parse(asm, rem):
    """kernel symbol -> (normalised instruction list, {field: value})"""
    kernels = set(re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", open(asm).read(), re.M))
    body, cur = {}, None
    for line in open(asm):
        t = line.split(";")[0].strip()
        if line[:1] not in " \t." and re.match(r"\w+:$", t) and t[:-1] in kernels:
            cur = body.setdefault(t[:-1], [])
        elif t.startswith(".Lfunc_end"):
            cur = None
        elif cur is not None and t and (not t.startswith(".") or t.startswith(".LBB")):
            cur.append(re.sub(r"__hip_cuid_\w+", "__hip_cuid", t))
    res, name = {}, None
    for line in open(rem):
        m = re.search(r"remark: .*Function Name: (\S+)", line)
        if m:
            name = m.group(1)
        for label, key in FIELDS:
            m = re.search(r"remark: .*\s" + re.escape(label) + r": (\d+)", line)
            if m and name:
                res.setdefault(name, {})[key] = int(m.group(1))
    out = {}
    for sym, ins in body.items():
        labels = {}
        norm = [re.sub(r"\.LBB\d+_\d+", lambda m: labels.setdefault(m.group(0), f"L{len(labels)}"), t) for t in ins]
        out[sym] = (norm, dict(res.get(sym, {}), ins=sum(not t.endswith(":") for t in norm)))
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("parent")
    ap.add_argument("result")
    ap.add_argument("--out", default="build/codegen", help="directory for the listings")
    ap.add_argument("--jobs", type=int, default=16)
    ap.add_argument("--ignore", default="", help="regex of kernel symbols that may exist in one tree only")
    a = ap.parse_args()
    trees = {"parent": a.parent, "result": a.result}
    srcs = {k: sorted(os.path.basename(p) for p in glob.glob(os.path.join(t, "csrc", "*.hip"))) for k, t in trees.items()}
    print(f"sources: {len(srcs['parent'])} parent, {len(srcs['result'])} result; "
          f"in one tree only: {sorted(set(srcs['parent']) ^ set(srcs['result']))}")
    with cf.ThreadPoolExecutor(max_workers=min(a.jobs, 16)) as ex:
        futs = {}
        for k, t in trees.items():
            os.makedirs(os.path.join(a.out, k), exist_ok=True)
            for s in srcs[k]:
                futs[k, s] = ex.submit(compile_one, t, s, os.path.join(a.out, k))
        parsed = {k: {s: parse(*futs[k, s].result()) for s in srcs[k]} for k in trees}
    cols = ["ins"] + [key for _, key in FIELDS]
    bad = 0
    for s in sorted(set(srcs["parent"]) | set(srcs["result"])):
        p, r = parsed["parent"].get(s, {}), parsed["result"].get(s, {})
        only = sorted(x for x in set(p) ^ set(r) if not (a.ignore and re.search(a.ignore, x)))
        same = sum(p[k][0] == r[k][0] for k in set(p) & set(r))
        print(f"\n{s}: {len(p)} parent kernels, {len(r)} result kernels, {same} identical; "
              f"symbol lists {'equal' if not only else 'DIFFER: ' + ', '.join(only)}")
        bad += len(only)
        print(f"  {'':9s} " + " ".join(f"{c:>7s}" for c in cols) + "  kernel")
        for k in sorted(set(p) & set(r)):
            (ip, mp), (ir, mr) = p[k], r[k]
            print(f"  {'identical' if ip == ir else 'differs':9s} " + " ".join(f"{mr.get(c, -1):7d}" for c in cols) + f"  {k}")
            if mp != mr:
                bad += 1
                print(f"  {'parent':9s} " + " ".join(f"{mp.get(c, -1):7d}" for c in cols))
    print(f"\nsymbol-list or count differences: {bad}")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
