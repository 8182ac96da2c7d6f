#!/usr/bin/env python3
"""Per-kernel comparison of two device-only assembly listings of csrc/mf_sgd.hip.

Produce the listings with the HIP_FLAGS of harp_amd/ops/build.py plus
``--cuda-device-only -S`` (about a minute each), once at the parent commit and once at
the result, then:

    python profiles/sgd_shared_pieces/asm_diff.py parent.s result.s

Per kernel symbol it compares (a) the instruction stream with basic-block labels renumbered
in order of appearance and (b) the ``.amdhsa_`` descriptor lines (registers, LDS, private
segment, accum offset). It prints the count of identical kernels per family and, for the
rest, checks the limits a pure refactor has to keep: VGPR and SGPR counts do not rise, a
private segment of 0 stays 0, LDS is equal. Exit status 1 if a limit is broken."""
import collections
import re
import sys

FAMILIES = (("mf_sgd_xcd_placed_kernel", "placed"), ("mf_sgd_xcd_flow_kernel", "flow"), ("mf_sgd_xcd_wide_kernel", "wide-XCD"),
            ("mf_sgd_xcd_kernel", "xcd"), ("mf_sgd_wide_kernel", "wide"), ("mf_rmse_wide_kernel", "RMSE wide"),
            ("mf_rmse_kernel", "RMSE"), ("mf_sgd_kernel", "flat"))
LIMITS = ("next_free_vgpr", "next_free_sgpr", "group_segment_fixed_size", "private_segment_fixed_size")


def family(sym):
    return next((name for key, name in FAMILIES if key in sym), "other")


def parse(path):
    """symbol -> (normalised instruction list, {amdhsa key: value})"""
    body, meta = {}, {}
    cur = desc = None
    for line in open(path):
        s = line.split(";")[0].rstrip()
        t = s.strip()
        m = re.match(r"\.amdhsa_kernel\s+(\S+)", t)
        if m:
            desc = m.group(1)
            meta[desc] = {}
        elif t == ".end_amdhsa_kernel":
            desc = None
        elif desc is not None and t.startswith(".amdhsa_"):
            k, v = t.split(None, 1)
            meta[desc][k[len(".amdhsa_"):]] = v
        elif re.match(r"_Z\w+:$", t) and not s[0].isspace():
            cur = t[:-1]
            body[cur] = []
        elif t.startswith(".Lfunc_end"):
            cur = None
        elif cur is not None and t and (not t.startswith(".") or t.startswith(".LBB")):
            body[cur].append(t)
    out = {}
    for sym in meta:
        labels = {}
        norm = [re.sub(r"\.LBB\d+_\d+", lambda m: labels.setdefault(m.group(0), f"L{len(labels)}"), t)
                for t in body[sym]]
        out[sym] = (norm, meta[sym])
    return out


def main():
    a, b = parse(sys.argv[1]), parse(sys.argv[2])
    print(f"kernels: {len(a)} parent, {len(b)} result; only in parent {sorted(set(a) - set(b))}, "
          f"only in result {sorted(set(b) - set(a))}")
    stats = collections.defaultdict(lambda: collections.Counter())
    deltas = collections.defaultdict(list)
    broken, occupancy = [], []
    for sym in sorted(set(a) & set(b)):
        (ia, ma), (ib, mb) = a[sym], b[sym]
        f = family(sym)
        stats[f]["total"] += 1
        stats[f]["identical"] += ia == ib and ma == mb
        stats[f]["same descriptor"] += ma == mb
        if ia == ib and ma == mb:
            continue
        n_ins = lambda x: sum(not t.endswith(":") for t in x)
        deltas[f].append((n_ins(ib) - n_ins(ia), int(mb["next_free_vgpr"]) - int(ma["next_free_vgpr"]),
                          int(mb["next_free_sgpr"]) - int(ma["next_free_sgpr"])))
        # waves per SIMD the VGPR count allows (512 unified VGPRs, allocated in blocks of 8)
        waves = lambda m: min(8, 512 // (-(-int(m["next_free_vgpr"]) // 8) * 8))
        if waves(mb) != waves(ma):
            occupancy.append(f"{sym}: {waves(ma)} -> {waves(mb)} waves/SIMD")
        for k in LIMITS:
            va, vb = int(ma[k]), int(mb[k])
            bad = vb != va if k == "group_segment_fixed_size" else (vb > 0 and va == 0) if k.startswith("private") else vb > va
            if bad:
                broken.append(f"{sym}: {k} {va} -> {vb}")
    print(f"{'family':10s} {'kernels':>8s} {'identical':>10s} {'same descriptor':>16s}")
    for f, c in sorted(stats.items()):
        print(f"{f:10s} {c['total']:8d} {c['identical']:10d} {c['same descriptor']:16d}")
    for f, d in sorted(deltas.items()):
        ins, vg, sg = zip(*d)
        print(f"{f}: {len(d)} differ; instructions {min(ins):+d}..{max(ins):+d} (sum {sum(ins):+d}), "
              f"VGPRs {min(vg):+d}..{max(vg):+d}, SGPRs {min(sg):+d}..{max(sg):+d}")
    print(f"VGPR-limited waves per SIMD changed: {len(occupancy)}")
    for x in occupancy:
        print("  " + x)
    print(f"limits broken: {len(broken)}")
    for x in broken:
        print("  " + x)
    return 1 if broken else 0


if __name__ == "__main__":
    sys.exit(main())
