#!/usr/bin/env python3
"""The K-means tail (span-ordered sort + resolve + label finish after the keyless sweep) timed over
candidate spans in one process, HIP events; the measurement behind ops.kmeans.RESOLVE_SPAN.

python scripts/kmeans_tail_onepass_ab.py [--spans 20 21 22 23 --rounds 4 --reps 3 --out FILE]
The spans alternate inside every round; a round's figure is the median of its reps. Every span's
labels are compared with those of K.assign, its sums with K.assign's to rounding. (The gates of
profiles/kmeans_tail_onepass ran an earlier form of this script that also held the per-span loop
and the scattered-store kernel, neither of which ships.)"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    import torch

    from harp_amd.ops import kmeans as K
    from harp_amd.ops import segment

    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=float, default=1e8)
    ap.add_argument("--k", type=int, default=10000)
    ap.add_argument("--d", type=int, default=100)
    ap.add_argument("--spans", type=int, nargs="+", default=[20, 21, 22, 23], help="log2 of the spans")
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    n = int(a.n)
    X = K.generate_points(n, a.d, 0, 1000, seed=1, device=dev)
    op = K.prepare(torch.rand(a.k, a.d, device=dev) * 1000, X.shape[1])
    lab = torch.empty(n, dtype=torch.int32, device=dev)
    sums = torch.zeros((K.padded_k(a.k), X.shape[1]), dtype=torch.float32, device=dev)
    K.assign(X, op, sums=sums, labels=lab, want_objective=False)
    torch.cuda.synchronize()
    final, ref_sums = lab.clone(), sums.clone()
    glab = lab // 32  # what the sweep leaves: the 32-row group
    ng = K.swept_k(op) // 32

    def tail(span):
        perm, start, rank, rowof = segment.bucket_labels_spans(lab, ng, span, want_rank=True)
        segment.resolve_rowsum(X, op.Cm2, perm, start, rowof, sums, NG=ng)
        segment.finish_labels(lab, rank, rowof)

    def timed(span):
        lab.copy_(glab)
        sums.zero_()
        s, e = torch.cuda.Event(True), torch.cuda.Event(True)
        s.record()
        tail(span)
        e.record()
        e.synchronize()
        return s.elapsed_time(e)

    res = {"n": n, "k": a.k, "d": a.d, "rounds": a.rounds, "reps": a.reps, "spans": {}}
    for sh in a.spans:  # warm-up (workspace) and the result check
        timed(1 << sh)
        ok = bool(torch.equal(lab, final))
        err = float((sums - ref_sums).abs().max() / ref_sums.abs().max())
        res["spans"][f"2^{sh}"] = {"labels_equal": ok, "sums_max_diff_over_max": err, "round_median_ms": []}
    for _ in range(a.rounds):
        for sh in a.spans:
            t = [timed(1 << sh) for _ in range(a.reps)]
            res["spans"][f"2^{sh}"]["round_median_ms"].append(round(statistics.median(t), 4))
    for key, v in res["spans"].items():
        print(key, v, flush=True)
    print(json.dumps(res), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
