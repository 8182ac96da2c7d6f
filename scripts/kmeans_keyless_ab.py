"""Keyed (variant 15) against keyless (variant 16) K-means assign in one process on the same
seeded points and centroids: label differences (each must be a near tie), sums agreement for
the clusters no differing point touches, and alternating timings of [sweep, bucket, sum].

python scripts/kmeans_keyless_ab.py [--n 1e8] [--k 10000] [--d 100] [--rounds 3] [--out FILE]
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from harp_amd.ops import _lib, kmeans as K, segment  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=float, default=1e8)
    ap.add_argument("--k", type=int, default=10000)
    ap.add_argument("--d", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    n, d = int(a.n), a.d
    dev = torch.device("cuda", 0)
    lib = _lib.kernels()
    X = K.generate_points(n, d, 0, 1000, seed=1, device=dev)
    torch.manual_seed(0)
    c = torch.rand(a.k, d, device=dev) * 1000
    op = K.prepare(c, X.shape[1])
    Kp, ks = op.Cm2.shape[0], K.swept_k(op)
    lab = {v: torch.empty(n, dtype=torch.int32, device=dev) for v in (15, 16)}
    sums = {v: torch.zeros((Kp, X.shape[1]), dtype=torch.float32, device=dev) for v in (15, 16)}

    def sweep(v):
        _lib.check(lib.harp_kmeans_assign(X.data_ptr(), X.stride(0), op.Cm2.data_ptr(), n, X.shape[1], ks, d,
                                          lab[v].data_ptr(), None, 0, None, None, v, _lib.stream_ptr(dev)), "assign")

    def ev():
        e = torch.cuda.Event(enable_timing=True)
        e.record()
        return e

    def bucket_sum(v):
        """[(before bucket, before sum, after sum)]: the keyless path sorts by (span of
        K.RESOLVE_SPAN points, group), resolves and finishes the labels (as ops.kmeans.assign does)."""
        sums[v].zero_()
        e0 = ev()
        if v == 15:
            perm, start = segment.bucket_labels(lab[v], Kp)
            e1 = ev()
            segment.bucket_rowsum(X, perm, start, sums[v])
        else:
            perm, start, rank, rowof = segment.bucket_labels_spans(lab[v], ks // 32, K.RESOLVE_SPAN, want_rank=True)
            e1 = ev()
            segment.resolve_rowsum(X, op.Cm2, perm, start, rowof, sums[v], NG=ks // 32)
            segment.finish_labels(lab[v], rank, rowof)
        return [(e0, e1, ev())]

    times = {}
    for r in range(a.rounds + 1):  # round 0 warms up
        for v in (15, 16):
            e0 = ev()
            sweep(v)
            e1 = ev()
            marks = bucket_sum(v)
            marks[-1][2].synchronize()
            if r:
                t = [e0.elapsed_time(e1), sum(m[0].elapsed_time(m[1]) for m in marks),
                     sum(m[1].elapsed_time(m[2]) for m in marks)]
                times.setdefault(v, []).append(t)
                print(f"round {r} variant {v}: sweep {t[0]:.2f} bucket {t[1]:.2f} sum {t[2]:.2f} total {sum(t):.2f} ms",
                      flush=True)
    l15, l16 = lab[15].long(), lab[16].long()
    assert int(l16.min()) >= 0 and int(l16.max()) < a.k
    idx = (l15 != l16).nonzero().flatten()
    c_bf = c.to(torch.bfloat16).double()
    cn = (c_bf ** 2).sum(1)
    worst, bad = 0.0, 0
    for i0 in range(0, idx.numel(), 1 << 20):
        ii = idx[i0:i0 + (1 << 20)]
        x = X[ii, :d].double()
        ga = cn[l16[ii]] - 2.0 * (x * c_bf[l16[ii]]).sum(1)
        gb = cn[l15[ii]] - 2.0 * (x * c_bf[l15[ii]]).sum(1)
        rel = (ga - gb).abs() / ga.abs()
        worst = max(worst, rel.max().item())
        bad += int((rel > 2.0 ** -17).sum())
    touched = torch.zeros(Kp, dtype=torch.bool, device=dev)
    touched[l15[idx]] = True
    touched[l16[idx]] = True
    s15, s16 = sums[15][~touched][:, : d + 1], sums[16][~touched][:, : d + 1]
    sums_ok = bool(torch.allclose(s15, s16, rtol=1e-5, atol=1e-2))
    counts_ok = int(sums[16][:, d].double().sum().item()) == n
    med = {v: [sorted(t[i] for t in times[v])[len(times[v]) // 2] for i in range(3)] for v in times}
    out = {"n": n, "k": a.k, "d": d, "labels_differing": int(idx.numel()), "near_tie_violations": bad,
           "worst_rel_gap": worst, "near_tie_bound": 2.0 ** -17, "untouched_clusters": int((~touched).sum()),
           "untouched_sums_agree": sums_ok, "count_total_ok": counts_ok,
           "median_ms_sweep_bucket_sum": {str(v): [round(x, 3) for x in med[v]] for v in med},
           "median_ms_total": {str(v): round(sum(med[v]), 3) for v in med},
           "rounds_ms": {str(v): [[round(x, 3) for x in t] for t in times[v]] for v in times}}
    print(json.dumps(out, indent=1))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
    return 0 if bad == 0 and sums_ok else 1


if __name__ == "__main__":
    sys.exit(main())
