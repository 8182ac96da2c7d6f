#!/usr/bin/env python3
"""SVD of a tall fp64 block: the d x d step alone, ``ops.jsvd.svd_small`` (csrc/jsvd.hip)
against ``torch.linalg.svd`` on the same TSQR factor, with and without the rotations W; then
``stats.svd`` with engine="native" against engine="torch" on n rows.
Warm-up, then the median of ``--reps`` timed calls, each ended by a device synchronise.
One JSON line per measurement.

python scripts/bench_svd.py [--n 1e6] [--ds 8,32,64,96,128] [--reps 10]
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=float, default=1e6)
    ap.add_argument("--ds", default="8,32,64,96,128")
    ap.add_argument("--reps", type=int, default=10)
    a = ap.parse_args()
    import torch

    from harp_amd.models import stats as ST
    from harp_amd.ops import jsvd as JS

    def median_s(fn):
        fn()
        torch.cuda.synchronize()
        ts = []
        for _ in range(a.reps):
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ts.append(time.perf_counter() - t0)
        return statistics.median(ts)

    n = int(a.n)
    for d in [int(x) for x in a.ds.split(",")]:
        g = torch.Generator(device="cuda").manual_seed(d)
        X = torch.randn(n, d, dtype=torch.float64, device="cuda", generator=g)
        M = torch.linalg.qr(X[:4096], mode="r")[1].t().contiguous()
        Z, s, W, sweeps = JS.svd_small(M)
        ref = torch.linalg.svdvals(M)
        print(json.dumps({
            "metric": "d x d SVD seconds (median)", "d": d, "reps": a.reps, "sweeps": int(sweeps),
            "svd_small_s": median_s(lambda: JS.svd_small(M)),
            "svd_small_no_w_s": median_s(lambda: JS.svd_small(M, want_w=False)),
            "torch_svd_s": median_s(lambda: torch.linalg.svd(M)),
            "torch_svdvals_s": median_s(lambda: torch.linalg.svdvals(M)),
            "max_rel_s_diff": float((s - ref).abs().max() / ref[0])}), flush=True)
        res = {"metric": "stats.svd seconds (median)", "n": n, "d": d, "reps": a.reps}
        for want_u in (True, False):
            for engine in ("native", "torch"):
                res[f"{engine}{'' if want_u else '_no_u'}_s"] = median_s(
                    lambda: ST.svd(X, want_u=want_u, engine=engine))
        print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
