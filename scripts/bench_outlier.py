"""Stand-alone timing of the native outlier engine on one GPU (not part of bench.py).

    python scripts/bench_outlier.py [--n 10000000 --d 32 --dtypes fp32,fp64 --runs 10 --warmup 3]

Per dtype, on n x d data with 1 % planted outliers, median of ``--runs`` after ``--warmup``:
  * one ``ops.outlier.mahalanobis_pass`` (whitened distance, mask, statistics) in both statistics
    forms, and its ratio to the read floor (bytes of X over ``--hbm-tbs`` TB/s);
  * the same pass without statistics, and the univariate pass;
  * a full BACON fit with the native and (unless ``--no-torch``) the torch engine, with the
    iteration counts and whether the two give the same weights.
One JSON line per measurement.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from harp_amd.models import stats as ST  # noqa: E402
from harp_amd.ops import outlier as OL  # noqa: E402

DTYPES = {"bf16": torch.bfloat16, "fp32": torch.float32, "fp64": torch.float64}


def timed(fn, runs: int, warmup: int) -> float:
    """Median wall time of fn() in milliseconds, the device drained before and after each run."""
    out = []
    for i in range(warmup + runs):
        torch.cuda.synchronize()
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        if i >= warmup:
            out.append((time.perf_counter() - t) * 1e3)
    return statistics.median(out)


def planted(n: int, d: int, dtype, dev) -> torch.Tensor:
    g = torch.Generator(device=dev).manual_seed(1)
    X = torch.empty((n, d), dtype=dtype, device=dev)
    step = 1 << 20
    for a in range(0, n, step):  # in slices: no n x d temporary in another dtype
        b = min(n, a + step)
        Y = torch.randn(b - a, d, generator=g, device=dev, dtype=torch.float32)
        bad = torch.rand(b - a, generator=g, device=dev) < 0.01
        Y[bad] += 25.0
        X[a:b] = Y.to(dtype)
    return X


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=10_000_000)
    ap.add_argument("--d", type=int, default=32)
    ap.add_argument("--dtypes", default="fp32,fp64")
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--hbm-tbs", type=float, default=8.0, help="HBM bandwidth of the read floor, TB/s")
    ap.add_argument("--no-torch", action="store_true", help="skip the torch engine's BACON fit")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    for name in a.dtypes.split(","):
        dtype = DTYPES[name]
        X = planted(a.n, a.d, dtype, dev)
        base = {"n": a.n, "d": a.d, "dtype": name, "runs": a.runs, "warmup": a.warmup}
        floor_ms = X.numel() * X.element_size() / (a.hbm_tbs * 1e12) * 1e3
        sub = X[:1 << 20].double()
        c = sub.mean(0)
        P = OL.whiten(torch.cov(sub.t()))
        del sub
        t2 = float(a.d + 3 * (2 * a.d) ** 0.5)
        mask = torch.zeros(a.n, dtype=torch.uint8, device=dev)
        for form, flags in (("mfma", 0), ("vector", OL.VECTOR_STATS)):
            ms = timed(lambda: OL.mahalanobis_pass(X, c, P, t2, c, mask=mask, flags=flags), a.runs, a.warmup)
            print(json.dumps(dict(base, what="mahalanobis_pass", stats=form, ms=round(ms, 4),
                                  read_floor_ms=round(floor_ms, 4), ratio_to_floor=round(ms / floor_ms, 3))),
                  flush=True)
        ms = timed(lambda: OL.mahalanobis_pass(X, c, P, t2, c, mask=mask, want_stats=False), a.runs, a.warmup)
        print(json.dumps(dict(base, what="mahalanobis_pass", stats="none", ms=round(ms, 4),
                              read_floor_ms=round(floor_ms, 4), ratio_to_floor=round(ms / floor_ms, 3))), flush=True)
        sc = torch.ones_like(c)
        ms = timed(lambda: OL.univariate(X, c, sc, 3.0), a.runs, a.warmup)
        print(json.dumps(dict(base, what="univariate", ms=round(ms, 4))), flush=True)
        res = {}
        ms = timed(lambda: res.update(native=ST.bacon_native(X)), a.runs, a.warmup)
        print(json.dumps(dict(base, what="bacon_fit", engine="native", ms=round(ms, 3),
                              iterations=res["native"]["iterations"],
                              inliers=int(res["native"]["weights"].sum()))), flush=True)
        if not a.no_torch:
            ms = timed(lambda: res.update(torch=ST.outliers_bacon(X)), a.runs, a.warmup)
            print(json.dumps(dict(base, what="bacon_fit", engine="torch", ms=round(ms, 3),
                                  inliers=int(res["torch"].sum()),
                                  same_weights=bool(torch.equal(res["torch"], res["native"]["weights"])))),
                  flush=True)
        del X, mask, res
        torch.cuda.empty_cache()
    return 0


if __name__ == "__main__":
    sys.exit(main())
