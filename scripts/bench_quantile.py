#!/usr/bin/env python3
"""Quantiles by radix select (csrc/quantile.hip) at 1e7 x 100 fp32 and 2e6 x 100 fp64, q = (0.1,
0.5, 0.9), against the only thing the torch engine's formulation can do above 2**24 elements,
``torch.sort(X, 0)`` plus indexing and the same interpolation; and at 1e5 x 100 (below the
limit) against ``stats.quantiles(engine="torch")`` itself.

Also the histogram kernel alone, pass by pass, on prefixes from a real select run, with the
shared-digit path off (the default) and on, for three kinds of data: normal, one constant, integers 0..3.

Protocol: HIP-event time per call, 2 warm-ups, median of 10. The read floor of an engine run is
``passes * bytes / HBM bandwidth`` at the 8 TB/s peak of the MI355X. One JSON line per case.
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_BYTES_PER_S = 8e12


def main():
    import torch

    from harp_amd.models import stats as ST
    from harp_amd.ops import quantile as QT

    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=float, default=1.0, help="multiplies every row count (rehearsal)")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_quantile needs a GPU"
    dev = torch.device("cuda", 0)
    q = (0.1, 0.5, 0.9)
    lines = []

    def timed(fn, reps=args.reps):
        for _ in range(2):
            fn()
        ms = []
        for _ in range(reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            ms.append(e0.elapsed_time(e1))
        return statistics.median(ms), min(ms), max(ms)

    def emit(rec):
        lines.append(rec)
        print(json.dumps(rec), flush=True)

    def sort_quantiles(X):
        n = X.shape[0]
        r = torch.tensor(q, dtype=torch.float64) * (n - 1)
        lo, hi = r.floor().long().to(dev), r.ceil().long().to(dev)
        S = torch.sort(X, 0).values
        return torch.lerp(S[lo].double(), S[hi].double(), (r - r.floor()).to(dev)[:, None])

    def block(kind, n, d, dtype):
        g = torch.Generator(device=dev).manual_seed(0)
        if kind == "normal":
            return torch.randn(n, d, generator=g, device=dev, dtype=dtype)
        if kind == "constant":
            return torch.full((n, d), 1.5, device=dev, dtype=dtype)
        return torch.randint(0, 4, (n, d), generator=g, device=dev).to(dtype)

    for n0, dtype in ((10_000_000, torch.float32), (2_000_000, torch.float64), (100_000, torch.float32)):
        n, d = max(1, int(n0 * args.scale)), 100
        X = block("normal", n, d, dtype)
        nbytes = X.numel() * X.element_size()
        floor_ms = QT.passes(dtype) * nbytes / HBM_BYTES_PER_S * 1e3
        got = ST.quantiles(X, q, engine="native")
        ref = sort_quantiles(X)
        assert torch.equal(got, ref), "native engine differs from sort"
        nat = timed(lambda: ST.quantiles(X, q, engine="native"))
        srt = timed(lambda: sort_quantiles(X))
        rec = {"case": "engine", "rows": n, "dim": d, "dtype": str(dtype), "bytes": nbytes, "passes": QT.passes(dtype),
               "native_ms": nat, "sort_ms": srt, "sort_over_native": srt[0] / nat[0], "read_floor_ms": floor_ms,
               "floor_over_native": floor_ms / nat[0]}
        if X.numel() <= ST.TORCH_QUANTILE_MAX:
            tq = timed(lambda: ST.quantiles(X, q))
            assert torch.equal(got, ST.quantiles(X, q))
            rec.update(torch_engine_ms=tq, torch_engine_over_native=tq[0] / nat[0])
        emit(rec)
        del X, got, ref

    # the histogram kernel alone, with and without the shared-digit path
    for n0, dtype in ((10_000_000, torch.float32), (2_000_000, torch.float64)):
        n, d = max(1, int(n0 * args.scale)), 100
        for kind in ("normal", "constant", "categorical"):
            X = block(kind, n, d, dtype)
            nbytes = X.numel() * X.element_size()
            r = torch.tensor(q, dtype=torch.float64) * (n - 1)
            ranks = torch.cat([r.floor(), r.ceil()]).long().tolist()
            T = len(ranks)
            prefix = torch.zeros((d, T), dtype=torch.int64, device=dev)
            remaining = torch.tensor(ranks, dtype=torch.int64, device=dev).repeat(d, 1)
            for p in range(QT.passes(dtype)):
                before = prefix.clone()
                hist, _ = QT.digit_histogram(X, before, p)
                shared, _ = QT.digit_histogram(X, before, p, QT.SHARED_DIGIT)
                assert torch.equal(hist, shared)
                off = timed(lambda: QT.digit_histogram(X, before, p))
                on = timed(lambda: QT.digit_histogram(X, before, p, QT.SHARED_DIGIT))
                floor_ms = nbytes / HBM_BYTES_PER_S * 1e3
                emit({"case": "hist", "data": kind, "rows": n, "dim": d, "dtype": str(dtype), "pass": p, "targets": T,
                      "plain_ms": off, "shared_ms": on, "shared_over_plain": on[0] / off[0],
                      "read_floor_ms": floor_ms, "floor_over_plain": floor_ms / off[0]})
                QT.pick(hist, prefix, remaining, p, dtype)
            del X

    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            for rec in lines:
                f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
