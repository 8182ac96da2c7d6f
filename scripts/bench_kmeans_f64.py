#!/usr/bin/env python3
"""One dense fp64 K-means step: ``kmeans_sparse(X, C0, 1, engine="native")`` (csrc/kmeans_f64.hip)
against ``engine="torch"`` ([n, K] distance tensor, one-hot, GEMM), and the assign and sums
kernels alone. Warm-up, then ``--reps`` timed calls per engine, the engines alternated inside
one loop, each call ended by a device synchronise; the native engine is timed twice in that
loop (a, b), so the spread of the same code is on record next to the difference between engines.
Kernel times are device events around ``--inner`` back-to-back launches (median of ``--reps``).

python scripts/bench_kmeans_f64.py [--shapes 1e6:32:256:fp32,1e6:32:256:fp64,1e7:100:1000:fp32] [--reps 10]
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

FP64_MATRIX_PEAK = 78.6e12  # MI355X fp64 matrix FLOP/s (spec sheet)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="1e6:32:256:fp32,1e6:32:256:fp64,1e7:100:1000:fp32")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--inner", type=int, default=5)
    ap.add_argument("--torch-limit", type=float, default=4e9,
                    help="largest n * K at which the torch engine is timed; above it one call is attempted "
                         "and what happens is recorded")
    a = ap.parse_args()
    import torch

    from harp_amd.models import kmeans_csr as M
    from harp_amd.ops import kmeans_f64 as KF
    from harp_amd.ops import segment as SG

    if not torch.cuda.is_available():
        raise SystemExit("bench_kmeans_f64: needs a GPU")
    dev = torch.device("cuda", 0)

    def once(fn):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t0

    def events(fn):
        fn()
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        ts = []
        for _ in range(a.reps):
            ev[0].record()
            for _ in range(a.inner):
                fn()
            ev[1].record()
            torch.cuda.synchronize()
            ts.append(ev[0].elapsed_time(ev[1]) / a.inner * 1e-3)
        return statistics.median(ts)

    for spec in a.shapes.split(","):
        n, d, K, dt = spec.split(":")
        n, d, K = int(float(n)), int(d), int(K)
        dtype = {"bf16": torch.bfloat16, "fp32": torch.float32, "fp64": torch.float64}[dt]
        g = torch.Generator(device=dev).manual_seed(d)
        X = (torch.rand(n, d, device=dev, generator=g) * 1000).to(dtype)
        C0 = X[:K].double()
        step = {e: (lambda e=e: M.kmeans_sparse(X, C0, 1, engine=e)) for e in ("native", "torch")}
        res = {"metric": "one K-means step, seconds", "n": n, "d": d, "K": K, "dtype": dt, "reps": a.reps}
        with_torch = n * K <= a.torch_limit
        if not with_torch:
            try:
                res["torch_single_call_s"] = once(step["torch"])
            except RuntimeError as e:  # torch.OutOfMemoryError is one
                res["torch_engine"] = type(e).__name__ + ": " + str(e).split(". ")[0]
            torch.cuda.empty_cache()
        runs = {"native_a": step["native"], "native_b": step["native"]}
        if with_torch:
            runs["torch"] = step["torch"]
        for fn in runs.values():
            once(fn)
        ts = {k: [] for k in runs}
        for _ in range(a.reps):
            for k, fn in runs.items():
                ts[k].append(once(fn))
        for k, v in ts.items():
            res[k + "_s"] = statistics.median(v)
            res[k + "_min_max_s"] = [min(v), max(v)]
        # the kernels alone
        lab = KF.assign(X, C0)
        perm, start = SG.bucket_labels(lab, K)
        kern = KF._kernels()
        W = torch.empty(kern.harp_kmeans_f64_operand_doubles(K, d), dtype=torch.float64, device=dev)
        sums, wss = torch.zeros(K, d, dtype=torch.float64, device=dev), torch.zeros(K, dtype=torch.float64, device=dev)
        code, st = KF._DTYPES[dtype], torch.cuda.current_stream().cuda_stream
        kern.harp_kmeans_f64_prepare(C0.data_ptr(), d, K, d, W.data_ptr(), st)
        res["assign_kernel_s"] = events(lambda: kern.harp_kmeans_f64_assign(
            X.data_ptr(), code, n, X.stride(0), d, W.data_ptr(), K, lab.data_ptr(), st))
        res["sums_kernel_s"] = events(lambda: kern.harp_kmeans_f64_sums(
            X.data_ptr(), code, n, X.stride(0), d, C0.data_ptr(), perm.data_ptr(), start.data_ptr(), K,
            sums.data_ptr(), wss.data_ptr(), st))
        res["bucket_labels_s"] = events(lambda: SG.bucket_labels(lab, K))
        flops = 2.0 * n * K * d
        res["assign_useful_fp64_flops"] = flops / res["assign_kernel_s"]
        res["assign_share_of_fp64_matrix_peak"] = res["assign_useful_fp64_flops"] / FP64_MATRIX_PEAK
        res["assign_padded_width"] = KF.padded_width(d)
        if with_torch:
            same = M.kmeans_sparse(X, C0, 1, engine="torch")["labels"] == M.kmeans_sparse(X, C0, 1, engine="native")["labels"]
            res["labels_equal_fraction"] = float(same.double().mean())
        print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
