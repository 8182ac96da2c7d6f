#!/usr/bin/env python3
"""fp64 kNN benchmark: the native engine (csrc/knn_f64.hip, MFMA distances with the top-k fused)
against ``engine="torch"`` (fp64 distance tile + torch.topk) on fp64 and fp32 rows, both computed
in fp64 (the torch engine widens fp32 rows first). Two shapes: many queries, and a small query set
that the launcher splits over the training rows. Median of ``--reps`` after a warm-up, the two
engines alternated in one process. The native search is timed with its operand prepared
beforehand (the classifier's steady state); prepare is reported on its own. Where the torch
engine's distance tile does not fit, it runs on the first ``--torch-queries`` queries in tiles of
``--torch-tile`` and its time is reported per query."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--train", type=int, default=1_000_000)
    ap.add_argument("--dim", type=int, default=32)
    ap.add_argument("--k", type=int, default=16)
    ap.add_argument("--queries", type=str, default="16384,1000")
    ap.add_argument("--torch-queries", type=int, default=2048)
    ap.add_argument("--torch-tile", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=10)
    args = ap.parse_args()
    import torch

    from harp_amd.models import kernels as KM
    from harp_amd.ops import knn_f64 as KF

    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(0)

    def ms(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        out = fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b), out

    for M in (int(v) for v in args.queries.split(",")):
        for dtype in (torch.float64, torch.float32):
            T = torch.randn(args.train, args.dim, device=dev, generator=g, dtype=dtype)
            Q = torch.randn(M, args.dim, device=dev, generator=g, dtype=dtype)
            Mt = min(M, args.torch_queries)
            Td = T.double()
            W = KF.prepare(T)
            native = lambda: KF.knn_search(T, Q, args.k, operand=W)
            ref = lambda: KM.knn_search(Td, Q[:Mt].double(), args.k, tile=args.torch_tile, engine="torch")
            native(), ref()  # warm-up
            tn, tt, tp = [], [], []
            for _ in range(args.reps):
                t, (dn, _) = ms(native)
                tn.append(t)
                t, (dt, _) = ms(ref)
                tt.append(t)
                tp.append(ms(lambda: KF.prepare(T))[0])
            tn_, tt_ = statistics.median(tn), statistics.median(tt)
            print(json.dumps({
                "metric": "fp64 kNN search", "rows": str(dtype).split(".")[-1], "train": args.train, "queries": M,
                "dim": args.dim, "k": args.k, "splits": KF._kernels().harp_knn_f64_splits(M, args.train, args.dim, args.k),
                "native_search_ms": tn_, "native_useful_tflops": 2.0 * M * args.train * args.dim / (tn_ * 1e-3) / 1e12,
                "native_prepare_ms": statistics.median(tp), "torch_queries": Mt, "torch_ms": tt_,
                "native_us_per_query": 1e3 * tn_ / M, "torch_us_per_query": 1e3 * tt_ / Mt,
                "torch_over_native_per_query": (tt_ / Mt) / (tn_ / M),
                "max_abs_dist_diff": float((dn[:Mt] - dt).abs().max().item())}), flush=True)
            del T, Q, Td, W


if __name__ == "__main__":
    main()
