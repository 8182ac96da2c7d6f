#!/usr/bin/env python3
"""Pivoted QR of a tall fp64 block: ``stats.pivoted_qr`` with engine="native" (Householder
TSQR + the d x d kernel of csrc/pqr.hip, everything on the device) against engine="host"
(copy to the host, LAPACK dgeqp3, CPU tensors back), and the d x d kernel alone.
Warm-up, then the median of ``--reps`` timed calls, each ended by a device synchronise.

python scripts/bench_pqr.py [--n 1e6] [--ds 18,64,128] [--reps 10]
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
    ap.add_argument("--ds", default="18,64,128")
    ap.add_argument("--reps", type=int, default=10)
    a = ap.parse_args()
    import torch

    from harp_amd.models import stats as ST
    from harp_amd.ops import pqr as PQ

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
        R1 = torch.linalg.qr(X[:4096], mode="r")[1].contiguous()
        res = {"metric": "pivoted QR seconds (median)", "n": n, "d": d, "reps": a.reps,
               "native_s": median_s(lambda: ST.pivoted_qr(X, engine="native")),
               "host_s": median_s(lambda: ST.pivoted_qr(X, engine="host")),
               "qrcp_small_s": median_s(lambda: PQ.qrcp_small(R1))}
        # harp_pqr_small alone (qrcp_small also scales and reads |R|_max back): device events
        # around 20 back-to-back launches
        from harp_amd.ops import _lib

        A = (R1 / R1.abs().max()).contiguous()
        Q2, R2, pm = torch.empty_like(A), torch.empty_like(A), torch.empty(d, dtype=torch.int32, device="cuda")
        launch = lambda: _lib.check(PQ._kernels().harp_pqr_small(  # noqa: E731
            A.data_ptr(), d, d, Q2.data_ptr(), R2.data_ptr(), pm.data_ptr(), _lib.stream_ptr(A.device)), "pqr_small")
        launch()
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        ts = []
        for _ in range(a.reps):
            ev[0].record()
            for _ in range(20):
                launch()
            ev[1].record()
            torch.cuda.synchronize()
            ts.append(ev[0].elapsed_time(ev[1]) / 20 * 1e-3)
        res["kernel_s"] = statistics.median(ts)
        nat, host = ST.pivoted_qr(X, engine="native"), ST.pivoted_qr(X, engine="host")
        res["same_permutation"] = bool(torch.equal(nat["permutation"].cpu(), host["permutation"].long()))
        res["max_abs_diagR_diff"] = float((nat["R"].diagonal().cpu().abs() - host["R"].diagonal().abs()).abs().max())
        print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
