#!/usr/bin/env python3
"""CSR statistics kernels (csrc/csr_stats.hip) at n = 1e6, d = 1000 and densities 0.1 %, 1 %,
5 %: both forced Gram paths, col_moments, spmm + argmax at C = 20, against the formulation
``ops.linalg.gram`` used for sparse input before these kernels (CSR^T @ dense copy) in fp32,
as it ran, and in fp64, the precision the policy promises.

Protocol: HIP-event time per call, 3 warm-ups, median of 10 (a formulation whose single call
exceeds ``--slow-s`` seconds gets 1 warm-up and the median of 3; its row says so). Peak
memory is the rise of ``torch.cuda.max_memory_allocated`` across one call. Without
``--density`` the script runs one child process per density, each under its own time limit,
and stops at the first that fails. One JSON line per density.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def one_density(args):
    import torch

    from harp_amd.ops import csr_stats as CS

    assert torch.cuda.is_available(), "bench_csr_stats needs a GPU"
    dev = torch.device("cuda", 0)
    n, d, C = args.rows, args.dim, args.classes
    z = max(1, round(args.density * d))
    g = torch.Generator(device=dev).manual_seed(0)
    cols = torch.randint(0, d, (n * z,), device=dev, generator=g)
    rows = torch.arange(n, device=dev).repeat_interleave(z)
    vals = torch.rand(n * z, device=dev, generator=g, dtype=torch.float64) * 2.0 - 0.5
    X = torch.sparse_coo_tensor(torch.stack([rows, cols]), vals, (n, d)).coalesce().to_sparse_csr()
    del cols, rows, vals
    A = CS.to_csr_operand(X)
    m = (A.rowptr[1:] - A.rowptr[:-1]).double()
    nb = (d + CS.GRAM_TILE - 1) // CS.GRAM_TILE
    res = {"rows": n, "dim": d, "density": args.density, "nnz": A.nnz, "sum_m2": float((m * m).sum()),
           "nnz2_over_n": A.nnz * A.nnz / n, "tiled_visits": n * nb * (nb + 1) // 2,
           "chooser": CS.gram_path(n, d, A.nnz), "GRAM_TILE": CS.GRAM_TILE, "MOM_LDS_MAX_D": CS.MOM_LDS_MAX_D}

    def timed(fn):
        """(median ms, peak MiB, repetitions, last result)"""
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.memory_allocated()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = fn()
        e1.record()
        torch.cuda.synchronize()
        peak = (torch.cuda.max_memory_allocated() - before) / 2 ** 20
        slow = e0.elapsed_time(e1) > 1e3 * args.slow_s
        warm, reps = (0, 3) if slow else (2, 10)  # the call above was the first warm-up
        for _ in range(warm):
            out = fn()
        ts = []
        for _ in range(reps):
            e0.record()
            out = fn()
            e1.record()
            torch.cuda.synchronize()
            ts.append(e0.elapsed_time(e1))
        return statistics.median(ts), peak, reps, out

    def put(name, fn):
        ms, peak, reps, out = timed(fn)
        res[name + "_ms"], res[name + "_peak_mib"] = round(ms, 4), round(peak, 1)
        if reps != 10:
            res[name + "_reps"] = reps
        return out

    put("block_offsets", lambda: (setattr(A, "blk", None), CS.block_offsets(A))[1])
    Gt = put("gram_tiled", lambda: CS.gram(A, path="tiled"))
    for tgt in args.sweep_workgroups:
        rps = max(256, -(-n // max(1, tgt // (nb * (nb + 1) // 2))))
        put(f"gram_tiled_wg{tgt}", lambda: CS.gram(A, path="tiled", rows_per_split=rps))
    Gd = put("gram_direct", lambda: CS.gram(A, path="direct"))
    put("col_moments", lambda: CS.col_moments(A))
    B = torch.rand(d, C, device=dev, dtype=torch.float64, generator=g)
    bias = torch.rand(C, device=dev, dtype=torch.float64, generator=g)
    put("spmm_argmax", lambda: CS.spmm(A, B, bias, argmax=True))

    def before(dtype):  # ops.linalg.gram's sparse branch before the CSR kernels, verbatim
        Xc = X.to_sparse_csr().to(dtype)
        return Xc.t() @ Xc.to_dense()

    scale = float(Gt.abs().max())
    res["tiled_vs_direct_max_rel"] = float((Gt - Gd).abs().max()) / scale
    for name, dtype in ([] if args.skip_before else [("before_fp64", torch.float64), ("before_fp32", torch.float32)]):
        try:
            Gb = put(name, lambda: before(dtype))
            res[name + "_vs_tiled_max_rel"] = float((Gt - torch.triu(Gb).double()).abs().max()) / scale
            del Gb
        except RuntimeError as e:  # reported, not hidden: the formulation itself may not run at this size
            res[name + "_error"] = str(e).splitlines()[0][:200]
    print(json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--dim", type=int, default=1000)
    ap.add_argument("--classes", type=int, default=20)
    ap.add_argument("--density", type=float, default=None, help="one density in this process")
    ap.add_argument("--densities", type=float, nargs="*", default=[0.001, 0.01, 0.05])
    ap.add_argument("--sweep-workgroups", type=int, nargs="*", default=[],
                    help="extra tiled timings at these workgroup targets")
    ap.add_argument("--slow-s", type=float, default=1.0)
    ap.add_argument("--skip-before", action="store_true")
    ap.add_argument("--step-timeout", type=int, default=240, help="seconds per density")
    args = ap.parse_args()
    if args.density is not None:
        return one_density(args)
    for p in args.densities:
        cmd = ["timeout", "-k", "10", str(args.step_timeout), sys.executable, os.path.abspath(__file__),
               "--density", str(p)] + [a for a in sys.argv[1:]]
        rc = subprocess.run(cmd).returncode
        if rc != 0:
            print(json.dumps({"density": p, "failed_rc": rc}), flush=True)
            return rc
    return 0


if __name__ == "__main__":
    sys.exit(main() or 0)
