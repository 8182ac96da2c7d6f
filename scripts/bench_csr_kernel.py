#!/usr/bin/env python3
"""Sparse kernel matrices (csrc/csr_kernel.hip): the RBF kernel of two CSR operands,
n = m = 20,000, d = 10,000 at densities 0.1 %, 1 % and 5 %, and one bag-of-words shape
(d = 1e6, 50 nonzeros per row), both forced paths, against what the library did for two
sparse operands before these kernels: ``to_dense`` + GEMM + ``harp_rbf_from_gram``, where the
dense operands fit (``--dense-limit-gib``).

Protocol: HIP-event time per call, 3 warm-ups, median of 10 (a formulation whose single call
exceeds ``--slow-s`` seconds gets 1 warm-up and the median of 3; its row says so). Peak
memory is the rise of ``torch.cuda.max_memory_allocated`` across one call, the operands
already resident. Without ``--case`` the script runs one child process per case, each under
its own time limit, and stops at the first that fails. One JSON line per case.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def operand(n, d, z, seed, dev):
    """CSR operand with z sorted distinct columns per row (one per stratum of d // z columns)."""
    import torch

    from harp_amd.ops import csr_stats as CS

    g = torch.Generator(device=dev).manual_seed(seed)
    span = d // z
    cols = (torch.arange(z, device=dev) * span)[None, :] + torch.randint(0, span, (n, z), device=dev, generator=g)
    vals = torch.rand(n * z, device=dev, generator=g, dtype=torch.float64) * 2.0 - 0.5
    return CS.CSROperand(torch.arange(n + 1, device=dev) * z, cols.reshape(-1).to(torch.int32), vals, n, d)


def one_case(args):
    import torch

    from harp_amd.models import kernels as KF
    from harp_amd.ops import csr_kernel as CK

    assert torch.cuda.is_available(), "bench_csr_kernel needs a GPU"
    dev = torch.device("cuda", 0)
    n, d, z = args.rows, args.dim, args.case
    X, Y = operand(n, d, z, 1, dev), operand(n, d, z, 2, dev)
    cell = z * CK.KERNEL_TILE * CK.KERNEL_SLAB / d
    res = {"rows": n, "dim": d, "nnz_per_row": z, "density": z / d, "entries_per_cell": round(cell, 3),
           "chooser": CK.kernel_path(n, n, d, X.nnz, Y.nnz), "TILE": CK.KERNEL_TILE, "SLAB": CK.KERNEL_SLAB,
           "operand_mib": round(2 * X.nnz * 12 / 2 ** 20, 1), "output_mib": round(n * n * 8 / 2 ** 20, 1)}

    def timed(fn):
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
        res[name + "_ms"], res[name + "_peak_mib"] = round(ms, 3), round(peak, 1)
        if reps != 10:
            res[name + "_reps"] = reps
        return out

    sigma = (z ** 0.5)  # distances of the order of z: kernel values away from 0 and 1
    CK.kernel_block(X, Y, "rbf", sigma=sigma, rows=(0, 64))  # row norms cached, as in a second call
    Km = put("merge", lambda: CK.kernel_block(X, Y, "rbf", sigma=sigma, path="merge"))
    Ks = put("slab", lambda: CK.kernel_block(X, Y, "rbf", sigma=sigma, path="slab"))
    res["paths_bitwise_equal"] = bool(torch.equal(Km, Ks))
    del Ks
    if 2 * n * d * 8 <= args.dense_limit_gib * 2 ** 30:
        Xs = torch.sparse_csr_tensor(X.rowptr, X.col.long(), X.val, size=(n, d))
        Ys = torch.sparse_csr_tensor(Y.rowptr, Y.col.long(), Y.val, size=(n, d))
        Kd = put("densify_gemm", lambda: KF.rbf_kernel(Xs.to_dense(), Ys.to_dense(), sigma))
        res["dense_vs_merge_max_abs"] = float((Kd - Km).abs().max())
    else:
        res["densify_gemm_skipped"] = f"two dense operands are {2 * n * d * 8 / 2 ** 30:.0f} GiB"
    print(json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=20_000)
    ap.add_argument("--dim", type=int, default=10_000)
    ap.add_argument("--case", type=int, default=None, help="nonzeros per row: one case in this process")
    ap.add_argument("--densities", type=float, nargs="*", default=[0.001, 0.01, 0.05])
    ap.add_argument("--bow-dim", type=int, default=1_000_000, help="bag-of-words case (0: skip)")
    ap.add_argument("--bow-nnz", type=int, default=50)
    ap.add_argument("--slow-s", type=float, default=1.0)
    ap.add_argument("--dense-limit-gib", type=float, default=16.0)
    ap.add_argument("--step-timeout", type=int, default=240, help="seconds per case")
    args = ap.parse_args()
    if args.case is not None:
        return one_case(args)
    cases = [(args.dim, max(1, round(p * args.dim))) for p in args.densities]
    if args.bow_dim:
        cases.append((args.bow_dim, args.bow_nnz))
    for d, z in cases:
        cmd = ["timeout", "-k", "10", str(args.step_timeout), sys.executable, os.path.abspath(__file__),
               "--rows", str(args.rows), "--dim", str(d), "--case", str(z), "--slow-s", str(args.slow_s),
               "--dense-limit-gib", str(args.dense_limit_gib)]
        rc = subprocess.run(cmd).returncode
        if rc != 0:
            print(json.dumps({"dim": d, "nnz_per_row": z, "failed_rc": rc}), flush=True)
            return rc
    return 0


if __name__ == "__main__":
    sys.exit(main() or 0)
