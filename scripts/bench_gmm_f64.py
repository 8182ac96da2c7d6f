#!/usr/bin/env python3
"""One EM iteration of a Gaussian mixture (E-step + sufficient statistics) in fp64: the native
engine (csrc/gmm_f64.hip: fused MFMA E-step and statistics, no n x K responsibilities) against
the ``ops.gmm`` kernels behind ``engine="auto"`` (responsibilities [K, n], then the statistics
pass; they read fp64 rows, so fp32 rows are widened once beforehand, outside the timing) and
against the torch expressions of ``engine="torch"``. Device events, one warm-up, the median of
``--reps``, the engines alternated in one process; the peak of the allocator above the resident
rows is taken over one call of each engine. The torch expressions build [K, d, n] and [n, K]
tensors and a batched triangular solve that does not fit at every shape: they run on the first
``--torch-rows`` rows and their time and peak are reported for those rows; where even that
fails (the batched triangular solve's workspace) the torch figures are null. The useful fp64 rate
of the native engine counts 3 n K d^2 flops: the E-step twice (n K d^2 each, P is triangular) and the upper Gram (n K d^2)."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", type=str, default="1000000x32x64,1000000x64x16,4000000x16x8")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--torch-reps", type=int, default=3)
    ap.add_argument("--torch-rows", type=int, default=250_000)
    args = ap.parse_args()
    import torch

    from harp_amd.models import kernels as KM
    from harp_amd.ops import gmm as GM
    from harp_amd.ops import gmm_f64 as GF

    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(0)

    def ms(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        out = fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b), out

    def peak(fn):
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        out = fn()
        torch.cuda.synchronize()
        return (torch.cuda.max_memory_allocated() - base) / 2 ** 20, out

    for n, d, K in (tuple(int(v) for v in s.split("x")) for s in args.shapes.split(",")):
        mu = 3 * torch.randn(K, d, device=dev, generator=g, dtype=torch.float64)
        A = 0.3 * torch.randn(K, d, d, device=dev, generator=g, dtype=torch.float64)
        cov = A @ A.transpose(1, 2) + torch.eye(d, device=dev, dtype=torch.float64)
        w = torch.full((K,), 1.0 / K, device=dev, dtype=torch.float64)
        z = torch.randint(0, K, (n,), device=dev, generator=g)
        X64 = mu[z] + torch.randn(n, d, device=dev, generator=g, dtype=torch.float64)
        for dtype in (torch.float64, torch.float32):
            X = X64.to(dtype)
            Xw = X.double()  # what em_gmm's default path keeps for the whole run
            nt = min(n, args.torch_rows)
            Xt = Xw[:nt]

            def native():
                return GF.estep_stats(X, w, mu, cov, "full")

            def parent():
                R, ll = GM.estep(Xw, w, mu, cov, "full")
                return GM.stats(Xw, R, "full") + (ll,)

            def ref():
                logp = KM._log_gauss(Xt, mu, cov, "full") + torch.log(w)[None, :]
                lse = torch.logsumexp(logp, 1)
                R = torch.exp(logp - lse[:, None])
                return R.sum(0), R.t() @ Xt, torch.einsum("nk,ni,nj->kij", R, Xt, Xt), lse.sum()

            pk = {name: peak(fn) for name, fn in (("native", native), ("parent", parent))}  # warm-up
            try:
                pk["torch"] = peak(ref)
            except RuntimeError:
                pk["torch"] = None
            t = {"native": [], "parent": [], "torch": []}
            for i in range(args.reps):
                t["native"].append(ms(native)[0])
                t["parent"].append(ms(parent)[0])
                if pk["torch"] and i < args.torch_reps:
                    t["torch"].append(ms(ref)[0])
            med = {k: statistics.median(v) if v else None for k, v in t.items()}
            got, want = pk["native"][1], pk["parent"][1]
            print(json.dumps({
                "metric": "EM-GMM iteration fp64", "rows": str(dtype).split(".")[-1], "n": n, "d": d, "K": K,
                "splits": GF._kernels().harp_gmm_f64_splits(n, d, K),
                "native_ms": med["native"], "parent_ms": med["parent"], "torch_rows": nt,
                "torch_ms": med["torch"],
                "native_useful_tflops": 3.0 * n * K * d * d / (med["native"] * 1e-3) / 1e12,
                "parent_over_native": med["parent"] / med["native"], 
                "torch_over_native_per_row": (med["torch"] / nt) / (med["native"] / n) if med["torch"] else None,
                "native_peak_mib": pk["native"][0], "parent_peak_mib": pk["parent"][0], 
                "torch_peak_mib": pk["torch"][0] if pk["torch"] else None,
                "max_rel_s2_diff_to_parent": float(((got[2] - want[2]).abs().max() / want[2].abs().max()).item())}), flush=True)
            del X, Xw, Xt, pk
        del X64


if __name__ == "__main__":
    main()
