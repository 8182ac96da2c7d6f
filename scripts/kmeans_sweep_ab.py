"""Sweep-only A/B of K-means assign variants in one process on the same seeded points and
centroids: the variants alternate for --rounds rounds of --reps sweeps each (HIP-event times), and
every variant's labels are compared bit for bit with the first one's. For rows of
KM_VARIANT_TABLE that write the same kind of label (all keyed, or all keyless).

python scripts/kmeans_sweep_ab.py --variants 16,17 [--n 1e8 --k 10000 --d 100 --rounds 4 --reps 3] [--out FILE]
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from harp_amd.ops import _lib, kmeans as K  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=float, default=1e8)
    ap.add_argument("--k", type=int, default=10000)
    ap.add_argument("--d", type=int, default=100)
    ap.add_argument("--variants", default="16")
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    n, d = int(a.n), a.d
    vs = [int(v) for v in a.variants.split(",")]
    dev = torch.device("cuda", 0)
    lib = _lib.kernels()
    X = K.generate_points(n, d, 0, 1000, seed=1, device=dev)
    torch.manual_seed(0)
    c = torch.rand(a.k, d, device=dev) * 1000
    op = K.prepare(c, X.shape[1])
    ks = K.swept_k(op)
    lab = torch.empty(n, dtype=torch.int32, device=dev)
    ref = None

    def sweep(v):
        _lib.check(lib.harp_kmeans_assign(X.data_ptr(), X.stride(0), op.Cm2.data_ptr(), n, X.shape[1], ks, d,
                                          lab.data_ptr(), None, 0, None, None, v, _lib.stream_ptr(dev)), "assign")

    same = {}
    for v in vs:  # warm-up, and the labels against the first variant's
        sweep(v)
        torch.cuda.synchronize()
        if ref is None:
            ref = lab.clone()
        same[v] = bool(torch.equal(lab, ref))
        print(f"variant {v}: labels equal to variant {vs[0]}: {same[v]}", flush=True)
    times = {v: [] for v in vs}
    for r in range(a.rounds):
        for v in vs:
            ts = []
            for _ in range(a.reps):
                e0 = torch.cuda.Event(enable_timing=True)
                e1 = torch.cuda.Event(enable_timing=True)
                e0.record()
                sweep(v)
                e1.record()
                e1.synchronize()
                ts.append(e0.elapsed_time(e1))
            times[v].append(ts)
            print(f"round {r} variant {v}: " + " ".join(f"{t:.2f}" for t in ts)
                  + f"  median {sorted(ts)[len(ts) // 2]:.2f} ms", flush=True)
    out = {"n": n, "k": a.k, "d": d, "labels_equal_to_first": {str(v): same[v] for v in vs},
           "round_medians_ms": {str(v): [round(sorted(t)[len(t) // 2], 3) for t in times[v]] for v in vs},
           "all_ms": {str(v): [[round(x, 3) for x in t] for t in times[v]] for v in vs}}
    print(json.dumps(out["round_medians_ms"]))
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
    return 0 if all(same.values()) else 1


if __name__ == "__main__":
    sys.exit(main())
