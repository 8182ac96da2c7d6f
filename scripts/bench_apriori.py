#!/usr/bin/env python3
"""Apriori engines on one GPU (models/apriori.py, csrc/apriori.hip).

``--case small``: the native engine against the torch engine (the dense incidence matrix, a
GEMM for level 2, gathered columns above; its code is the one that ran before the native
engine existed) at a shape the torch engine can hold: n = 2e5 transactions, 200 items, each
item in 5 % of the transactions plus a planted 6-item pattern in 15 %, minSupport 0.03, so
the run reaches level 6 and both engines must return the same sets.

``--case large``: the native engine alone at n = 1e6, 1e4 items, 10 pairs per transaction
with a few popular items: pack, level 1, the pair kernel over ALL 1e4 items (the level-2 worst
case) and a whole run at a minSupport that keeps ``--frequent`` items.

Protocol: wall time around ``torch.cuda.synchronize()`` (the engines end in host code),
``--warmup`` warm-ups, median of ``--runs``; peak memory is the rise of
``torch.cuda.max_memory_allocated`` across the timed calls. One JSON line per case.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    import torch

    from harp_amd.models import apriori as AP
    from harp_amd.ops import apriori as AO

    ap = argparse.ArgumentParser()
    ap.add_argument("--case", choices=("small", "large", "both"), default="both")
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--frequent", type=int, default=1000)
    ap.add_argument("--scale", type=float, default=1.0, help="shrink n (dry runs)")
    ap.add_argument("--device", default="cuda", help="cpu = dry run of the script on the torch mirrors")
    args = ap.parse_args()
    dev = torch.device(args.device, 0) if args.device == "cuda" else torch.device(args.device)
    gpu = dev.type == "cuda"
    assert not gpu or torch.cuda.is_available(), "bench_apriori needs a GPU"
    sync = torch.cuda.synchronize if gpu else (lambda: None)
    name = torch.cuda.get_device_name(0) if gpu else "cpu"

    def timed(fn, runs=None):
        """(median ms, min ms, max ms, peak MiB, last result)"""
        runs = runs or args.runs
        out = None
        for _ in range(args.warmup):
            out = fn()
        sync()
        if gpu:
            torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.memory_allocated() if gpu else 0
        ts = []
        for _ in range(runs):
            sync()
            t0 = time.perf_counter()
            out = fn()
            sync()
            ts.append(1e3 * (time.perf_counter() - t0))
        peak = (torch.cuda.max_memory_allocated() - before) / 2 ** 20 if gpu else 0.0
        return round(statistics.median(ts), 3), round(min(ts), 3), round(max(ts), 3), round(peak, 1), out

    def row(t):
        return {"median_ms": t[0], "min_ms": t[1], "max_ms": t[2], "peak_MiB": t[3]}

    if args.case in ("small", "both"):
        n, items, sup, conf = int(200_000 * args.scale), 200, 0.03, 0.7
        g = torch.Generator(device=dev).manual_seed(0)
        keep = torch.rand(n, items, device=dev, generator=g) < 0.05
        keep[torch.rand(n, device=dev, generator=g) < 0.15, :6] = True
        tids, its = keep.nonzero(as_tuple=True)
        del keep
        nat = timed(lambda: AP.apriori_transactions(tids, its, items, sup, conf))
        tor = timed(lambda: AP.apriori_transactions(tids, its, items, sup, conf, engine="torch"))
        T = AP.incidence(tids, its, items)
        B = AO.pack(tids, its, n, items)
        need = sup * n
        nat_mine = timed(lambda: AP._mine_native(B, need, None, None))
        tor_mine = timed(lambda: AP._mine_torch(T, float(n), need, None, None, 1 << 14))
        # exact oracle: the torch engine on CPU tensors (fp32 GEMM, counts < 2^24). On the GPU its level-2
        # GEMM returns bf16, which rounds supports above 256, so its counts are compared, not asserted
        cpu = AP.apriori_transactions(tids.cpu(), its.cpu(), items, sup, conf, engine="torch")
        assert nat[4]["counts"] == cpu["counts"] and nat[4]["rules"] == cpu["rules"]
        a, b = nat[4]["counts"], tor[4]["counts"]
        diff = [abs(a[c] - b[c]) for c in a if c in b and a[c] != b[c]]
        print(json.dumps({"case": "small", "n": n, "items": items, "pairs": tids.numel(), "min_support": sup,
                          "native_equals_cpu_torch_engine": True,
                          "gpu_torch_engine": {"same_sets": set(a) == set(b), "counts_that_differ": len(diff),
                                               "max_count_difference": max(diff, default=0)},
                          "levels": max(len(c) for c in nat[4]["counts"]), "itemsets": len(nat[4]["counts"]),
                          "rules": len(nat[4]["rules"]), "bitmap_MiB": round(B.nbytes / 2 ** 20, 1),
                          "native_pairs_to_result": row(nat), "torch_pairs_to_result": row(tor),
                          "native_levels_only": row(nat_mine), "torch_levels_only": row(tor_mine),
                          "device": name}), flush=True)
        del T, B, tids, its

    if args.case in ("large", "both"):
        n, items, per = int(1_000_000 * args.scale), 10_000, 10
        g = torch.Generator(device=dev).manual_seed(1)
        tids = torch.arange(n, device=dev).repeat_interleave(per)
        its = (items * torch.rand(per * n, device=dev, generator=g) ** 3).long().clamp_(max=items - 1)
        its.view(n, per)[torch.rand(n, device=dev, generator=g) < 0.05, :4] = torch.arange(4, device=dev)  # a pattern
        pk = timed(lambda: AO.pack(tids, its, n, items))
        B = pk[4]
        l1 = timed(lambda: AO.item_counts(B))
        cnt = l1[4].long()
        allidx = torch.arange(items, device=dev)
        pr = timed(lambda: AO.pair_counts(B, allidx))
        assert torch.equal(torch.diagonal(pr[4]).long(), cnt)
        pr = row(pr)  # drops the [items, items] result
        thr = int(torch.sort(cnt, descending=True).values[args.frequent]) + 1
        sup = (thr - 0.5) / n
        run = timed(lambda: AP.apriori_transactions(tids, its, items, sup, 0.5))
        out = run[4]
        print(json.dumps({"case": "large", "n": n, "items": items, "pairs": tids.numel(),
                          "bitmap_MiB": round(B.nbytes / 2 ** 20, 1), "pack": row(pk), "item_counts": row(l1),
                          "pair_counts_all_items": pr,
                          "pair_slab_words": AO.pair_slab_words(items, B.W),
                          "run": dict(row(run), min_support=sup, frequent_items=int((cnt >= thr).sum()),
                                      levels=max(len(c) for c in out["counts"]), itemsets=len(out["counts"]),
                                      rules=len(out["rules"])),
                          "device": name}), flush=True)


if __name__ == "__main__":
    main()
