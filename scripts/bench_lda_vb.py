"""LDA-VB E-step: the native engine (``ops.lda_vb``, ``csrc/lda_vb.hip``) against the torch engine
(``models.lda_vb._estep`` plus its word-topic ``index_add_``) on one GPU, in one process.

A synthetic Zipf corpus (default D = 1e5 documents of about 100 distinct terms, V = 5e4), K in
{10, 100, 1000}, 29 fixed passes (``gamma_tol = 0``: both engines do the same work). Per engine
and K: the E-step time (device events, median of ``--reps`` after one warm-up call) and
``max_memory_allocated`` above the inputs. The torch engine needs about five [nnz, K] fp64
temporaries at once; where that exceeds ``--torch-mem-fraction`` of the device memory it is
not run and the row says so. Prints one JSON line per measurement and a markdown table.

    python scripts/bench_lda_vb.py [--docs 100000] [--vocab 50000] [--topics 10,100,1000]
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from harp_amd.models import lda_vb as V  # noqa: E402
from harp_amd.ops import lda_vb as E  # noqa: E402


def zipf_corpus(n_docs: int, vocab: int, draws: int, seed: int, dev):
    """(doc, word, cnt), doc-sorted: ``draws`` Zipf(1) word draws per document, merged into counts."""
    g = torch.Generator(device=dev).manual_seed(seed)
    p = 1.0 / torch.arange(1, vocab + 1, dtype=torch.float64, device=dev)
    w = torch.multinomial(p, n_docs * draws, replacement=True, generator=g)
    key = torch.arange(n_docs, device=dev).repeat_interleave(draws) * vocab + w
    key, cnt = torch.unique(key, return_counts=True)  # sorted: by document, then word
    return key // vocab, key % vocab, cnt.double()


def timed(fn, reps: int):
    fn()  # warm-up: code objects, allocator
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return sorted(ms)[len(ms) // 2]


def measure(fn, reps: int, dev):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats(dev)
    base = torch.cuda.memory_allocated(dev)
    ms = timed(fn, reps)
    return ms, torch.cuda.max_memory_allocated(dev) - base


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--docs", type=int, default=100000)
    ap.add_argument("--vocab", type=int, default=50000)
    ap.add_argument("--draws", type=int, default=135, help="word draws per document (about 100 distinct terms)")
    ap.add_argument("--topics", default="10,100,1000")
    ap.add_argument("--passes", type=int, default=29)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--torch-mem-fraction", type=float, default=0.5)
    ap.add_argument("--seed", type=int, default=0)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_lda_vb.py measures on a GPU: none found")
    dev = torch.device("cuda", 0)
    doc, word, cnt = zipf_corpus(a.docs, a.vocab, a.draws, a.seed, dev)
    nnz = doc.numel()
    plan = E.DocPlan.build(doc, word, a.docs)
    total = torch.cuda.get_device_properties(dev).total_memory
    print(json.dumps({"docs": a.docs, "vocab": a.vocab, "nnz": nnz, "terms_per_doc": nnz / a.docs,
                      "passes": a.passes, "long_docs": plan.n_long}), flush=True)
    rows = []
    for K in [int(k) for k in a.topics.split(",")]:
        g = torch.Generator().manual_seed(a.seed + K)
        beta = torch.rand((K, a.vocab), generator=g, dtype=torch.float64) + 1.0
        log_beta = (beta / beta.sum(1, keepdim=True)).log().to(dev)
        log_beta_t = log_beta.t().contiguous()
        alpha = torch.full((K,), 0.1, dtype=torch.float64, device=dev)
        cfg = V.LDAVBConfig(num_topics=K, gamma_iters=a.passes, gamma_tol=0.0)
        out = {}

        def native():
            out.pop("native", None)  # the peak counts one call's outputs, not the previous call's too
            out["native"] = E.estep(plan, cnt, log_beta_t, alpha, a.passes, 0.0)

        def torch_engine():
            out.pop("torch", None)
            gamma, phi, logz = V._estep(doc, word, cnt, a.docs, log_beta, alpha, cfg)
            S = torch.zeros((K, a.vocab), dtype=torch.float64, device=dev)
            S.index_add_(1, word, (cnt[:, None] * phi).t())
            out["torch"] = (gamma, S, logz)

        n_ms, n_mem = measure(native, a.reps, dev)
        row = {"K": K, "native_ms": n_ms, "native_peak_bytes": n_mem, "torch_ms": None, "torch_peak_bytes": None,
               "max_rel_gamma_diff": None}
        need = 5 * nnz * K * 8
        if need <= a.torch_mem_fraction * total:
            t_ms, t_mem = measure(torch_engine, a.reps, dev)
            gn, gt = out["native"][0], out["torch"][0]
            row.update(torch_ms=t_ms, torch_peak_bytes=t_mem,
                       max_rel_gamma_diff=float(((gn - gt).abs() / gt.abs()).max()))
        else:
            row["torch_skipped"] = f"needs about {need / 1e9:.0f} GB of [nnz, K] temporaries"
        out.clear()
        rows.append(row)
        print(json.dumps(row), flush=True)
    print("\n| K | native ms | native peak MB | torch ms | torch peak MB | torch / native | max rel gamma diff |")
    print("|---|---|---|---|---|---|---|")
    for r in rows:
        if r["torch_ms"] is None:
            print(f"| {r['K']} | {r['native_ms']:.1f} | {r['native_peak_bytes'] / 1e6:.0f} | not run: "
                  f"{r['torch_skipped']} | - | - | - |")
        else:
            print(f"| {r['K']} | {r['native_ms']:.1f} | {r['native_peak_bytes'] / 1e6:.0f} | {r['torch_ms']:.1f} | "
                  f"{r['torch_peak_bytes'] / 1e6:.0f} | {r['torch_ms'] / r['native_ms']:.2f} | "
                  f"{r['max_rel_gamma_diff']:.1e} |")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
