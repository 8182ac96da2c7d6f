"""Association rules by Apriori (DAAL ``association_rules``, batch).

Reference: ml/daal/.../daal_association (DAAL association_rules Batch with
``minSupport`` / ``minConfidence``; input = (transaction id, item id) pairs; results =
large item sets with their supports and rules ``X => Y`` with confidences).

Two engines, identical results:

* ``engine="torch"`` (the default of :func:`apriori`): transactions become a dense 0/1
  incidence matrix T [n_trans, n_items] (bf16 on the GPU: exact for 0/1 products, counts
  accumulate in fp32). Level-2 supports for every pair at once are ONE GEMM T^T T on the
  matrix cores; level k > 2 candidates (joined + pruned on the host, Apriori property) are
  counted in chunks as the row-sum of the product of their gathered columns.
* ``engine="native"`` (the default of :func:`apriori_transactions`): transactions become
  vertical bitmaps (``ops.apriori``: one row of bits per item), never a dense matrix. Level 1
  is a popcount per row, level 2 a bit "GEMM" over the frequent items, level k the AND /
  popcount of candidate runs that share their first k-1 items; join and prune are vectorised,
  so the level loop holds no Python loop over itemsets.

A distributed run partitions transactions and allreduces each level's support vector (one
collective per level; fp64 sums in the torch engine, int64 in the native one).
"""
from __future__ import annotations

import itertools
from typing import Dict, List, Optional, Sequence, Tuple

import torch

from ..ops import apriori as AO
from ..parallel.comm import Communicator
from .common import reduce_partials


def incidence(tids: torch.Tensor, items: torch.Tensor, n_items: int, device=None) -> torch.Tensor:
    """(transaction, item) pairs -> dense 0/1 matrix (transactions renumbered densely)."""
    dev = device or tids.device
    ut, t = torch.unique(tids, return_inverse=True)
    T = torch.zeros((ut.numel(), n_items), dtype=torch.float32, device=dev)
    T[t.to(dev), items.to(dev)] = 1.0
    return T


def _allsum(comm, v: torch.Tensor) -> torch.Tensor:
    if comm is None or comm.world_size == 1:
        return v.double()
    return reduce_partials(comm, {"v": v})["v"]


def _allsum_int(comm, v: torch.Tensor) -> torch.Tensor:
    """int32 device counts -> their int64 sum over the workers (exact), on ``v``'s device."""
    if comm is None or comm.world_size == 1:
        return v.long()
    return reduce_partials(comm, {"v": v}, dtype=torch.int64)["v"].to(v.device)


def _mine_torch(T, n, need, comm, max_len, chunk) -> Dict[Tuple[int, ...], float]:
    dev = T.device
    mm_dtype = torch.bfloat16 if dev.type == "cuda" else torch.float32
    s1 = _allsum(comm, T.sum(0).double().cpu())
    large: Dict[Tuple[int, ...], float] = {}
    L1 = [i for i in range(T.shape[1]) if s1[i] >= need]
    for i in L1:
        large[(i,)] = float(s1[i])
    prev = [(i,) for i in L1]
    k = 2
    while prev and (max_len is None or k <= max_len):
        if k == 2:
            idx = torch.tensor(L1, device=dev)
            Tc = T[:, idx].to(mm_dtype)
            S = (Tc.t() @ Tc).float() if dev.type == "cuda" else Tc.t() @ Tc
            iu = torch.triu_indices(len(L1), len(L1), 1)
            sup = _allsum(comm, S[iu[0], iu[1]].double().cpu())
            cands = [(L1[a], L1[b]) for a, b in zip(iu[0].tolist(), iu[1].tolist())]
        else:
            prev_set = set(prev)
            cands = []
            for a, b in itertools.combinations(prev, 2):
                if a[:-1] == b[:-1]:
                    c = a + (b[-1],) if a[-1] < b[-1] else b + (a[-1],)
                    if all(sub in prev_set for sub in itertools.combinations(c, k - 1)):
                        cands.append(c)
            cands = sorted(set(cands))
            if not cands:
                break
            C = torch.tensor(cands, device=dev)
            parts = []
            for a in range(0, len(cands), chunk):
                G = T[:, C[a:a + chunk]]  # [n, c, k]
                parts.append(G.prod(2).sum(0).double())
            sup = _allsum(comm, torch.cat(parts).cpu())
        prev = []
        for c, s in zip(cands, sup.tolist()):
            if s >= need:
                large[tuple(c)] = s
                prev.append(tuple(c))
        prev.sort()
        k += 1
    return large


def _mine_native(B: AO.Bitmaps, need, comm, max_len) -> Dict[Tuple[int, ...], float]:
    """Level loop on bitmaps. Every level is tensor code: pair / run counting on the device,
    join and prune vectorised; the itemsets reach Python once, after the last level."""
    dev = B.device
    c1 = _allsum_int(comm, AO.item_counts(B))
    keep = c1.double() >= need
    prev = torch.nonzero(keep).to(torch.int32)  # [m, 1], sorted
    levels = [(prev, c1[keep])]
    k = 2
    while prev.shape[0] and (max_len is None or k <= max_len):
        if k == 2:
            m = prev.shape[0]
            S = AO.pair_counts(B, prev[:, 0])
            iu = torch.triu_indices(m, m, 1, device=dev)
            cand = torch.stack([prev[iu[0], 0], prev[iu[1], 0]], 1)
            cnt = S[iu[0], iu[1]]
        else:
            cand = AO.join(prev)
            if cand.shape[0]:
                cand = cand[AO.prune(cand, prev)]
            cnt = AO.count(B, cand) if cand.shape[0] else None
        if cand.shape[0] == 0:
            break
        cnt = _allsum_int(comm, cnt)
        keep = cnt.double() >= need
        prev = cand[keep]
        levels.append((prev, cnt[keep]))
        k += 1
    large: Dict[Tuple[int, ...], float] = {}
    for sets, cnt in levels:
        for c, s in zip(sets.tolist(), cnt.tolist()):
            large[tuple(c)] = float(s)
    return large


def _rules(sets: Dict[Tuple[int, ...], float], min_confidence: float) -> List[tuple]:
    rules = []
    for c, s in sets.items():
        if len(c) < 2:
            continue
        for r in range(1, len(c)):
            for ante in itertools.combinations(c, r):
                cons = tuple(x for x in c if x not in ante)
                conf = s / sets[ante]
                if conf >= min_confidence:
                    rules.append((ante, cons, conf, s))
    return rules


def _pairs_table(itemsets: Sequence[Tuple[int, ...]]) -> torch.Tensor:
    """DAAL's itemset layout: one (set index, item) row per member."""
    rows = [(i, x) for i, c in enumerate(itemsets) for x in c]
    return torch.tensor(rows, dtype=torch.int64).reshape(-1, 2)


def _result(large: Dict[Tuple[int, ...], float], n: float, min_confidence: float) -> Dict[str, object]:
    order = sorted(large.items(), key=lambda kv: (len(kv[0]), kv[0]))
    sets = {c: s / n for c, s in order}
    counts = {c: int(round(s)) for c, s in order}
    rules = _rules(sets, min_confidence)
    return {"large_itemsets": sets, "rules": rules, "n_transactions": int(n), "counts": counts,
            # the DAAL result tables
            "largeItemsets": _pairs_table(list(counts)),
            "largeItemsetsSupport": torch.tensor([(i, s) for i, s in enumerate(counts.values())],
                                                 dtype=torch.int64).reshape(-1, 2),
            "antecedentItemsets": _pairs_table([r[0] for r in rules]),
            "consequentItemsets": _pairs_table([r[1] for r in rules]),
            "confidence": torch.tensor([r[2] for r in rules], dtype=torch.float64)}


def _check_engine(engine: str) -> None:
    if engine not in ("torch", "native"):
        raise ValueError(f"engine={engine!r}: expected 'torch' or 'native'")


def _total(comm, n_local: int) -> float:
    assert n_local < 2 ** 31, "a rank holds fewer than 2^31 transactions"
    return float(_allsum(comm, torch.tensor([float(n_local)]))[0])


def apriori(T: torch.Tensor, min_support: float = 0.01, min_confidence: float = 0.6,
            comm: Optional[Communicator] = None, max_len: Optional[int] = None,
            chunk: int = 1 << 14, engine: str = "torch") -> Dict[str, object]:
    """Returns large item sets {tuple(items): support fraction} and rules
    [(antecedent, consequent, confidence, support)] sorted like DAAL (by itemset size,
    then lexicographically), ``counts`` {tuple(items): integer support} and the DAAL result
    tables as tensors: ``largeItemsets`` / ``antecedentItemsets`` / ``consequentItemsets``
    ((set index, item) rows), ``largeItemsetsSupport`` ((index, count) rows) and
    ``confidence`` (one value per rule). ``engine="native"`` packs ``T != 0`` into bitmaps
    and counts on them; both engines return the same result."""
    _check_engine(engine)
    n = _total(comm, T.shape[0])
    need = min_support * n
    if engine == "native":
        large = _mine_native(AO.pack_dense(T), need, comm, max_len)
    else:
        large = _mine_torch(T, n, need, comm, max_len, chunk)
    return _result(large, n, min_confidence)


def apriori_transactions(tids: torch.Tensor, items: torch.Tensor, n_items: int, min_support: float = 0.01,
                         min_confidence: float = 0.6, comm: Optional[Communicator] = None,
                         max_len: Optional[int] = None, engine: str = "native", device=None) -> Dict[str, object]:
    """:func:`apriori` on (transaction id, item id) pairs, this worker's own transactions
    (tids are renumbered densely per worker, as :func:`incidence` does; a duplicated pair is
    harmless). With the native engine the pairs go straight to bitmaps on ``device`` (default:
    the pairs' device) and no dense matrix is formed."""
    _check_engine(engine)
    if engine == "torch":
        return apriori(incidence(tids, items, n_items, device), min_support, min_confidence, comm, max_len)
    dev = device or tids.device
    ut, t = torch.unique(tids.to(dev), return_inverse=True)
    n_local = ut.numel()
    n = _total(comm, n_local)
    B = AO.pack(t, items.to(dev), n_local, n_items)
    del ut, t
    return _result(_mine_native(B, min_support * n, comm, max_len), n, min_confidence)
