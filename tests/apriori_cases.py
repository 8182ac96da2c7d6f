"""Inputs and oracles shared by test_apriori_native.py (CPU) and test_apriori_gpu.py."""
import itertools
import json
import os
import random

import torch

FIXTURE_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "datasets", "daal_ar", "batchdense",
                           "train")
FIXTURE = os.path.join(FIXTURE_DIR, "apriori_1000.csv")
EXPECTED = os.path.join(FIXTURE_DIR, "apriori_1000_expected.json")
EXPECTED_SIZES = {1: 29, 2: 406, 3: 2718, 4: 183, 5: 2}  # produced by the torch engine before the native one existed
EXPECTED_RULES = 96


def transactions(n=300, items=12, seed=0):
    """The generator of tests/test_apriori.py."""
    r = random.Random(seed)
    tids, its = [], []
    for t in range(n):
        basket = {i for i in range(items) if r.random() < 0.15}
        if r.random() < 0.4:
            basket |= {1, 3, 5}
        if r.random() < 0.3:
            basket |= {2, 7}
        for i in sorted(basket):
            tids.append(t)
            its.append(i)
    return torch.tensor(tids), torch.tensor(its)


def brute(T, min_sup, min_conf):
    n = T.shape[0]
    rows = [set(torch.nonzero(T[i]).reshape(-1).tolist()) for i in range(n)]
    large = {}
    for k in range(1, T.shape[1] + 1):
        found = False
        for c in itertools.combinations(range(T.shape[1]), k):
            s = sum(1 for r in rows if set(c) <= r)
            if s / n >= min_sup:
                large[c] = s
                found = True
        if not found:
            break
    rules = set()
    for c, s in large.items():
        for r in range(1, len(c)):
            for a in itertools.combinations(c, r):
                if s / large[a] >= min_conf:
                    rules.add((a, tuple(x for x in c if x not in a)))
    return large, rules


_fixture = None


def fixture():
    """(tids, items, expected) of the golden fixture, loaded once."""
    global _fixture
    if _fixture is None:
        with open(FIXTURE) as f:
            rows = [tuple(int(x) for x in line.split(",")) for line in f if line.strip()]
        with open(EXPECTED) as f:
            exp = json.load(f)
        _fixture = (torch.tensor([r[0] for r in rows]), torch.tensor([r[1] for r in rows]), exp)
    return _fixture


def assert_matches_expected(out, exp):
    want = {tuple(c): s for c, s in exp["itemsets"]}
    sizes = {}
    for c in want:
        sizes[len(c)] = sizes.get(len(c), 0) + 1
    assert sizes == EXPECTED_SIZES and len(exp["rules"]) == EXPECTED_RULES
    assert out["n_transactions"] == exp["n_transactions"]
    assert out["counts"] == want
    assert list(out["counts"]) == list(want)  # DAAL order: by size, then lexicographic
    assert [(a, b) for a, b, _, _ in out["rules"]] == [(tuple(a), tuple(b)) for a, b in exp["rules"]]


def decode_sets(pairs):
    """(set index, item) rows -> list of item tuples."""
    sets = {}
    for i, x in pairs.reshape(-1, 2).long().tolist():
        sets.setdefault(i, []).append(x)
    return [tuple(sets[i]) for i in sorted(sets)]


# ------------------------------------------------------------------ join / prune
# sorted 3-itemsets; the join gives (1,2,3,4) (1,2,3,5) (1,2,4,5) (1,3,4,5) (2,3,4,5)
LEVEL3 = [(1, 2, 3), (1, 2, 4), (1, 2, 5), (1, 3, 4), (1, 3, 5), (2, 3, 4), (2, 3, 5), (2, 4, 5), (3, 4, 5)]


def join_itertools(prev):
    out = []
    for a, b in itertools.combinations(prev, 2):
        if a[:-1] == b[:-1]:
            out.append(a + (b[-1],) if a[-1] < b[-1] else b + (a[-1],))
    return sorted(set(out))


def prune_itertools(cands, prev, all_subsets=True):
    """Keep flags: every (k-1)-subset in prev (``all_subsets``), or only those that drop one of
    the first k-2 positions (what prune checks: the other two are the joined rows)."""
    ps = set(prev)
    k = len(cands[0]) if cands else 0
    drops = range(k) if all_subsets else range(k - 2)
    return [all(c[:d] + c[d + 1:] in ps for d in drops) for c in cands]


def prune_cases():
    """(name, candidates, sorted previous level). In LEVEL3, (1,2,4,5) and (1,3,4,5) miss
    (1,4,5), absent from the middle of the level; without (3,4,5), the subset that (2,3,4,5)
    misses sorts after every row; in the last case the subsets (3,4,6) and (2,4,6) sort before
    every row (the level does not hold the candidates' joined rows, which prune never reads)."""
    cands = join_itertools(LEVEL3)
    return [("absent", cands, LEVEL3),
            ("sorts_last", cands, LEVEL3[:-1]),
            ("sorts_first", [(2, 3, 4, 6), (3, 4, 7, 8)], [(3, 4, 7), (3, 4, 8), (3, 7, 8), (4, 7, 8)])]
