"""Native Apriori engine on CPU tensors (the torch mirrors of ops/apriori.py): against the
torch engine, a brute-force enumeration, the golden fixture, two gloo workers and the CLI.
Every comparison is exact integer equality."""
import json

import numpy as np
import torch

from harp_amd import cli
from harp_amd.models import apriori as AP
from harp_amd.ops import apriori as AO
from harp_amd.runtime.launcher import launch
from tests import apriori_cases as AC


def _same(a, b):
    assert a["counts"] == b["counts"] and list(a["counts"]) == list(b["counts"])
    assert a["large_itemsets"] == b["large_itemsets"]
    assert a["rules"] == b["rules"]
    assert a["n_transactions"] == b["n_transactions"]
    for k in ("largeItemsets", "largeItemsetsSupport", "antecedentItemsets", "consequentItemsets", "confidence"):
        assert torch.equal(a[k], b[k])


def test_native_matches_torch_engine_and_brute_force():
    tids, its = AC.transactions()
    T = AP.incidence(tids, its, 12)
    ref = AP.apriori(T, 0.1, 0.6)
    large, rules = AC.brute(T, 0.1, 0.6)
    for out in (AP.apriori(T, 0.1, 0.6, engine="native"), AP.apriori_transactions(tids, its, 12, 0.1, 0.6)):
        _same(out, ref)
        assert out["counts"] == large
        assert {(a, b) for a, b, _, _ in out["rules"]} == rules
        assert (1, 3, 5) in out["counts"]
    assert max(len(c) for c in large) >= 3  # the level-k path ran
    assert AP.apriori_transactions(tids, its, 12, 0.1, 0.6, engine="torch")["counts"] == large


def test_result_tables_layout():
    tids, its = AC.transactions()
    out = AP.apriori_transactions(tids, its, 12, 0.1, 0.6)
    assert AC.decode_sets(out["largeItemsets"]) == list(out["counts"])
    assert out["largeItemsetsSupport"].tolist() == [[i, s] for i, s in enumerate(out["counts"].values())]
    assert AC.decode_sets(out["antecedentItemsets"]) == [r[0] for r in out["rules"]]
    assert AC.decode_sets(out["consequentItemsets"]) == [r[1] for r in out["rules"]]
    assert out["confidence"].tolist() == [r[2] for r in out["rules"]]


def test_duplicated_pairs():
    tids, its = AC.transactions()
    tids = tids * 7 + 3  # sparse ids: renumbered densely
    dup = torch.cat([torch.arange(tids.numel()), torch.arange(0, tids.numel(), 3), torch.arange(5)])
    dup = dup[torch.randperm(dup.numel(), generator=torch.Generator().manual_seed(1))]
    a = AP.apriori_transactions(tids[dup], its[dup], 12, 0.1, 0.6)
    _same(a, AP.apriori_transactions(tids, its, 12, 0.1, 0.6))
    assert a["n_transactions"] == torch.unique(tids).numel()


def test_bitmaps_layout():
    tids, its = torch.tensor([0, 64, 64, 129, 5]), torch.tensor([0, 0, 0, 2, 2])
    B = AO.pack(tids, its, 130, 3)
    assert B.words.shape == (3, 4) and B.W == 8 and B.nbytes % 16 == 0  # 130 bits -> 256 (16-byte multiple)
    assert B.words[0].tolist() == [1, 1, 0, 0] and B.words[2].tolist() == [32, 0, 2, 0]
    assert AO.item_counts(B).tolist() == [2, 0, 2]
    B63 = AO.pack(torch.tensor([63]), torch.tensor([0]), 64, 1)
    assert AO.item_counts(B63).tolist() == [1] and AO.pair_counts(B63, torch.tensor([0])).tolist() == [[1]]


def test_golden_fixture_full_depth():
    tids, its, exp = AC.fixture()
    out = AP.apriori_transactions(tids, its, exp["n_items"], exp["min_support"], exp["min_confidence"])
    AC.assert_matches_expected(out, exp)


def _job(comm, tids, its):
    m = (tids % comm.world_size) == comm.rank
    return AP.apriori_transactions(tids[m], its[m], 12, 0.1, 0.6, comm=comm)


def test_distributed_two_workers():
    tids, its = AC.transactions()
    single = AP.apriori_transactions(tids, its, 12, 0.1, 0.6)
    for r in launch(_job, 2, args=(tids, its), timeout=300):
        _same(r, single)


def test_join_and_prune_against_itertools():
    prev = torch.tensor(AC.LEVEL3)
    cand = AO.join(prev)
    assert [tuple(c) for c in cand.tolist()] == AC.join_itertools(AC.LEVEL3)
    for name, cands, level in AC.prune_cases():
        got = AO.prune(torch.tensor(cands), torch.tensor(level)).tolist()
        assert got == AC.prune_itertools(cands, level, all_subsets=False), name
        if name != "sorts_first":  # the joined rows are in the level: same as checking every subset
            assert got == AC.prune_itertools(cands, level), name
    assert AO.prune(torch.tensor(AC.join_itertools(AC.LEVEL3)), prev).tolist() == [True, True, False, False, True]
    # level 2 from single items: one group, every ordered pair, nothing to check
    ones = torch.tensor([[2], [5], [7]])
    pairs = AO.join(ones)
    assert pairs.tolist() == [[2, 5], [2, 7], [5, 7]] and AO.prune(pairs, ones).all()
    # k = 3: one position to check
    p2 = [(1, 2), (1, 3), (1, 4), (2, 3), (3, 4)]
    c3 = AO.join(torch.tensor(p2))
    assert [tuple(c) for c in c3.tolist()] == AC.join_itertools(p2) == [(1, 2, 3), (1, 2, 4), (1, 3, 4)]
    want = AC.prune_itertools(AC.join_itertools(p2), p2)
    assert AO.prune(c3, torch.tensor(p2)).tolist() == want == [True, False, True]
    assert AO.join(torch.zeros((0, 2), dtype=torch.long)).shape == (0, 3)
    assert AO.join(torch.tensor([[1, 2]])).shape == (0, 3)


def test_groups_split_long_runs():
    cand = torch.tensor([[0, 1, x] for x in range(2, 9)] + [[0, 2, 3]] + [[1, 2, x] for x in range(3, 6)])
    assert AO.groups(cand, cap=3).tolist() == [0, 3, 6, 7, 8, 11]
    assert AO.groups(cand).tolist() == [0, 7, 8, 11]
    assert AO.groups(cand[:1]).tolist() == [0, 1]


def test_cli_daal_ar_round_trip(tmp_path, capsys):
    tids, its, exp = AC.fixture()
    inp = tmp_path / "in"
    inp.mkdir()
    half = tids < 500  # two files with disjoint tids: one per worker
    for name, m in (("ar_1.csv", half), ("ar_2.csv", ~half)):
        np.savetxt(inp / name, torch.stack([tids[m], its[m]], 1).numpy(), fmt="%d", delimiter=",")
    work = tmp_path / "out"
    assert cli.main(["daal", "ar", "2", "1", "0", "1", str(inp), str(work), "--min-support", "0.005",
                     "--backend", "gloo"]) == 0
    res = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert res["app"] == "daal" and res["result"]["n_transactions"] == 1000
    load = lambda k: torch.from_numpy(np.loadtxt(work / f"ar_{k}.csv", delimiter=",", ndmin=2))  # noqa: E731
    sets = AC.decode_sets(load("largeItemsets"))
    sup = load("largeItemsetsSupport").long().tolist()
    assert [[list(c), s] for c, (_, s) in zip(sets, sup)] == exp["itemsets"]
    rules = list(zip(AC.decode_sets(load("antecedentItemsets")), AC.decode_sets(load("consequentItemsets"))))
    assert rules == [(tuple(a), tuple(b)) for a, b in exp["rules"]]
    conf = load("confidence").reshape(-1)
    assert conf.numel() == AC.EXPECTED_RULES and bool((conf >= 0.7).all())
