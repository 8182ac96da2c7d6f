"""CPU checks of the exact SYRK tests' own tools (tests/syrk_cases.py): the layout oracle
against the element formula and against X^T X, and the case tables against the launch rules,
so what tests/test_syrk_exact_gpu.py claims to reach can be checked without a GPU."""
import pytest
import torch

from tests import syrk_cases as SC


@pytest.mark.parametrize("n,d,ld,d_pad", [(1, 1, 48, 128), (47, 3, 48, 128), (49, 31, 96, 128), (100, 127, 192, 128),
                                          (193, 128, 384, 256), (60, 5, 144, 32)])
def test_feature_major_oracle(n, d, ld, d_pad):
    Xb = SC.int_rows(n, d, seed=n * 1000 + d)
    XT = SC.feature_major_ref(Xb, n, d, ld, d_pad)
    assert XT.shape == (ld // 48, d_pad, 48) and XT.dtype == torch.bfloat16 and XT.is_contiguous()
    # the element formula, one element at a time
    want = torch.zeros_like(XT)
    for k in range(n):
        for f in range(d):
            want[k // 48, f, k % 48] = Xb[k, f]
        want[k // 48, d, k % 48] = 1
    assert torch.equal(XT, want)
    # the Gram of the dense view: X^T X, the column sums and the count
    G = SC.gram_ref(XT).double()
    X = Xb.double()
    assert torch.equal(G[:d, :d], X.t() @ X)
    assert torch.equal(G[:d, d], X.sum(0))
    assert G[d, d].item() == n
    assert int(G[d + 1:].abs().sum()) == 0 and int(G[:, d + 1:].abs().sum()) == 0


def test_feature_major_oracle_ones_row_elsewhere():
    Xb = SC.int_rows(50, 7, seed=5)
    XT = SC.feature_major_ref(Xb, 50, 7, 96, 32, ones_row=20)
    D = SC.dense(XT)
    assert torch.equal(D[:7, :50], Xb.t()) and bool((D[20, :50] == 1).all())
    D[20, :50] = 0
    assert int(D[7:].float().abs().sum()) == 0 and int(D[:, 50:].float().abs().sum()) == 0


def test_tile_form_table_matches_launch_rules():
    for d_pad, d, tile, nt, _ in SC.TILE_FORMS:
        assert d < d_pad and d_pad % 128 == 0
        for ld in SC.TILE_LDS:
            assert SC.exact_ok(ld)
            p = SC.launch_plan(d_pad, ld, 0)
            assert (p["mt"], p["nt"]) == (tile, nt)
            assert sum(p["stages"]) == ld // 48
            assert p["branch"] == ("target_wg" if d_pad in (1664, 2304) else "per_xcd")
    # the forms named in the table
    assert SC.launch_plan(128, 192)["ntiles"] == 1 and SC.launch_plan(128, 192)["lone"] == 1
    assert SC.launch_plan(896, 192)["ntiles"] == 25
    assert SC.launch_plan(1664, 192)["ntiles"] == 85 and SC.launch_plan(2304, 192)["ntiles"] == 41
    assert SC.launch_plan(1024, 192)["ntiles"] == 8 and SC.launch_plan(768, 192)["lone"] == 1
    # ld = 192: one split of 4 stages everywhere; ld = 6192: two auto splits, the last one
    # short (65 + 64 stages), wherever the halving of the split count passes through 2
    assert all(SC.launch_plan(t[0], 192)["stages"] == [4] for t in SC.TILE_FORMS)
    two = [t[0] for t in SC.TILE_FORMS if SC.launch_plan(t[0], 6192)["stages"] == [65, 64]]
    one = [t[0] for t in SC.TILE_FORMS if SC.launch_plan(t[0], 6192)["stages"] == [129]]
    assert len(two) + len(one) == len(SC.TILE_FORMS)
    assert {128, 256, 512, 1024} <= set(two), (two, one)
    assert set(one) == {t[0] for t in SC.TILE_EXTRA}
    for d_pad, d, ld, stages in SC.TILE_EXTRA:
        assert SC.exact_ok(ld) and d < d_pad and SC.launch_plan(d_pad, ld)["stages"] == stages


def test_ring_remap_lockstep_tables_match_launch_rules():
    for ld, ns, stages in SC.RING_EDGES:
        for d_pad in SC.RING_PANELS:
            assert SC.launch_plan(d_pad, ld, ns)["stages"] == stages
    for d_pad, ld, ns, wg in SC.REMAP:
        p = SC.launch_plan(d_pad, ld, ns)
        assert p["workgroups"] == wg and wg > 8 and p["splits"] > 1
    assert sum(wg % 8 != 0 for *_, wg in SC.REMAP) >= 3 and sum(wg % 8 == 0 for *_, wg in SC.REMAP) >= 1
    for d_pad, ld, ns, stages in SC.LOCKSTEP:
        p = SC.launch_plan(d_pad, ld, ns)
        assert p["mt"] == 256 and p["stages"] == stages and p["workgroups"] <= 256
