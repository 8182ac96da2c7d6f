"""Native decision-forest kernels (``csrc/forest.hip``) against their torch mirror in
``harp_amd/ops/forest.py`` (run on CPU tensors), the forest invariants of
``tests/test_forest.py`` on GPU-trained forests, determinism and the prediction kernel.

Chosen split indices are never compared across implementations (exact ties are common); gains
are, and the tie rule is tested on a constructed histogram."""
import pytest
import torch

from harp_amd.models import trees as T
from harp_amd.ops import forest as F

from tests.test_forest import SHAPES, _cls, check_forest, fit_and_check, make_cls, tie_histogram

pytestmark = pytest.mark.gpu

# the shapes of test_forest.py, plus row counts just past a multiple of the wave / block / chunk
KSHAPES = SHAPES + [(257, 3, 8, 2), (4097, 4, 32, 3)]
LEVELS = (0, 3, 8)
_traces = {}


def _trace(shape, kind):
    """CPU mirror run (3 trees, depth 9, sqrt features) with the state of levels 0, 3 and 8."""
    key = (shape, kind)
    if key not in _traces:
        n, d, B, C = shape
        X, y, th = _cls(*shape)
        Xb = F.bin_features(X, th)
        mult = F.bootstrap(1, 0, 3, 0, n, "cpu")  # holds rows of multiplicity 0
        assert int((mult == 0).sum()) > 0
        g = torch.Generator().manual_seed(4)
        stats = torch.nn.functional.one_hot(y, C).double() * (torch.rand(n, generator=g, dtype=torch.float64) + 0.5)[:, None]
        keep = {}
        F.grow(Xb, d, B, C, kind, mult, task=F.GINI, max_depth=9, k_sub=T._n_sub("sqrt", d), seed=1, y=y,
               stats=stats, trace=lambda lvl, s: keep.__setitem__(lvl, s) if lvl in LEVELS else None)
        assert 0 in keep
        _traces[key] = (Xb, mult, y, stats, keep)
    return _traces[key]


def _ids(s):
    return "x".join(map(str, s))


@pytest.mark.parametrize("shape", KSHAPES, ids=_ids)
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_bin_kernel(cuda, shape, dtype):
    n, d, B, C = shape
    X, _, _ = _cls(*shape)
    X = X.to(dtype).clone()
    th = T._bins(X, B)
    for f in range(d):  # rows that sit exactly on thresholds
        X[f:n:7, f] = th[f, torch.arange(f, n, 7) % (B - 1)].to(dtype)
    th = T._bins(X, B)
    X[0, :] = th[:, 0].to(dtype)
    if dtype == torch.float32:
        th = th.float().double()  # thresholds a fp32 value can equal
        X[1, :] = th[:, -1].float()
    want = F.bin_features(X, th)
    got = F.bin_features(X.to(cuda), th.to(cuda))
    assert got.dtype == torch.uint8 and got.shape == (n, F.padded_width(d))
    assert torch.equal(got.cpu(), want)
    assert bool((want[:, :d].long() > 0).any()) and int(want.max()) <= B - 1


def test_bootstrap_and_subset_kernels(cuda):
    for seed, tree0, nt, row0, n in ((9, 0, 10, 0, 10000), (9, 4, 3, 123457, 4097), (2 ** 31 + 5, 7, 1, 2 ** 28, 63)):
        assert torch.equal(F.bootstrap(seed, tree0, nt, row0, n, cuda).cpu(), F.bootstrap(seed, tree0, nt, row0, n, "cpu"))
    g = torch.Generator().manual_seed(0)
    for d, k in ((1, 1), (7, 2), (33, 5), (100, 10), (5, 5)):
        tr = torch.randint(0, 50, (300,), generator=g).sort().values.int()
        nd = torch.randint(0, 5000, (300,), generator=g).int()
        want = F.feature_subset(11, tr, nd, d, k)
        assert bool((want.sum(1) == k).all())
        assert torch.equal(F.feature_subset(11, tr.to(cuda), nd.to(cuda), d, k).cpu(), want)


@pytest.mark.parametrize("shape", KSHAPES, ids=_ids)
def test_hist_and_route_kernels_count(cuda, shape):
    n, d, B, C = shape
    Xb, mult, y, _, keep = _trace(shape, F.COUNT)
    Xg, mg, yg = Xb.to(cuda), mult.to(cuda), y.int().to(cuda)
    for lvl, s in keep.items():
        order, cnt, frt = s["order"].to(cuda), s["cnt"].to(cuda), s["fr_tree"].to(cuda)
        H = F.level_hist(Xg, order, cnt, frt, mg, d, B, C, F.COUNT, y=yg)
        assert torch.equal(F.counts_as_int64(H).cpu(), s["H"]), lvl
        sp, bf, bb = s["split"].to(cuda), s["feature"].to(cuda), s["bin"].to(cuda)
        nleft = F.route_count(Xg, order, cnt, sp, bf, bb)
        assert torch.equal(nleft.cpu(), s["nleft"]), lvl
        new = F.route_scatter(Xg, order, cnt, sp, bf, bb, nleft, s["child_start"].to(cuda)).cpu()
        a = 0
        for c in s["new_cnt"].tolist():  # the order inside a child is free
            assert torch.equal(new[a:a + c].sort().values, s["new_order"][a:a + c].sort().values), lvl
            a += c


def test_hist_kernel_chunk_boundaries(cuda):
    """All rows live (multiplicity >= 1): 4097 rows are two full chunks and one row."""
    n, d, B, C = 4097, 4, 32, 3
    X, y, th = _cls(n, d, B, C)
    Xb = F.bin_features(X, th)
    mult = (torch.arange(n) % 3 + 1).to(torch.uint8)[None, :]
    order = torch.randperm(n, generator=torch.Generator().manual_seed(0)).int()
    for cnt in ([n], [2048, 2049], [1, 4096], [2047, 1, 2049]):
        cnt = torch.tensor(cnt, dtype=torch.int32)
        frt = torch.zeros(cnt.numel(), dtype=torch.int32)
        want = F.level_hist(Xb, order, cnt, frt, mult, d, B, C, F.COUNT, y=y)
        got = F.level_hist(Xb.to(cuda), order.to(cuda), cnt.to(cuda), frt.to(cuda), mult.to(cuda), d, B, C, F.COUNT,
                           y=y.int().to(cuda))
        assert torch.equal(F.counts_as_int64(got).cpu(), want)
        assert int(want.sum()) == int(mult.sum()) * d


@pytest.mark.parametrize("shape", KSHAPES, ids=_ids)
def test_hist_kernel_real(cuda, shape):
    n, d, B, C = shape
    Xb, mult, y, stats, keep = _trace(shape, F.REAL)
    for lvl, s in keep.items():
        H = F.level_hist(Xb.to(cuda), s["order"].to(cuda), s["cnt"].to(cuda), s["fr_tree"].to(cuda), mult.to(cuda), d, B,
                         C, F.REAL, stats=stats.to(cuda))
        torch.testing.assert_close(H.cpu(), s["H"], rtol=1e-12, atol=0)
    # regression statistics (w, w*y, w*y^2) with positive targets: sums without cancellation
    s = keep[0]
    reg = torch.stack([torch.ones(n, dtype=torch.float64), stats.sum(1) + 1, (stats.sum(1) + 1) ** 2], 1)
    want = F.level_hist(Xb, s["order"], s["cnt"], s["fr_tree"], mult, d, B, 3, F.REAL, stats=reg)
    got = F.level_hist(Xb.to(cuda), s["order"].to(cuda), s["cnt"].to(cuda), s["fr_tree"].to(cuda), mult.to(cuda), d, B,
                       3, F.REAL, stats=reg.to(cuda))
    torch.testing.assert_close(got.cpu(), want, rtol=1e-12, atol=0)


def _near_optimal(H, task, min_leaf, mask, bf, bb, sp):
    """Rule 1b of test_forest.check_forest on the mirror's gain table."""
    table = F.ref_gain_table(H, task, min_leaf, mask)
    M = H.shape[0]
    best = table.reshape(M, -1).max(1).values
    tot = F._ref_prefix(H)[:, 0, -1].double()
    margin = 1e-9 * F.ref_impurity(tot, task)[0].clamp_min(1.0)
    ar = torch.arange(M)
    chosen = table[ar, bf.long(), bb.long()]
    split = sp.bool()
    assert bool((chosen[split] >= best[split] - margin[split]).all())
    assert torch.equal(split, best > F.SPLIT_EPS)


@pytest.mark.parametrize("shape", KSHAPES, ids=_ids)
@pytest.mark.parametrize("task,kind", [(F.GINI, F.COUNT), (F.ENTROPY, F.COUNT), (F.GINI, F.REAL), (F.ENTROPY, F.REAL),
                                       (F.MSE, F.REAL)],
                         ids=["gini-count", "entropy-count", "gini-real", "entropy-real", "mse-real"])
def test_split_kernels(cuda, shape, task, kind):
    n, d, B, C = shape
    if task == F.MSE:
        Xb, mult, y, stats, keep = _trace(shape, F.REAL)
        reg = torch.stack([torch.ones(n, dtype=torch.float64), stats.sum(1) - 1, (stats.sum(1) - 1) ** 2], 1)
        hs = [(F.level_hist(Xb, s["order"], s["cnt"], s["fr_tree"], mult, d, B, 3, F.REAL, stats=reg), s)
              for s in keep.values()]
    else:
        hs = [(s["H"], s) for s in _trace(shape, kind)[4].values()]
    for min_leaf in (1, 20):
        for H, s in hs:
            for mask in (None, s["mask"]):
                cg, cb = F.split_feature(H, kind, task, min_leaf, mask)
                Hg = H.to(cuda) if kind == F.REAL else H.int().to(cuda)
                gg, gb = F.split_feature(Hg, kind, task, min_leaf, None if mask is None else mask.to(cuda))
                torch.testing.assert_close(gg.cpu(), cg, rtol=1e-12, atol=0)
                bf, bb, bg, sp, L, R, Tt = (t.cpu() for t in F.split_node(Hg, kind, gg, gb))
                _near_optimal(H, task, min_leaf, mask, bf, bb, sp)
                torch.testing.assert_close(bg, F.split_node(H, kind, cg, cb)[2], rtol=1e-12, atol=0)
                pre = F._ref_prefix(H)
                ar = torch.arange(H.shape[0])
                torch.testing.assert_close(L, pre[ar, bf.long(), bb.long()].double(), rtol=0, atol=0)
                torch.testing.assert_close(L + R, pre[ar, bf.long(), -1].double(), rtol=1e-12, atol=0)
                torch.testing.assert_close(Tt, pre[:, 0, -1].double(), rtol=0, atol=0)


@pytest.mark.parametrize("kind", [F.COUNT, F.REAL], ids=["count", "real"])
@pytest.mark.parametrize("task", [F.GINI, F.ENTROPY], ids=["gini", "entropy"])
def test_tie_rule_kernel(cuda, kind, task):
    H = tie_histogram(torch.int32 if kind == F.COUNT else torch.float64).to(cuda)
    cg, cb = F.split_feature(H, kind, task, 1, None)
    assert cg[0, 3] == cg[0, 5] and int(cb[0, 3]) == 2 and int(cb[0, 5]) == 2
    bf, bb, bg, sp, L, R, Tt = F.split_node(H, kind, cg, cb)
    assert (int(bf), int(bb), int(sp)) == (3, 2, 1)
    assert L[0].tolist() == [30, 5] and R[0].tolist() == [4, 40] and Tt[0].tolist() == [34, 45]
    mask = torch.ones((1, 8), dtype=torch.uint8)
    mask[0, 3] = 0
    cg, cb = F.split_feature(H, kind, task, 1, mask.to(cuda))
    assert int(F.split_node(H, kind, cg, cb)[0]) == 5 and float(cg[0, 3]) == float("-inf")


@pytest.mark.parametrize("shape", SHAPES, ids=_ids)
@pytest.mark.parametrize("crit", ["gini", "entropy"])
def test_gpu_forest_invariants(cuda, shape, crit):
    n, d, B, C = shape
    X, y, th = _cls(*shape)
    f = fit_and_check(X, y, th, C, 5, 8, "sqrt", 1, crit, device=cuda)
    # same integer histograms, same gains bit for bit: the GPU forest is the mirror's forest
    ref = fit_and_check(X, y, th, C, 5, 8, "sqrt", 1, crit)
    for a, b in zip(f.trees, ref.trees):
        assert a.feature.numel() == b.feature.numel()
    fit_and_check(X, y, th, C, 5, 8, None, 20, crit, device=cuda)


def test_gpu_regression_and_weights_invariants(cuda):
    g = torch.Generator().manual_seed(2)
    X = torch.randn(2000, 8, generator=g, dtype=torch.float64)
    y = X[:, 0] * 2 + (X[:, 1] > 0).double() * X[:, 2] + 0.1 * torch.randn(2000, generator=g, dtype=torch.float64)
    th = T._bins(X, 64)
    stats = torch.stack([torch.ones_like(y), y, y * y], 1)
    f = T.DecisionForest("regression", n_trees=3, max_depth=7, n_bins=64, seed=4, engine="native")
    f.fit(X.to(cuda), y.to(cuda), thresholds=th.to(cuda))
    check_forest(f.trees, X, th, F.bootstrap(4, 0, 3, 0, 2000, "cpu"), stats=stats, seed=4, count=False)
    assert max(t.feature.numel() for t in f.trees) > 31
    Xc, yc, thc = _cls(2000, 7, 16, 3)
    w = torch.rand(2000, generator=g, dtype=torch.float64) + 0.25
    t = T.DecisionTree(max_depth=8, n_bins=16, min_samples_leaf=3, engine="native")
    t.fit(Xc.to(cuda), yc.to(cuda), sample_weight=w.to(cuda), num_classes=3, thresholds=thc.to(cuda))
    check_forest([t], Xc, thc, torch.ones((1, 2000), dtype=torch.uint8),
                 stats=torch.nn.functional.one_hot(yc, 3).double() * w[:, None], count=False)


def test_determinism(cuda):
    X, y, th = _cls(3000, 33, 64, 2)
    fits = []
    for _ in range(2):
        f = T.DecisionForest(n_trees=6, max_depth=8, n_bins=64, seed=2, engine="native")
        fits.append(f.fit(X.to(cuda), y.to(cuda), num_classes=2, thresholds=th.to(cuda)))
    for a, b in zip(fits[0].trees, fits[1].trees):
        assert torch.equal(a.feature, b.feature) and torch.equal(a.left, b.left)
        assert torch.equal(a.threshold, b.threshold) and torch.equal(a.value, b.value)


@pytest.mark.parametrize("n_trees", [1, 8])
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_predict_kernel(cuda, n_trees, dtype):
    X, y, th = _cls(2000, 7, 16, 3)
    f = T.DecisionForest(n_trees=n_trees, max_depth=8, n_bins=16, seed=6, engine="native")
    f.fit(X, y, num_classes=3, thresholds=th)
    if n_trees > 1:  # one tree that is a bare root
        root = T.DecisionTree(max_depth=0, engine="native").fit(X, y, num_classes=3, thresholds=th)
        assert root.feature.numel() == 1
        f.trees[3] = root
    Xq, _ = make_cls(5000, 7, 3, seed=9)
    Xq = Xq.to(dtype)
    thr = torch.cat([t.threshold[t.left >= 0] for t in f.trees])
    fea = torch.cat([t.feature[t.left >= 0] for t in f.trees])
    sel = torch.arange(0, 5000, 3)[:thr.numel()]
    if dtype == torch.float32:
        for t in f.trees:  # thresholds a fp32 sample can sit on
            t.threshold = t.threshold.float().double()
        thr = thr.float().double()
    Xq[sel, fea[:sel.numel()]] = thr[:sel.numel()].to(dtype)  # samples exactly on thresholds
    for n in (1, 63, 5000):
        Q = Xq[:n]
        want = torch.stack([t.predict_proba(Q) for t in f.trees]).mean(0)
        want_leaf = torch.stack([t.apply(Q) for t in f.trees])
        f._pack = None
        assert torch.allclose(f.predict_proba(Q.to(cuda)).cpu(), want, rtol=0, atol=1e-12)
        assert torch.equal(f.apply(Q.to(cuda)).cpu(), want_leaf)
        assert torch.equal(f.predict(Q.to(cuda)).cpu(), want.argmax(1))
    # the mirror of the packed walk agrees too
    p, leaf = F.predict_packed(Xq, F.pack_trees(f.trees, "cpu"), leaves=True)
    assert torch.allclose(p, want, rtol=0, atol=1e-12) and torch.equal(leaf, want_leaf)


def test_unsupported_shapes_raise(cuda):
    X, y, _ = _cls(70, 1, 4, 2)
    Xg, yg = X.to(cuda), y.to(cuda)
    with pytest.raises(ValueError):
        T.DecisionTree(n_bins=300, engine="native").fit(Xg, yg, thresholds=torch.zeros((1, 299), dtype=torch.float64))
    with pytest.raises(ValueError):
        T.DecisionForest(n_trees=2, engine="native").fit(Xg, yg, num_classes=40)
    # the launchers refuse too (status 3), before any launch
    lib = F._lib.kernels()
    H = torch.zeros(8, device=cuda)
    s = F._lib.stream_ptr(cuda)
    assert lib.harp_forest_split_feature(H.data_ptr(), 0, 1, 1, 300, 2, 0, 1.0, None, H.data_ptr(), H.data_ptr(), s) == 3
    assert lib.harp_forest_split_feature(H.data_ptr(), 0, 1, 1, 4, 40, 0, 1.0, None, H.data_ptr(), H.data_ptr(), s) == 3
    assert lib.harp_forest_hist(H.data_ptr(), 16, H.data_ptr(), H.data_ptr(), H.data_ptr(), H.data_ptr(), H.data_ptr(),
                                1, 1, H.data_ptr(), 1, H.data_ptr(), None, 1, 300, 2, 0, H.data_ptr(), s) == 3
    assert lib.harp_forest_bin(H.data_ptr(), 0, 1, 1, H.data_ptr(), 299, H.data_ptr(), 16, s) == 3
    assert lib.harp_forest_predict(H.data_ptr(), 0, 1, 1, H.data_ptr(), H.data_ptr(), H.data_ptr(), H.data_ptr(),
                                   H.data_ptr(), 1, 40, 1, H.data_ptr(), None, s) == 3
    torch.cuda.synchronize()
