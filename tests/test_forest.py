"""Native decision-forest engine on CPU tensors: the torch mirror in ``harp_amd/ops/forest.py``
of the kernels in ``csrc/forest.hip``.

Implementations are never compared by the split they choose: empty adjacent bins and small
nodes produce identical partitions, hence exactly tied gains. ``check_forest`` instead rebuilds
every node's histogram from the rows that reach it and checks the trained trees against it
(statistics, feature subset, min_samples_leaf, near-optimal gain, leaf rule, numbering); the
tie rule is tested on a constructed histogram. ``tests/test_forest_gpu.py`` reuses the helpers.
"""
import itertools
import math
import os

import pytest
import torch

from harp_amd.core.writable import DataInput, DataOutput
from harp_amd.models import trees as T
from harp_amd.ops import forest as F
from harp_amd.runtime.launcher import launch

SHAPES = [(70, 1, 4, 2), (2000, 7, 16, 3), (3000, 33, 64, 2), (1500, 5, 256, 11)]  # n, d, n_bins, classes


def make_cls(n, d, C, seed=0):
    """Classification data with some coarsely quantised features (repeated quantiles -> runs of
    empty bins) and labels that need several levels."""
    g = torch.Generator().manual_seed(seed)
    X = torch.randn(n, d, generator=g, dtype=torch.float64)
    X[:, ::3] = (X[:, ::3] * 3).round() / 3
    s = X[:, 0] * 1.5 + X[:, d // 2] * X[:, d - 1].sign() + 0.4 * torch.randn(n, generator=g, dtype=torch.float64)
    q = torch.quantile(s, torch.linspace(0, 1, C + 1, dtype=torch.float64)[1:-1])
    return X, torch.bucketize(s, q)


def _depths(left):
    dep = torch.zeros(left.numel(), dtype=torch.int64)
    for i in range(left.numel()):  # level order: parents come first
        if left[i] >= 0:
            dep[left[i]] = dep[left[i] + 1] = dep[i] + 1
    return dep


def check_forest(trees, X, th, mult, *, y=None, stats=None, seed=0, tree0=0, count=True):
    """Invariants of natively trained ``trees`` (CPU arrays) on their training rows ``X`` (CPU)
    with thresholds ``th``, row multiplicities ``mult`` [T, n] and labels ``y`` or per-row
    statistics ``stats`` [n, C]; ``seed`` / ``tree0`` key the mirrored feature subsets."""
    n, d = X.shape
    B = th.shape[1] + 1
    Xb = torch.searchsorted(th, X.double().t().contiguous(), right=True).t()
    for ti, tree in enumerate(trees):
        C = tree.value.shape[1] if tree.task == "classification" else 3
        w = mult[ti].double()
        S = torch.nn.functional.one_hot(y.long(), C).double() * w[:, None] if stats is None else stats * w[:, None]
        f, left = tree.feature, tree.left
        N = f.numel()
        inner = left >= 0
        # d. level-order numbering: the k-th internal node (in id order) owns children 2k+1, 2k+2
        assert torch.equal(left[inner], 1 + 2 * torch.arange(int(inner.sum())))
        assert N == 1 + 2 * int(inner.sum())
        assert bool((f[inner] >= 0).all()) and bool((f[~inner] == -1).all())
        bins = torch.zeros(N, dtype=torch.int64)
        for i in torch.nonzero(inner)[:, 0].tolist():
            bins[i] = int(torch.searchsorted(th[f[i]], tree.threshold[i]))
            assert th[f[i], bins[i]] == tree.threshold[i]
        dep = _depths(left)
        k_sub = T._n_sub(tree.max_features, d)
        node_of = torch.zeros(n, dtype=torch.int64)
        live = w > 0
        for level in range(int(dep.max()) + 1):
            ids = torch.nonzero(dep == level)[:, 0]
            m = ids.numel()
            loc = torch.full((N,), -1, dtype=torch.int64)
            loc[ids] = torch.arange(m)
            act = live & (loc[node_of] >= 0)
            li, lx, ls = loc[node_of][act], Xb[act], S[act]
            H = torch.zeros((m * d * B, C), dtype=torch.float64)
            idx = (li[:, None] * d + torch.arange(d)[None, :]) * B + lx
            H.index_add_(0, idx.reshape(-1), ls[:, None, :].expand(-1, d, -1).reshape(-1, C))
            H = H.view(m, d, B, C)
            Lc = H.cumsum(2)[:, :, :-1, :]
            tot = H.sum(2, keepdim=True)
            Rc = tot - Lc
            # a. node statistics
            node = tot[:, 0, 0, :]
            if tree.task == "classification":
                want = node / node.sum(1, keepdim=True).clamp_min(1e-300)
            else:
                want = (node[:, 1] / node[:, 0].clamp_min(1e-300))[:, None]
            if count:
                assert torch.allclose(tree.value[ids], want, rtol=0, atol=1e-14)
            else:
                assert torch.allclose(tree.value[ids], want, rtol=1e-9, atol=0)
            # b / c. splits against the rebuilt gain table
            gain = tree._gain(Lc, Rc, tot)
            nL, nR = tree._count(Lc), tree._count(Rc)
            ok = (nL >= tree.min_leaf) & (nR >= tree.min_leaf)
            if k_sub is not None and k_sub < d:
                sub = F.feature_subset(seed, torch.full((m,), tree0 + ti, dtype=torch.int32), ids.int(), d, k_sub).bool()
                ok = ok & sub[:, :, None]
            else:
                sub = torch.ones((m, d), dtype=torch.bool)
            allowed = torch.where(ok, gain, torch.full_like(gain, float("-inf")))
            best = allowed.reshape(m, -1).max(1).values if B > 1 else torch.full((m,), float("-inf"))
            margin = 1e-9 * tree._impurity(node).clamp_min(1.0)
            for j, i in enumerate(ids.tolist()):
                if left[i] >= 0:
                    fi, bi = int(f[i]), int(bins[i])
                    assert bool(sub[j, fi]), (ti, i)
                    assert nL[j, fi, bi] >= tree.min_leaf and nR[j, fi, bi] >= tree.min_leaf, (ti, i)
                    assert gain[j, fi, bi] >= best[j] - margin[j], (ti, i, float(gain[j, fi, bi]), float(best[j]))
                elif level < tree.max_depth:
                    assert best[j] <= 1e-12 + margin[j], (ti, i, float(best[j]))
            # route with the tree's own splits, in bin space
            fs = f[node_of].clamp_min(0)
            right = Xb.gather(1, fs[:, None])[:, 0] > bins[node_of]
            node_of = torch.where(left[node_of] >= 0, left[node_of] + right.long(), node_of)


_data = {}


def _cls(n, d, B, C):
    if (n, d, B, C) not in _data:
        X, y = make_cls(n, d, C)
        _data[(n, d, B, C)] = (X, y, T._bins(X, B))
    return _data[(n, d, B, C)]


def fit_and_check(X, y, th, C, n_trees, depth, mf, min_leaf, crit, seed=5, device=None):
    Xd, yd = (X, y) if device is None else (X.to(device), y.to(device))
    f = T.DecisionForest(n_trees=n_trees, max_depth=depth, max_features=mf, n_bins=th.shape[1] + 1, seed=seed,
                         min_samples_leaf=min_leaf, engine="native", criterion=crit)
    f.fit(Xd, yd, num_classes=C, thresholds=th if device is None else th.to(device))
    assert len(f.trees) == n_trees
    mult = F.bootstrap(seed, 0, n_trees, 0, X.shape[0], "cpu")
    check_forest(f.trees, X, th, mult, y=y, seed=seed)
    return f


CONFIGS = list(itertools.product((1, 5), (1, 8), (None, "sqrt"), (1, 20), ("gini", "entropy")))


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("cfg", CONFIGS, ids=lambda c: "-".join(map(str, c)))
def test_forest_invariants(shape, cfg):
    n, d, B, C = shape
    X, y, th = _cls(*shape)
    f = fit_and_check(X, y, th, C, *cfg)
    if cfg[1] == 8 and cfg[3] == 1 and n >= 1500:
        assert max(t.feature.numel() for t in f.trees) > 15  # the trees do grow


def test_invariants_regression():
    g = torch.Generator().manual_seed(2)
    X = torch.randn(2000, 8, generator=g, dtype=torch.float64)
    y = X[:, 0] * 2 + (X[:, 1] > 0).double() * X[:, 2] + 0.1 * torch.randn(2000, generator=g, dtype=torch.float64)
    th = T._bins(X, 64)
    t = T.DecisionTree("regression", max_depth=7, n_bins=64, engine="native").fit(X, y, thresholds=th)
    stats = torch.stack([torch.ones_like(y), y, y * y], 1)
    check_forest([t], X, th, torch.ones((1, 2000), dtype=torch.uint8), stats=stats, count=False)
    assert t.feature.numel() > 31
    ref = T.DecisionTree("regression", max_depth=7, n_bins=64).fit(X, y, thresholds=th)
    assert ((t.predict(X) - y) ** 2).mean() <= ((ref.predict(X) - y) ** 2).mean() * 1.01
    f = T.DecisionForest("regression", n_trees=3, max_depth=7, n_bins=64, seed=4, engine="native")
    f.fit(X, y, thresholds=th)
    check_forest(f.trees, X, th, F.bootstrap(4, 0, 3, 0, 2000, "cpu"), stats=stats, seed=4, count=False)


def test_invariants_real_weights():
    X, y, th = _cls(2000, 7, 16, 3)
    g = torch.Generator().manual_seed(3)
    w = torch.rand(2000, generator=g, dtype=torch.float64) + 0.25
    t = T.DecisionTree(max_depth=8, n_bins=16, min_samples_leaf=3, engine="native")
    t.fit(X, y, sample_weight=w, num_classes=3, thresholds=th)
    stats = torch.nn.functional.one_hot(y, 3).double() * w[:, None]
    check_forest([t], X, th, torch.ones((1, 2000), dtype=torch.uint8), stats=stats, count=False)
    # integer weights take the exact count kind
    wi = torch.randint(0, 4, (2000,), generator=g)
    t = T.DecisionTree(max_depth=8, n_bins=16, engine="native").fit(X, y, sample_weight=wi.double(), num_classes=3,
                                                                    thresholds=th)
    check_forest([t], X, th, wi.to(torch.uint8)[None, :], y=y)


def test_invariants_constant_feature():
    X, y, _ = _cls(2000, 7, 16, 3)
    X = X.clone()
    X[:, 2] = 1.25
    th = T._bins(X, 16)
    f = fit_and_check(X, y, th, 3, 5, 8, "sqrt", 1, "gini")
    assert all(bool((t.feature != 2).all()) for t in f.trees)


def test_invariants_one_tree_stops_early():
    """Labels decided by one threshold: a tree that may split on feature 0 at its root is done
    at depth 1, the trees whose root subset lacks it go on."""
    g = torch.Generator().manual_seed(7)
    X = torch.randn(1500, 6, generator=g, dtype=torch.float64)
    th = T._bins(X, 16)
    y = (X[:, 0] >= th[0, 7]).long()
    f = fit_and_check(X, y, th, 2, 5, 8, 2, 1, "gini", seed=11)
    sizes = sorted(t.feature.numel() for t in f.trees)
    assert sizes[0] == 3 and sizes[-1] > 3, sizes
    assert (f.predict(X) == y).double().mean() > 0.97


def test_bootstrap_multiplicities():
    w = F.bootstrap(9, 0, 10, 0, 10000, "cpu")
    assert w.dtype == torch.uint8 and w.shape == (10, 10000)
    # a row's multiplicity depends on its global index, not on the shard it is computed in
    assert torch.equal(F.bootstrap(9, 0, 10, 3000, 4000, "cpu"), w[:, 3000:7000])
    assert torch.equal(F.bootstrap(9, 4, 3, 9999, 1, "cpu"), w[4:7, 9999:])
    wd = w.double()
    assert abs(float(wd.mean()) - 1) < 0.02 and abs(float(wd.var()) - 1) < 0.02
    assert int(w.max()) <= F.MAX_MULT
    assert not torch.equal(F.bootstrap(10, 0, 1, 0, 10000, "cpu"), w[:1])
    # the table is the Poisson(1) cdf scaled to 2**32
    cdf, term = 0.0, math.exp(-1)
    for k, v in enumerate(F.POISSON1_TABLE):
        cdf += term
        term /= k + 1
        assert abs(v - cdf * 2.0 ** 32) <= 2


def tie_histogram(dtype):
    """[1, 8, 16, 2]: feature 5 copies feature 3, whose bins 3..8 are empty, so candidates
    2..8 of both give the same (best) partition; the other features separate nothing."""
    H = torch.zeros((1, 8, 16, 2), dtype=dtype)
    H[0, :, 0] = torch.tensor([17, 22])
    H[0, :, 1] = torch.tensor([17, 23])
    for f in (3, 5):
        H[0, f] = 0
        H[0, f, 2] = torch.tensor([30, 5])
        H[0, f, 9] = torch.tensor([4, 40])
    return H


@pytest.mark.parametrize("kind", [F.COUNT, F.REAL])
@pytest.mark.parametrize("task", [F.GINI, F.ENTROPY])
def test_tie_rule(kind, task):
    H = tie_histogram(torch.int64 if kind == F.COUNT else torch.float64)
    cg, cb = F.split_feature(H, kind, task, 1, None)
    assert cg[0, 3] == cg[0, 5] and cb[0, 3] == 2 and cb[0, 5] == 2
    bf, bb, bg, sp, L, R, Tt = F.split_node(H, kind, cg, cb)
    assert (int(bf), int(bb), int(sp)) == (3, 2, 1)
    assert L[0].tolist() == [30, 5] and R[0].tolist() == [4, 40] and Tt[0].tolist() == [34, 45]
    table = F.ref_gain_table(H, task, 1, None)[0]
    assert bool((table[3, 2:9] == bg[0]).all()) and bool((table[5, 2:9] == bg[0]).all())
    assert float(table.max()) == float(bg)
    # with feature 3 masked out the copy wins
    mask = torch.ones((1, 8), dtype=torch.uint8)
    mask[0, 3] = 0
    cg, cb = F.split_feature(H, kind, task, 1, mask)
    assert int(F.split_node(H, kind, cg, cb)[0]) == 5


def test_mirror_gain_formulas():
    """The mirror's class-ordered sums and its log2 agree with DecisionTree._impurity."""
    g = torch.Generator().manual_seed(1)
    S = torch.randint(0, 50, (200, 11), generator=g).double()
    for task, crit in ((F.GINI, "gini"), (F.ENTROPY, "entropy")):
        ref = T.DecisionTree(criterion=crit)._impurity(S)
        assert torch.allclose(F.ref_impurity(S, task)[0], ref, rtol=1e-12, atol=1e-9)
    p = torch.rand(1000, generator=g, dtype=torch.float64).clamp_min(1e-300)
    assert torch.allclose(F._ref_log2(p), torch.log2(p), rtol=1e-14, atol=1e-15)
    assert float(F._ref_log2(torch.tensor([1.0], dtype=torch.float64))) == 0.0


@pytest.fixture(scope="module")
def sk_data():
    sk_ds = pytest.importorskip("sklearn.datasets")
    X, y = sk_ds.make_classification(3000, 16, n_informative=8, n_classes=3, random_state=0)
    X, y = torch.tensor(X), torch.tensor(y)
    return X[:2000], y[:2000], X[2000:], y[2000:]


def _acc(m, X, y):
    return (m.predict(X) == y).double().mean().item()


def test_accuracy_against_existing_gates(sk_data):
    from sklearn.tree import DecisionTreeClassifier

    Xtr, ytr, Xte, yte = sk_data
    tree = T.DecisionTree(max_depth=6, n_bins=128, engine="native").fit(Xtr, ytr)
    ours = _acc(tree, Xte, yte)
    ref = DecisionTreeClassifier(max_depth=6, random_state=0).fit(Xtr, ytr).score(Xte, yte)
    assert ours > ref - 0.04
    rf = T.DecisionForest(n_trees=25, max_depth=10, engine="native").fit(Xtr, ytr)
    assert _acc(rf, Xte, yte) > ours
    p = rf.predict_proba(Xte)
    assert torch.allclose(p.sum(1), torch.ones(1000, dtype=torch.float64))
    assert rf.apply(Xte).shape == (25, 1000)


def test_native_tree_writable_roundtrip(sk_data):
    Xtr, ytr, Xte, _ = sk_data
    t = T.DecisionTree(max_depth=4, engine="native").fit(Xtr, ytr)
    out = DataOutput()
    t.write(out)
    t2 = T.DecisionTree()
    t2.read(DataInput(out.getvalue()))
    assert torch.equal(t.predict(Xte), t2.predict(Xte))
    assert torch.equal(t.predict_proba(Xte), t2.predict_proba(Xte))


def test_engine_argument():
    with pytest.raises(ValueError):
        T.DecisionTree(engine="triton")
    X, y, th = _cls(70, 1, 4, 2)
    with pytest.raises(ValueError):
        T.DecisionTree(n_bins=300, engine="native").fit(X, y, thresholds=torch.zeros((1, 299), dtype=torch.float64))
    with pytest.raises(ValueError):
        T.DecisionTree(engine="native").fit(X, y, num_classes=40, thresholds=th)
    with pytest.raises(ValueError):
        T.DecisionForest(n_trees=2).fit_distributed(X, y, None, mode="rows")


def _arrays(f):
    return [(t.feature, t.left, t.threshold, t.value) for t in f.trees]


def _rows_job(comm, X, y, th, cut):
    sl = slice(0, cut) if comm.rank == 0 else slice(cut, X.shape[0])
    f = T.DecisionForest(n_trees=4, max_depth=6, n_bins=th.shape[1] + 1, seed=3, engine="native")
    f.fit_distributed(X[sl], y[sl], comm, num_classes=3, mode="rows", thresholds=th)
    return _arrays(f)


def test_rows_mode_two_workers():
    X, y, th = _cls(2000, 7, 16, 3)
    res = launch(_rows_job, 2, args=(X, y, th, 700), timeout=300)
    one = T.DecisionForest(n_trees=4, max_depth=6, n_bins=16, seed=3, engine="native")
    one.fit(X, y, num_classes=3, thresholds=th)
    for a, b, c in zip(res[0], res[1], _arrays(one)):
        for x, z, w in zip(a, b, c):
            assert torch.equal(x, z) and torch.equal(x, w)
    assert max(t.feature.numel() for t in one.trees) > 15


def test_cli_daal_dforest(tmp_path):
    from harp_amd import cli

    X, y, _ = _cls(2000, 7, 16, 3)
    inp, work = tmp_path / "in", tmp_path / "work"
    os.makedirs(inp)
    for i, sl in enumerate((slice(0, 900), slice(900, 2000))):
        rows = torch.cat([X[sl], y[sl].double()[:, None]], 1).tolist()
        with open(inp / f"part-{i}.csv", "w") as fh:
            fh.write("\n".join(",".join(repr(v) for v in r) for r in rows) + "\n")
    rc = cli.main(["daal", "dforest", "2", "1", "0", "1", str(inp), str(work), "--k", "3", "--n-trees", "6",
                   "--max-depth", "6", "--backend", "gloo"])
    assert rc == 0
    import numpy as np

    nodes = np.loadtxt(work / "dforest_nodes.csv", delimiter=",", ndmin=2)  # tree, feature, threshold, left
    values = np.loadtxt(work / "dforest_values.csv", delimiter=",", ndmin=2)
    assert nodes.shape[0] == values.shape[0] and values.shape[1] == 3 and nodes.shape[1] == 4
    trees = []
    for t in range(6):
        sel = nodes[:, 0] == t
        tr = T.DecisionTree(max_depth=6)
        tr.feature = torch.tensor(nodes[sel, 1]).long()
        tr.threshold = torch.tensor(nodes[sel, 2])
        tr.left = torch.tensor(nodes[sel, 3]).long()
        tr.value = torch.tensor(values[sel])
        assert tr.feature.numel() >= 3
        trees.append(tr)
    f = T.DecisionForest(n_trees=6)
    f.trees = trees
    # the margin test_trees.py grants between implementations of the same split rule
    ref = T.DecisionForest(n_trees=6, max_depth=6).fit(X, y, num_classes=3)
    assert _acc(f, X, y) > _acc(ref, X, y) - 0.04
