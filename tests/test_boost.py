"""The native boosting engine (``harp_amd/ops/boost.py``, CPU mirror) against the torch engine
of ``harp_amd/models/trees.py``: stump, AdaBoost, LogitBoost, the BrownBoost step, row-sharded
training and the ``daal`` CLI apps. The GPU kernels are held to this mirror in
``tests/test_boost_gpu.py``.

Every set has n <= 200,000 rows, so both engines compute the same quantile thresholds."""
import math
import os

import numpy as np
import pytest
import torch

from harp_amd.models import trees as T
from harp_amd.ops import boost as BO
from harp_amd.runtime.launcher import launch
from harp_amd.utils import datasets as DS

from tests.test_reference_datasets import P

SHAPES = [(3000, 8, 3), (2049, 17, 2), (4097, 5, 4), (257, 3, 2)]  # n, d, classes
_data = {}


def make_boost_data(n, d, K, seed=0):
    """Labels: a noisy function of three features, cut at its quantiles into K classes."""
    key = (n, d, K, seed)
    if key not in _data:
        g = torch.Generator().manual_seed(seed)
        X = torch.randn(n, d, generator=g, dtype=torch.float64)
        s = (X[:, 0] + 0.7 * X[:, min(1, d - 1)] - 0.5 * X[:, min(2, d - 1)]
             + 0.6 * torch.randn(n, generator=g, dtype=torch.float64))
        q = torch.quantile(s, torch.linspace(0, 1, K + 1, dtype=torch.float64)[1:-1])
        _data[key] = (X, torch.bucketize(s, q))
    return _data[key]


def _ids(s):
    return "x".join(map(str, s))


def _roots(learners):
    return [(int(h.feature[0]), float(h.threshold[0])) for h in learners]


def _same_adaboost(a, b):
    assert len(a.learners) == len(b.learners) > 1
    assert _roots(a.learners) == _roots(b.learners)
    rel = max(abs(p - q) / abs(p) for p, q in zip(a.alphas, b.alphas))
    print(f"alpha rel {rel:.3g}")
    assert rel <= 1e-10


# ---------------------------------------------------------------- 1. AdaBoost
@pytest.mark.parametrize("shape", SHAPES, ids=_ids)
def test_adaboost_matches_torch_engine(shape):
    X, y = make_boost_data(*shape)
    _same_adaboost(T.AdaBoost(25).fit(X, y), T.AdaBoost(25, engine="native").fit(X, y))


def test_adaboost_matches_torch_engine_on_reference_fixture():
    X, y = DS.load_features_labels(P("daal_adaboost", "train"))
    yb = (y > 0).long()
    _same_adaboost(T.AdaBoost(30).fit(X, yb), T.AdaBoost(30, engine="native").fit(X, yb))


def test_adaboost_deep_learners_share_the_bins():
    X, y = make_boost_data(3000, 8, 3)
    m = T.AdaBoost(8, learner_depth=2, engine="native").fit(X, y)
    assert len(m.learners) == 8 and max(h.feature.numel() for h in m.learners) > 3
    acc = float((m.predict(X) == y).double().mean())
    assert acc > float((T.stump(X, y, engine="native").predict(X) == y).double().mean())
    assert float((m._decision_packed(X) - m.decision(X)).abs().max()) <= 1e-12


# ---------------------------------------------------------------- 2. LogitBoost
@pytest.mark.parametrize("shape", SHAPES, ids=_ids)
def test_logitboost_matches_torch_engine(shape):
    X, y = make_boost_data(*shape)
    a, b = T.LogitBoost(10).fit(X, y), T.LogitBoost(10, engine="native").fit(X, y)
    diff = float((a.decision(X) - b.decision(X)).abs().max())
    print(f"decision diff {diff:.3g}")
    assert diff <= 1e-6
    assert len(b.rounds) == 10 and all(len(fs) == shape[2] for fs in b.rounds)
    assert float((b._decision_packed(X) - b.decision(X)).abs().max()) <= 1e-12


def test_logitboost_deep_learners():
    X, y = make_boost_data(3000, 8, 3)
    a, b = T.LogitBoost(4, depth=2).fit(X, y), T.LogitBoost(4, depth=2, engine="native").fit(X, y)
    assert float(((a.predict(X) == y).double().mean() - (b.predict(X) == y).double().mean()).abs()) < 0.02


# ---------------------------------------------------------------- 3. stump
@pytest.mark.parametrize("shape", SHAPES, ids=_ids)
@pytest.mark.parametrize("weighted", [False, True])
def test_stump_matches_torch_engine(shape, weighted):
    X, y = make_boost_data(*shape)
    g = torch.Generator().manual_seed(5)
    w = torch.rand(shape[0], generator=g, dtype=torch.float64) + 0.5 if weighted else None
    a, b = T.stump(X, y, w), T.stump(X, y, w, engine="native")
    assert a.feature.tolist() == b.feature.tolist() and a.left.tolist() == b.left.tolist()
    assert torch.equal(a.threshold, b.threshold)
    assert float((a.value - b.value).abs().max()) <= 1e-12


# ---------------------------------------------------------------- 4. errors, independent of the histograms
@pytest.mark.parametrize("shape", SHAPES, ids=_ids)
def test_adaboost_errors_by_replay(shape):
    """Every recorded error is the weighted misclassification of that stump on raw
    ``x >= threshold``, with the weights replayed in plain torch."""
    X, y = make_boost_data(*shape)
    m = T.AdaBoost(25, engine="native").fit(X, y)
    w = torch.full((shape[0],), 1.0 / shape[0], dtype=torch.float64)
    for h, a, e in zip(m.learners, m.alphas, m.errors):
        cls = h.value.argmax(1)
        pred = torch.where(X[:, int(h.feature[0])] >= h.threshold[0], cls[2], cls[1])
        miss = (pred != y).double()
        err = float((w * miss).sum() / w.sum())
        assert abs(err - e) <= 1e-12
        assert abs(a - (math.log((1 - err) / max(err, 1e-12)) + math.log(shape[2] - 1))) <= 1e-9
        w = w * torch.exp(a * miss)
        w = w / w.sum()


# ---------------------------------------------------------------- 5. BrownBoost step
def _brown_state(n, seed):
    g = torch.Generator().manual_seed(seed)
    r = 0.4 * torch.randn(n, generator=g, dtype=torch.float64)
    u = torch.where(torch.rand(n, generator=g, dtype=torch.float64) < 0.7, 1.0, -1.0).double()
    return r, u


@pytest.mark.parametrize("frac", [1.0, 0.5, 1e-3])
def test_brown_step_matches_torch_step(frac):
    """The device-side search brackets the same roots as the torch step. A step that ends
    because the time runs out returns t = s exactly and the potential it leaves is at most the
    target; every other step conserves the potential."""
    c, nu = 2.0, 1e-3
    s = frac * c
    r, u = _brown_state(1500, 11)
    assert float((torch.exp(-(r + s) ** 2 / c) * u).sum()) > 0
    a0, t0 = T.brown_line_search(r, u, s, c, 60, nu)
    a1, t1, reads = BO.brown_solve(r, u, s, c, 60, nu)
    print(f"s={s} torch ({a0}, {t0}) native ({a1}, {t1}) reads {reads}")
    assert abs(a1 - a0) <= 2e-6
    pot = lambda z: float((1 - torch.erf(z / math.sqrt(c))).sum())
    target, after = pot(r + s), pot(r + s - t1 + a1 * u)
    assert (t1 == s) == (frac == 1e-3)  # only the state with almost no time left runs out
    if t1 == s:
        assert t0 == s and after <= target
    else:
        assert abs(after - target) <= 1e-9 * abs(target)
        assert abs(t1 - t0) <= 1e-6


def test_brown_t_search_runs_out_exactly():
    c, s = 2.0, 1e-3
    r, u = _brown_state(300, 3)
    scal = torch.tensor([s, c], dtype=torch.float64)
    target = BO.brown_sums(r, u, scal, torch.zeros((1, 2), dtype=torch.float64))[0, 0]
    assert float(BO.brown_t_search(r, u, scal, 5.0, target)[4]) == s


def test_brownboost_on_reference_fixture():
    X, y = DS.load_features_labels(P("daal_brownboost", "train"))
    Xt, yt = DS.load_features_labels(P("daal_brownboost", "test"))
    yb, ybt = (y > 0).long(), (yt > 0).long()
    a = T.BrownBoost(c=2.0, max_rounds=5).fit(X, yb)
    b = T.BrownBoost(c=2.0, max_rounds=5, engine="native").fit(X, yb)
    assert _roots(a.learners[:1]) == _roots(b.learners[:1])
    acc = lambda m: float((m.predict(Xt) == ybt).double().mean())
    assert acc(b) >= acc(a) - 0.02


def test_brownboost_native_matches_torch_engine_synthetic():
    X, y = make_boost_data(2049, 17, 2)
    a = T.BrownBoost(c=2.0, max_rounds=4).fit(X, y)
    b = T.BrownBoost(c=2.0, max_rounds=4, engine="native").fit(X, y)
    assert _roots(a.learners) == _roots(b.learners)
    assert max(abs(p - q) for p, q in zip(a.alphas, b.alphas)) <= 2e-6
    assert all(k >= 2 for k in b.host_reads)


# ---------------------------------------------------------------- 6. gloo, two row shards
def _rows_job(comm, X, y, th, cut):
    sl = slice(0, cut) if comm.rank == 0 else slice(cut, X.shape[0])
    K = int(y.max()) + 1
    a = T.AdaBoost(12, engine="native").fit_distributed(X[sl], y[sl], comm, num_classes=K, thresholds=th)
    l = T.LogitBoost(6, engine="native").fit_distributed(X[sl], y[sl], comm, num_classes=K, thresholds=th)
    return _roots(a.learners), a.alphas, l.decision(X)


def test_fit_distributed_two_workers():
    X, y = make_boost_data(3000, 8, 3, seed=2)
    th = T._bins(X, 256)
    res = launch(_rows_job, 2, args=(X, y, th, 1100), timeout=300)
    a = T.AdaBoost(12, engine="native").fit(X, y, num_classes=3, thresholds=th)
    l = T.LogitBoost(6, engine="native").fit(X, y, num_classes=3, thresholds=th)
    for roots, alphas, dec in res:
        assert roots == _roots(a.learners) and len(roots) == 12
        assert max(abs(p - q) for p, q in zip(alphas, a.alphas)) <= 1e-9
        assert float((dec - l.decision(X)).abs().max()) <= 1e-9


# ---------------------------------------------------------------- 7. CLI
@pytest.mark.parametrize("algo", ["adaboost", "logitboost"])
def test_cli_daal_boost(tmp_path, algo):
    """Both engines over two shard files. The node tables (learner, feature, threshold, left)
    are identical. The leaf values are quotients of fp64 sums of at most 2049 terms of order
    1 that the engines accumulate under different weight normalisations (AdaBoost) or in
    different orders (LogitBoost), so they cannot agree bit for bit. They are held to 1e-12,
    the bound of the stump's leaf values above: two orders of one such sum differ by at most
    2 m 2^-53 = 5e-13 relative (the engines differ by 3e-15 and 3e-14 on these sets)."""
    from harp_amd import cli

    X, y = make_boost_data(2049, 17, 2)
    inp = tmp_path / "in"
    os.makedirs(inp)
    lab = (2 * y - 1).double() if algo == "adaboost" else y.double()  # adaboost: the -1 / +1 convention
    for i, sl in enumerate((slice(0, 900), slice(900, 2049))):
        rows = torch.cat([X[sl], lab[sl][:, None]], 1).tolist()
        with open(inp / f"part-{i}.csv", "w") as fh:
            fh.write("\n".join(",".join(repr(v) for v in r) for r in rows) + "\n")
    out = {}
    for engine in T.ENGINES:
        work = tmp_path / engine
        rc = cli.main(["daal", algo, "1", "1", "0", "1", str(inp), str(work), "--rounds", "6", "--k", "2",
                       "--engine", engine, "--backend", "gloo"])
        assert rc == 0
        out[engine] = [np.loadtxt(work / f"{algo}_{k}.csv", delimiter=",", ndmin=2)
                       for k in ("nodes", "values", "alphas")]
    (n0, v0, a0), (n1, v1, a1) = out["torch"], out["native"]
    assert n0.shape == (18 if algo == "adaboost" else 36, 4)
    assert np.array_equal(n0, n1)
    print(f"values differ by {np.abs(v0 - v1).max():.3g}")
    assert np.abs(v0 - v1).max() <= 1e-12
    assert np.abs(a0 - a1).max() <= 1e-10 * np.abs(a0).max()


def test_cli_daal_boost_sharded_native(tmp_path):
    """Two workers, one shard file each. Native engine: the model of ``fit_distributed``,
    i.e. of one process on all rows with the quantiles of rank 0's shard. Torch engine: every
    worker trains on the gathered rows, the model of one process on all rows."""
    from types import SimpleNamespace

    from harp_amd import cli

    X, y = make_boost_data(2049, 17, 2)
    inp, work = tmp_path / "in", tmp_path / "work"
    os.makedirs(inp)
    for i, sl in enumerate((slice(0, 900), slice(900, 2049))):
        rows = torch.cat([X[sl], y[sl].double()[:, None]], 1).tolist()
        with open(inp / f"part-{i}.csv", "w") as fh:
            fh.write("\n".join(",".join(repr(v) for v in r) for r in rows) + "\n")
    first = cli._my_files(SimpleNamespace(world_size=2, rank=0), str(inp))  # rank 0's shard
    assert len(first) == 1
    X0 = DS.load_dense_csv(first[0])[:, :-1]
    want = {"native": T.AdaBoost(6, engine="native").fit(X, y, num_classes=2, thresholds=T._bins(X0, 256)),
            "torch": T.AdaBoost(6).fit(X, y, num_classes=2)}
    for engine, m in want.items():
        assert cli.main(["daal", "adaboost", "2", "1", "0", "1", str(inp), str(work), "--rounds", "6", "--engine",
                         engine, "--backend", "gloo"]) == 0
        nodes = np.loadtxt(work / "adaboost_nodes.csv", delimiter=",", ndmin=2)
        alphas = np.loadtxt(work / "adaboost_alphas.csv", delimiter=",", ndmin=2).reshape(-1)
        assert nodes.shape == (18, 4) and alphas.size == 6
        assert [(int(f), t) for f, t in nodes[0::3, 1:3].tolist()] == _roots(m.learners), engine
        assert np.abs(alphas - np.array(m.alphas)).max() <= 1e-9, engine

    for algo in ("stump", "brownboost"):  # one worker's rows only
        with pytest.raises(ValueError, match="maps = 1"):
            cli._run_daal_boost(SimpleNamespace(world_size=2, rank=0), {"algo": algo, "engine": "native"}, None)
    for algo in ("stump", "brownboost"):
        assert cli.main(["daal", algo, "1", "1", "0", "1", str(inp), str(work), "--rounds", "2", "--backend",
                         "gloo"]) == 0
        assert np.loadtxt(work / f"{algo}_nodes.csv", delimiter=",", ndmin=2).shape[1] == 4


# ---------------------------------------------------------------- 8. limits
def test_limits_and_engine_argument():
    X, y = make_boost_data(257, 3, 2)
    wide = torch.zeros((3, 256), dtype=torch.float64)  # 257 bins
    for make in (lambda: T.AdaBoost(2, engine="native"), lambda: T.LogitBoost(2, engine="native"),
                 lambda: T.BrownBoost(max_rounds=2, engine="native")):
        with pytest.raises(ValueError):
            make().fit(X, y, thresholds=wide)
    for make in (lambda: T.AdaBoost(2, engine="native"), lambda: T.LogitBoost(2, engine="native")):
        with pytest.raises(ValueError):
            make().fit(X, y, num_classes=33)
    with pytest.raises(ValueError):
        T.stump(X, y, num_classes=33, engine="native")
    for make in (lambda: T.AdaBoost(engine="triton"), lambda: T.LogitBoost(engine="triton"),
                 lambda: T.BrownBoost(engine="triton"), lambda: T.stump(X, y, engine="triton")):
        with pytest.raises(ValueError):
            make()
    for m in (T.AdaBoost(2), T.LogitBoost(2)):
        with pytest.raises(ValueError):
            m.fit_distributed(X, y, None)
    for m in (T.AdaBoost(2), T.LogitBoost(2), T.BrownBoost(max_rounds=2)):  # the torch engine bins per learner
        with pytest.raises(ValueError, match="native"):
            m.fit(X, y, thresholds=T._bins(X, 256))
    for m in (T.AdaBoost(2), T.LogitBoost(2)):
        with pytest.raises(ValueError, match="native"):
            m.fit(X, y, trace=lambda t, s: None)
    with pytest.raises(ValueError):
        BO.brown_sums(torch.zeros(4, dtype=torch.float64), torch.ones(4, dtype=torch.float64),
                      torch.ones(2, dtype=torch.float64), torch.zeros((65, 2), dtype=torch.float64))


def test_models_of_the_two_engines_are_interchangeable():
    X, y = make_boost_data(3000, 8, 3)
    a, b = T.AdaBoost(5).fit(X, y), T.AdaBoost(5, engine="native").fit(X, y)
    before = b._decision_packed(X)
    a.learners, b.learners = b.learners, a.learners
    assert torch.equal(a.predict(X), b.predict(X))
    # the packed route follows the model: other learners, other alphas, edited leaves
    b.learners = T.AdaBoost(5, engine="native").fit(X[:, [3, 4, 5]], y).learners
    assert float((b._decision_packed(X) - b._decision_loop(X)).abs().max()) <= 1e-12
    assert float((b._decision_packed(X) - before).abs().max()) > 0.1
    b.alphas = [2 * v for v in b.alphas]
    assert float((b._decision_packed(X) - b._decision_loop(X)).abs().max()) <= 1e-12
    lb = T.LogitBoost(3, engine="native").fit(X, y)
    lb._decision_packed(X)
    lb.rounds[0][0].value = lb.rounds[0][0].value + 1.0
    assert float((lb._decision_packed(X) - lb._decision_loop(X)).abs().max()) <= 1e-12
