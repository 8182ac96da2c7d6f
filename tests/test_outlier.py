"""Native outlier detection on the CPU (the fp64 torch mirror of csrc/outlier.hip in
ops/outlier.py; the kernels are checked against it in test_outlier_gpu.py): the three detectors
take ``engine="native"`` and give the torch engine's weights, BACON runs on row shards with one
all-reduce per pass and no row gather, and ``daal outlier`` round-trips through the CLI.

Exact mask comparison needs a margin: two engines that compute a distance in two ways may put a
row that lies on a threshold on different sides. Every BACON test therefore first asserts, from
the native run's own models, that no row lies within relative 1e-9 of any pass's threshold and
that the m-th and (m + 1)-th initial distances differ by more than that; then all rows are
compared, none left out. The seeds below satisfy the assertion."""
import json
import os

import numpy as np
import pytest
import torch
from scipy.stats import chi2

from harp_amd import cli
from harp_amd.models import stats as ST
from harp_amd.ops import outlier as OL
from harp_amd.ops import quantile as QT
from harp_amd.runtime.launcher import launch
from harp_amd.utils import datasets as DS

from tests.test_reference_fixtures import golden

DTYPES = (torch.bfloat16, torch.float32, torch.float64)
MARGIN = 1e-9


def fixture_block() -> torch.Tensor:
    return DS.load_dense_csv(golden("daal_outlier", "train", "outlierdetection.csv"))


def planted_block() -> torch.Tensor:
    """The 200 + 5 block of test_partial_results.py, from a generator of its own."""
    g = torch.Generator().manual_seed(7)
    return torch.cat([torch.randn(200, 3, generator=g, dtype=torch.float64),
                      torch.full((5, 3), 25.0, dtype=torch.float64)])


def wide_block(n=600, d=7, seed=3, dtype=torch.float64) -> torch.Tensor:
    g = torch.Generator().manual_seed(seed)
    X = torch.randn(n, d, generator=g, dtype=torch.float64) @ torch.randn(d, d, generator=g, dtype=torch.float64)
    X[::50] += 40.0
    return X.to(dtype)


def assert_margin(X: torch.Tensor, trace, m: int) -> None:
    """No row of X within relative MARGIN of a pass's threshold; the initial subset is cut
    between two distances further apart than that."""
    assert len(trace) >= 2
    for i, (center, P, t2, strict) in enumerate(trace):
        d2 = OL.reference_pass(X.cpu(), center.cpu(), None if P is None else P.cpu(), t2, center.cpu(),
                               want_dist=True, want_stats=False)["dist2"]
        if i == 0:
            s = torch.sort(d2).values
            assert float(s[m - 1]) == t2
            assert m == len(s) or float(s[m] - s[m - 1]) > MARGIN * float(s[m]), "tie at the initial cut"
            assert m == 1 or float(s[m - 1] - s[m - 2]) > MARGIN * float(s[m - 1]), "tie at the initial cut"
        else:
            gap = float(((d2 - t2).abs() / t2).min())
            assert gap > MARGIN, f"pass {i}: a row lies {gap:.2e} (relative) from the threshold"


def native_bacon(X, **kw):
    trace = []
    out = ST.bacon_native(X, trace=trace, **kw)
    n, p = X.shape
    assert_margin(X, trace, min(n, max(4 * p, p + 1)))
    return out


# ------------------------------------------------------------------ the engine keyword
def test_engine_keyword():
    X = planted_block()
    for fn in (ST.outliers_univariate, ST.outliers_multivariate, ST.outliers_bacon):
        w = fn(X, engine="native")
        assert w.dtype == X.dtype and w.shape[0] == X.shape[0]
        assert torch.equal(fn(X), fn(X, engine="torch"))
        with pytest.raises(ValueError, match="engine"):
            fn(X, engine="triton")


def test_width_limit():
    X = torch.randn(300, 65, generator=torch.Generator().manual_seed(0), dtype=torch.float64)
    for fn in (ST.outliers_univariate, ST.outliers_multivariate, ST.outliers_bacon):
        with pytest.raises(ValueError, match="64"):
            fn(X, engine="native")
    assert ST.outliers_univariate(X).shape == X.shape  # the torch engine has no limit


# ------------------------------------------------------------------ univariate
@pytest.mark.parametrize("dtype", DTYPES, ids=("bf16", "fp32", "fp64"))
def test_univariate_equals_torch_on_special_values(dtype):
    g = torch.Generator().manual_seed(11)
    X = (torch.randn(257, 6, generator=g, dtype=torch.float64) * 3).to(dtype)
    X[3, 0], X[4, 1], X[5, 2] = float("nan"), float("inf"), float("-inf")
    X[6, 3], X[7, 3] = 0.0, -0.0
    X[:, 4] = 1.5  # zero scatter: every |x - loc| / 1e-300 is 0 / tiny or huge
    X[9, 4] = 1.25
    loc = X.double().nan_to_num(0, 0, 0).mean(0)
    sc = X.double().nan_to_num(0, 0, 0).std(0)
    sc[4] = 0.0
    for thr in (0.0, 1.0, 3.0):
        ref = ST.outliers_univariate(X, thr, init="given", location=loc, scatter=sc)
        got = ST.outliers_univariate(X, thr, init="given", location=loc, scatter=sc, engine="native")
        assert got.dtype == dtype and torch.equal(got, ref)
    assert torch.equal(ST.outliers_univariate(X, init="default", engine="native"),
                       ST.outliers_univariate(X, init="default"))
    Xc = wide_block(300, 5, dtype=dtype)
    assert torch.equal(ST.outliers_univariate(Xc, engine="native"), ST.outliers_univariate(Xc))


# ------------------------------------------------------------------ the pass and its pieces
def test_model_from_stats_is_torch_cov():
    X = wide_block(500, 6)
    member = torch.rand(500, generator=torch.Generator().manual_seed(1)) < 0.7
    c = X[member].mean(0) + 0.01
    P = OL.whiten(torch.cov(X[member].t()))
    d2 = OL.reference_pass(X, c, P, 0.0, c, want_dist=True, want_stats=False)["dist2"]
    t2 = float(torch.sort(d2).values[349:351].mean())
    mask = torch.zeros(500, dtype=torch.uint8)
    out = OL.mahalanobis_pass(X, c, P, t2, c, mask=mask)
    assert int(out["count"]) == 350 == int(mask.sum()) == int(out["changed"])
    mean, cov = OL.model_from_stats(out["record"], c)
    sub = X[mask.bool()]
    assert torch.allclose(mean, sub.mean(0), rtol=1e-12, atol=1e-12)
    assert torch.allclose(cov, torch.cov(sub.t()), rtol=1e-10, atol=1e-12)
    again = OL.mahalanobis_pass(X, c, P, t2, c, mask=mask)
    assert int(again["changed"]) == 0 and torch.equal(again["record"][2:], out["record"][2:])
    # the squared distance is stats.mahalanobis_sq's
    ref = ST.mahalanobis_sq(X, c, torch.cov(X[member].t()))
    assert torch.allclose(d2, ref, rtol=1e-10, atol=0)


def test_pass_reads_a_strided_block_and_all_dtypes():
    W = wide_block(300, 12)
    for dtype in DTYPES:
        Wd = W.to(dtype)
        X = Wd[:, 2:9]
        c = X.double().mean(0)
        a = OL.mahalanobis_pass(X, c, None, 50.0, c, want_dist=True, strict=False)
        b = OL.mahalanobis_pass(X.contiguous(), c, None, 50.0, c, want_dist=True, strict=False)
        assert torch.equal(a["record"], b["record"]) and torch.equal(a["dist2"], b["dist2"])
        assert torch.equal(a["dist2"], ((X.double() - c) ** 2).sum(1))


# ------------------------------------------------------------------ BACON and multivariate
@pytest.mark.parametrize("init", ("median", "cov"))
@pytest.mark.parametrize("data", ("fixture", "planted", "wide"))
def test_bacon_equals_torch_engine(data, init):
    X = {"fixture": fixture_block, "planted": planted_block, "wide": wide_block}[data]()
    out = native_bacon(X, init=init)
    ref = ST.outliers_bacon(X, init=init)
    assert torch.equal(out["weights"], ref)
    assert torch.equal(ST.outliers_bacon(X, init=init, engine="native"), ref)
    if data == "planted":
        assert ref[-5:].sum() == 0 and ref[:200].mean() > 0.9
    if data == "fixture":
        assert {i for i in range(len(ref)) if ref[i] == 0} == {3, 11}


@pytest.mark.parametrize("dtype", DTYPES, ids=("bf16", "fp32", "fp64"))
def test_bacon_dtypes_and_iteration_cap(dtype):
    X = wide_block(400, 5, seed=5, dtype=dtype)
    out = native_bacon(X)
    assert out["weights"].dtype == dtype and torch.equal(out["weights"], ST.outliers_bacon(X))
    assert out["iterations"] >= 2
    capped = ST.bacon_native(X, max_iter=1)
    assert capped["iterations"] == 1
    assert torch.equal(capped["weights"], ST.outliers_bacon(X, max_iter=1))


@pytest.mark.parametrize("data", ("fixture", "planted", "wide"))
def test_multivariate_equals_torch_engine(data):
    X = {"fixture": fixture_block, "planted": planted_block, "wide": wide_block}[data]()
    for thr in (None, 5.0):
        r = ST.covariance(X)
        d2 = ST.mahalanobis_sq(X, r["mean"], r["covariance"])
        t = thr if thr is not None else float(chi2.ppf(0.999, X.shape[1]))
        assert float(((d2 - t).abs() / t).min()) > MARGIN
        assert torch.equal(ST.outliers_multivariate(X, thr, engine="native"), ST.outliers_multivariate(X, thr))


# ------------------------------------------------------------------ distributed
class _Hook:
    """Counts all-reduces; anything that gathers raises."""

    def __init__(self):
        self.allreduces = 0

    def __call__(self, op):
        if op == "all_reduce":
            self.allreduces += 1
        elif op != "barrier":
            raise AssertionError(f"collective {op} on the native BACON path")


def _boom(*a, **k):
    raise AssertionError("gather_rows on the native BACON path")


def _shard_worker(comm, shards):
    X = shards[comm.rank]
    hook = _Hook()
    saved = ST.gather_rows
    comm.fault_hook, ST.gather_rows = hook, _boom
    try:
        out = ST.bacon_native(X, comm=comm)
    finally:
        comm.fault_hook, ST.gather_rows = None, saved
    try:
        ST.outliers_bacon(X, comm=comm)
        refused = False
    except ValueError:
        refused = True
    multi = ST.outliers_multivariate(X, comm=comm, engine="native")
    return out["weights"], out["iterations"], hook.allreduces, refused, multi


@pytest.mark.parametrize("world", (2, 3))
def test_sharded_equals_single_process(world):
    for dtype in (torch.float32, torch.float64):
        X = wide_block(401, 4, seed=9, dtype=dtype)
        cuts = [0, 150, 150, 401] if world == 3 else [0, 401, 401]  # uneven, one shard empty
        shards = [X[cuts[r]:cuts[r + 1]] for r in range(world)]
        assert any(s.shape[0] == 0 for s in shards)
        ref = native_bacon(X)
        assert torch.equal(ref["weights"], ST.outliers_bacon(X))
        multi = ST.outliers_multivariate(X)
        # the median select, the select on the fp64 distances, the initial subset's pass and
        # one per iteration
        expect = QT.passes(dtype) + QT.passes(torch.float64) + 1 + ref["iterations"]
        for r, (w, its, allreduces, refused, mw) in enumerate(launch(_shard_worker, world, args=(shards,),
                                                                     timeout=300)):
            assert torch.equal(w, ref["weights"][cuts[r]:cuts[r + 1]])
            assert its == ref["iterations"] and allreduces == expect and refused
            assert torch.equal(mw, multi[cuts[r]:cuts[r + 1]])


# ------------------------------------------------------------------ CLI
@pytest.mark.parametrize("method", ("uni", "multi", "bacon"))
def test_cli_daal_outlier(tmp_path, capsys, method):
    X = wide_block(120, 4, seed=2).mul(100).round() / 100
    inp = tmp_path / "in"
    os.makedirs(inp)
    np.savetxt(inp / "block_1.csv", X.numpy(), delimiter=",", fmt="%.17g")
    fn = {"uni": ST.outliers_univariate, "multi": ST.outliers_multivariate, "bacon": ST.outliers_bacon}[method]
    ref = fn(X).numpy().reshape(120, -1)
    for engine in ("native", "torch"):
        work = tmp_path / f"out_{engine}"
        assert cli.main(["daal", "outlier", "1", "1", "0", "1", str(inp), str(work), "--method", method,
                         "--engine", engine, "--backend", "gloo"]) == 0
        assert json.loads(capsys.readouterr().out.strip().splitlines()[-1])["app"] == "daal"
        got = np.loadtxt(work / "outlier_weights.csv", delimiter=",").reshape(120, -1)
        assert np.array_equal(got, ref)
    if method == "bacon":
        work = tmp_path / "out_alpha"
        assert cli.main(["daal", "outlier", "1", "1", "0", "1", str(inp), str(work), "--method", "bacon",
                         "--alpha", "0.2", "--backend", "gloo"]) == 0
        capsys.readouterr()
        assert np.array_equal(np.loadtxt(work / "outlier_weights.csv", delimiter=","),
                              ST.outliers_bacon(X, alpha=0.2).numpy())
    if method == "uni":
        work = tmp_path / "out_thr"
        assert cli.main(["daal", "outlier", "1", "1", "0", "1", str(inp), str(work), "--method", "uni",
                         "--threshold", "1.5", "--backend", "gloo"]) == 0
        capsys.readouterr()
        assert np.array_equal(np.loadtxt(work / "outlier_weights.csv", delimiter=","),
                              ST.outliers_univariate(X, 1.5).numpy())


def test_cli_daal_outlier_on_two_workers(tmp_path, capsys):
    """Two workers, one file each: the weights file holds the workers' rows in rank order."""
    X = wide_block(160, 3, seed=4).mul(100).round() / 100
    inp = tmp_path / "in"
    os.makedirs(inp)
    np.savetxt(inp / "block_1.csv", X[:70].numpy(), delimiter=",", fmt="%.17g")
    np.savetxt(inp / "block_2.csv", X[70:].numpy(), delimiter=",", fmt="%.17g")
    work = tmp_path / "out"
    assert cli.main(["daal", "outlier", "2", "1", "0", "1", str(inp), str(work), "--method", "bacon",
                     "--backend", "gloo"]) == 0
    capsys.readouterr()
    got = np.loadtxt(work / "outlier_weights.csv", delimiter=",")
    ref = native_bacon(X)["weights"].numpy()
    assert got.shape == (160,) and got.sum() == ref.sum()
    halves = (np.concatenate([ref[:70], ref[70:]]), np.concatenate([ref[70:], ref[:70]]))
    assert any(np.array_equal(got, h) for h in halves)
