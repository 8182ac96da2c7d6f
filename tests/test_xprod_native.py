"""Native cross-products on the CPU: the torch mirror of csrc/xprod.hip behind ``engine="native"``
of the statistics and regression models, its gloo form, the limits and the CLI."""
import numpy as np
import pytest
import torch

from harp_amd import cli
from harp_amd.models import regression as RG
from harp_amd.models import stats as ST
from harp_amd.ops import linalg as LA
from harp_amd.ops import xprod as XP
from harp_amd.runtime.launcher import launch


def rows(n=301, d=7, seed=0):
    g = torch.Generator().manual_seed(seed)
    X = torch.randn(n, d, generator=g, dtype=torch.float64) * 3 + 10
    return X, X @ torch.randn(d, 2, generator=g, dtype=torch.float64) + torch.randn(n, 2, generator=g, dtype=torch.float64)


def within(a, b, n, scale):
    """|a - b| <= 4 n 2^-52 scale: both sides sum n terms of size <= scale, each within n u of it."""
    return bool(((a - b).abs() <= 4 * n * 2.0 ** -52 * scale).all())


def test_mirror_equals_the_fp64_engine_on_the_same_shift():
    X, _ = rows()
    n, s, xtx = ST._shifted_sums(X, torch.float64)
    r = XP.cross_products(X)
    big = (X.abs().t() @ X.abs()).max()
    assert r["n"].item() == n and within(r["sum"], s, 301, X.abs().sum(0)) and within(r["xtx"], xtx, 301, big)
    m = XP.col_moments(X)
    assert torch.equal(m["min"], X.min(0).values) and torch.equal(m["max"], X.max(0).values)
    assert within(m["sumsq"], (X * X).sum(0), 301, (X * X).sum(0)) and torch.equal(m["shift"], X[0])


def test_native_equals_torch_engine_at_fp64():
    X, y = rows()
    big = (X.abs().t() @ X.abs()).max() / 300
    a, b = ST.covariance(X, engine="native"), ST.covariance(X, dtype="fp64")
    assert within(a["covariance"], b["covariance"], 301, big) and within(a["mean"], b["mean"], 301, X.abs().max())
    a, b = ST.low_order_moments(X, engine="native"), ST.low_order_moments(X, dtype="fp64")
    for k in b:
        assert within(a[k], b[k], 301, b[k].abs()), k
    for ridge in (0.0, 1.0):  # the torch engine solves the unshifted system: both within its conditioning
        a, b = RG.train_linear(X, y, ridge=ridge, engine="native"), RG.train_linear(X, y, ridge=ridge)
        cond = torch.linalg.cond(LA.gram(RG._augment(X, y, True))[:8, :8].double())
        assert within(a["beta"], b["beta"], 301, cond * b["beta"].abs().max())
    a, b = ST.pca(X, engine="native"), ST.pca(X)
    assert within(a["eigenvalues"], b["eigenvalues"], 301, 1.0)


def _worker(comm, shards):
    X, y = shards[comm.rank]
    return {"cov": ST.covariance(X, comm, engine="native")["covariance"],
            "mom": ST.low_order_moments(X, comm, engine="native"),
            "beta": RG.train_linear(X, y, comm, engine="native")["beta"]}


def test_two_gloo_workers_one_empty_equal_one():
    X, y = rows(50, 6)
    one = {"cov": ST.covariance(X, engine="native")["covariance"], "mom": ST.low_order_moments(X, engine="native"),
           "beta": RG.train_linear(X, y, engine="native")["beta"]}
    for out in launch(_worker, 2, args=([(X, y), (X[:0], y[:0])],), timeout=300):
        assert torch.equal(out["cov"], one["cov"]) and torch.equal(out["beta"], one["beta"])
        for k in one["mom"]:
            assert torch.equal(out["mom"][k], one["mom"][k]), k


def test_limits_and_engine_names():
    X, y = rows(20, 6)
    wide = torch.zeros(4, 255, dtype=torch.float64)
    for call in (lambda: ST.covariance(torch.zeros(4, 257), engine="native"),
                 lambda: RG.train_linear(wide, torch.zeros(4, 2), engine="native"),       # d + m = 257
                 lambda: ST.covariance(X, dtype="bf16", engine="native"),
                 lambda: ST.low_order_moments(X, dtype="bf16", engine="native"),
                 lambda: ST.covariance(LA.FeatureMajor(torch.zeros(4, 128, 48, dtype=torch.bfloat16), 20, 6), engine="native"),
                 lambda: ST.correlation(X.to_sparse_csr(), engine="native"),
                 lambda: ST.covariance(X[:, ::2], engine="native"),                       # column stride 2
                 lambda: RG.train_linear(X, y, method="qr", engine="native")):
        with pytest.raises(ValueError, match="engine=\"torch\""):
            call()
    for call in (lambda: ST.covariance(X, engine="bogus"), lambda: ST.low_order_moments(X, engine="bogus"),
                 lambda: ST.pca(X, engine="bogus"), lambda: RG.train_linear(X, y, engine="bogus")):
        with pytest.raises(ValueError, match="engine"):
            call()
    assert ST.low_order_moments(torch.zeros(4, 300, dtype=torch.float64), engine="native")["sum"].shape == (300,)


@pytest.mark.parametrize("algo", ["cov", "linreg"])
def test_cli_daal_native(tmp_path, capsys, algo):
    X, y = rows(40, 5)
    inp, work = tmp_path / "in", tmp_path / "out"
    inp.mkdir()
    np.savetxt(inp / "block_1.csv", torch.cat([X, y[:, :1]], 1).numpy(), delimiter=",", fmt="%.17g")
    assert cli.main(["daal", algo, "1", "1", "0", "1", str(inp), str(work), "--engine", "native",
                     "--backend", "gloo"]) == 0
    capsys.readouterr()
    if algo == "cov":
        ref = ST.covariance(torch.cat([X, y[:, :1]], 1), engine="native")["covariance"]
        assert np.array_equal(np.loadtxt(work / "cov_covariance.csv", delimiter=",", ndmin=2), ref.numpy())
    else:
        ref = RG.train_linear(X, y[:, :1], engine="native")["beta"]
        assert np.array_equal(np.loadtxt(work / "linreg_beta.csv", delimiter=",", ndmin=2), ref.numpy())
