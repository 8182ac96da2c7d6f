"""Native fp64 EM-GMM on the CPU: the torch mirror of csrc/gmm_f64.hip behind ``engine="native"``,
the limits, the unchanged ``engine="auto"``, gloo row shards and the ``daal em`` CLI."""
import numpy as np
import pytest
import torch

from harp_amd import cli
from harp_amd.models import kernels as KM
from harp_amd.runtime.launcher import launch


def blobs(n=600, seed=5):
    """The two clusters of test_em_gmm_matches_sklearn's setup."""
    g = torch.Generator().manual_seed(seed)
    A = torch.randn(n // 2, 2, generator=g, dtype=torch.float64) * 0.3 + torch.tensor([2.0, 0.0], dtype=torch.float64)
    B = torch.randn(n // 2, 2, generator=g, dtype=torch.float64) @ torch.tensor([[0.5, 0.2], [0.0, 0.3]],
                                                                               dtype=torch.float64) - 1
    return torch.cat([A, B])[torch.randperm(n, generator=g)]


def close(a, b, tol):
    return all(torch.allclose(a[k], b[k], rtol=tol, atol=tol) for k in ("weights", "means", "covariances", "loglik"))


@pytest.mark.parametrize("kind,dtype", [("full", torch.float64), ("diag", torch.float64), ("full", torch.float32)])
def test_native_mirror_equals_torch(kind, dtype):
    X = blobs().to(dtype)
    kw = dict(n_iterations=20, accuracy_threshold=0, covariance=kind, seed=3)
    a, b = KM.em_gmm(X, 3, engine="native", **kw), KM.em_gmm(X, 3, engine="torch", **kw)
    assert a["n_iterations"] == b["n_iterations"] == 20 and close(a, b, 1e-10)
    assert torch.equal(KM.gmm_predict(X, a, engine="native"), KM.gmm_predict(X, a, engine="torch"))
    assert torch.equal(KM.gmm_predict(X.t().contiguous().t(), a, engine="native"), KM.gmm_predict(X, a))


def test_limits_and_engine_names():
    X = blobs(80)
    with pytest.raises(ValueError, match="engine"):
        KM.em_gmm(X, 2, engine="bogus")
    with pytest.raises(ValueError, match="engine"):
        KM.gmm_predict(X, {}, engine="bogus")
    with pytest.raises(ValueError, match="64 columns.*engine=\"auto\""):
        KM.em_gmm(torch.zeros(80, 65, dtype=torch.float64), 2, engine="native")
    with pytest.raises(ValueError, match="1024 components.*engine=\"auto\""):
        KM.em_gmm(X, 1025, engine="native")
    with pytest.raises(ValueError, match="sparse.*engine=\"auto\""):
        KM.em_gmm(X.to_sparse_csr(), 2, engine="native")


def test_auto_is_unchanged():
    """engine="auto" is the call of test_em_gmm_matches_sklearn, to the bit, with and without the
    keyword; engine="torch" is estep="torch"."""
    X = blobs()
    kw = dict(n_iterations=300, accuracy_threshold=1e-10, reg=1e-6)
    ref = KM.em_gmm(X, 2, **kw)
    for other in (KM.em_gmm(X, 2, engine="auto", **kw), KM.em_gmm(X, 2, estep="torch", **kw),
                  KM.em_gmm(X, 2, engine="torch", **kw)):
        assert other["n_iterations"] == ref["n_iterations"] and close(other, ref, 0.0)
    assert ref["n_iterations"] < 300 and ref["means"].shape == (2, 2)


def _worker(comm, X, init):
    shard = X if comm.rank == 1 else X[:0]  # rank 0 holds no rows
    return KM.em_gmm(shard, 2, comm, n_iterations=15, accuracy_threshold=0, init=init, engine="native")


def test_two_gloo_workers_with_an_empty_shard_equal_one():
    X = blobs(200)
    init = {"weights": torch.tensor([0.5, 0.5], dtype=torch.float64), "means": X[:2].clone(),
            "covariances": torch.eye(2, dtype=torch.float64).expand(2, 2, 2).clone()}
    one = KM.em_gmm(X, 2, n_iterations=15, accuracy_threshold=0, init=init, engine="native")
    for out in launch(_worker, 2, args=(X, init), timeout=300):
        assert close(out, one, 1e-9)


@pytest.mark.parametrize("kind", ["full", "diag"])
def test_cli_daal_em_round_trip(tmp_path, kind):
    X = blobs(200)
    inp = tmp_path / "in"
    inp.mkdir()
    np.savetxt(inp / "block_1.csv", X.numpy(), delimiter=",", fmt="%.17g")
    direct = KM.em_gmm(X, 2, n_iterations=12, accuracy_threshold=0.0, covariance=kind, seed=4, engine="native")
    got = {}
    for engine in ("native", "torch"):
        work = tmp_path / engine
        assert cli.main(["daal", "em", "1", "1", "0", "12", str(inp), str(work), "--k", "2", "--method", kind,
                         "--accuracy-threshold", "0", "--seed", "4", "--engine", engine, "--backend", "gloo"]) == 0
        got[engine] = {k: np.loadtxt(work / f"em_{k}.csv", delimiter=",", ndmin=2)
                       for k in ("weights", "means", "covariances", "loglik", "nIterations")}
    nat = got["native"]
    assert nat["covariances"].shape == ((4, 2) if kind == "full" else (2, 2)) and nat["nIterations"].item() == 12
    for k, v in nat.items():
        assert np.allclose(v, got["torch"][k], rtol=1e-10, atol=1e-10)
    assert np.array_equal(nat["means"], direct["means"].numpy())
    assert np.array_equal(nat["covariances"], direct["covariances"].reshape(-1, 2).numpy())
    assert np.array_equal(nat["weights"].reshape(-1), direct["weights"].numpy())
    assert nat["loglik"].item() == float(direct["loglik"])
