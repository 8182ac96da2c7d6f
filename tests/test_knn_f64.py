"""Native fp64 kNN on the CPU: the torch mirror of csrc/knn_f64.hip behind ``engine="native"``,
the limits, the unchanged ``engine="auto"``, the gloo classifier and the CLI."""
import numpy as np
import pytest
import torch

from harp_amd import cli
from harp_amd.models import kernels as KM
from harp_amd.ops import knn as knn_ops
from harp_amd.runtime.launcher import launch


def ints(n, d, seed):
    return torch.randint(0, 16, (n, d), generator=torch.Generator().manual_seed(seed)).double()


def clusters(n, seed):
    g = torch.Generator().manual_seed(seed)
    y = torch.randint(0, 4, (n,), generator=g)
    return 20.0 * torch.eye(4, 6, dtype=torch.float64)[y] + torch.randn(n, 6, dtype=torch.float64, generator=g), y


@pytest.mark.parametrize("N,d,k,dtype", [(3, 1, 5, torch.float64), (300, 2, 32, torch.float32), (70, 33, 9, torch.bfloat16)])
def test_native_mirror_equals_stable_sort(N, d, k, dtype):
    T, Q = ints(N, d, N).to(dtype), ints(41, d, k).to(dtype)
    D = ((Q.double()[:, None, :] - T.double()[None, :, :]) ** 2).sum(-1)
    rd, ri = D.sort(dim=1, stable=True)
    dist, idx = KM.knn_search(T, Q, k, engine="native")
    assert dist.dtype == torch.float64 and idx.dtype == torch.int64
    assert torch.equal(dist, rd[:, :k]) and torch.equal(idx, ri[:, :k])


def test_limits_and_engine_names():
    T = ints(40, 257, 0)
    with pytest.raises(ValueError, match="256 columns"):
        KM.knn_search(T, T, 3, engine="native")
    with pytest.raises(ValueError, match="k <= 32"):
        KM.knn_search(T[:, :8], T[:, :8], 33, engine="native")
    with pytest.raises(ValueError, match="sparse"):
        KM.knn_search(T[:, :8].to_sparse_csr(), T[:, :8], 3, engine="native")
    with pytest.raises(ValueError, match="engine"):
        KM.knn_search(T, T, 3, engine="bogus")
    with pytest.raises(ValueError, match="engine"):
        KM.KNNClassifier(3, engine="bogus")


def test_auto_is_unchanged():
    T, Q = torch.randn(200, 7, generator=torch.Generator().manual_seed(1)), torch.randn(30, 7)
    for got, ref in zip(KM.knn_search(T, Q, 6), knn_ops.knn_search(T, Q, 6)):
        assert torch.equal(got, ref)
    for got, ref in zip(KM.knn_search(T, Q, 6, engine="torch"), knn_ops.knn_search(T, Q, 6)):
        assert torch.equal(got, ref)


def _worker(comm, X, y, Q):
    half = slice(comm.rank * 100, (comm.rank + 1) * 100)
    return KM.KNNClassifier(5, comm, engine="native").fit(X[half], y[half], num_classes=4).predict(Q)


def test_two_gloo_workers_equal_one():
    (X, y), (Q, _) = clusters(200, 0), clusters(50, 1)
    one = KM.KNNClassifier(5, engine="native").fit(X, y, num_classes=4).predict(Q)
    for out in launch(_worker, 2, args=(X, y, Q), timeout=300):
        assert torch.equal(out, one)


def test_cli_daal_knn_engines_agree(tmp_path, capsys):
    (X, y), (Q, yq) = clusters(120, 2), clusters(30, 3)
    inp, tst = tmp_path / "in", tmp_path / "test"
    for p, rows, lab in ((inp, X, y), (tst, Q, yq)):
        p.mkdir()
        np.savetxt(p / "block_1.csv", torch.cat([rows, lab[:, None].double()], 1).numpy(), delimiter=",", fmt="%.17g")
    pred = {}
    for engine in ("native", "torch"):
        work = tmp_path / engine
        assert cli.main(["daal", "knn", "1", "1", "0", "1", str(inp), str(work), "--k", "5", "--engine", engine,
                         "--test-dir", str(tst), "--backend", "gloo"]) == 0
        assert "knn accuracy: 1.000000" in capsys.readouterr().out
        pred[engine] = np.loadtxt(work / "knn_predictions.csv", delimiter=",").reshape(-1)
        assert float(np.loadtxt(work / "knn_accuracy.csv", delimiter=",")) == 1.0
    assert np.array_equal(pred["native"], pred["torch"]) and np.array_equal(pred["native"], yq.double().numpy())
