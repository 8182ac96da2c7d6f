"""Sparse (CSR) statistics on the CPU: covariance, low-order moments, correlation PCA and
naive Bayes on CSR input equal the dense-input results without ever densifying the data
(ops/csr_stats.py references; the GPU kernels are checked in test_csr_stats_gpu.py)."""
import json
import os

import numpy as np
import pytest
import torch

from harp_amd import cli
from harp_amd.models import naive_bayes as NB
from harp_amd.models import stats as ST
from harp_amd.ops import csr_stats as CS
from harp_amd.runtime.launcher import launch

MOMENTS = ("minimum", "maximum", "sum", "sumSquares", "sumSquaresCentered", "mean", "secondOrderRawMoment",
           "variance", "standardDeviation", "variation")


def sparse_block(n, d, density, seed, counts=False):
    """Seeded operand: every 17th row empty, one fully dense row (more than 64 nonzeros in
    one feature block once d > 64). ``counts``: small non-negative integers (bag of words)."""
    g = torch.Generator().manual_seed(seed)
    X = torch.rand(n, d, generator=g, dtype=torch.float64) * 2.0 - 0.5
    if counts:
        X = torch.floor(X.abs() * 9.0) + 1.0
    keep = torch.rand(n, d, generator=g) < density
    keep[::17] = False
    if n > 5:
        keep[5, :] = True
    return X * keep


def rel(a, b) -> float:
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300))


@pytest.fixture
def no_densify(monkeypatch):
    def boom(self, *a, **k):
        raise AssertionError("to_dense called on a sparse statistics path")

    def arm():
        monkeypatch.setattr(torch.Tensor, "to_dense", boom)

    return arm


def _check_moments(got, ref):
    for k in MOMENTS:
        assert rel(got[k], ref[k]) <= 1e-10, k


def _check_pca(got, ref):
    assert rel(got["eigenvalues"], ref["eigenvalues"]) <= 1e-10
    sign = torch.sign((got["eigenvectors"] * ref["eigenvectors"]).sum(1, keepdim=True))
    assert float((got["eigenvectors"] * sign - ref["eigenvectors"]).abs().max()) <= 1e-8


@pytest.mark.parametrize("layout", ["csr", "coo"])
def test_statistics_equal_dense_without_densifying(no_densify, layout):
    X = sparse_block(500, 70, 0.08, 0)
    ref_cov, ref_mom, ref_pca = ST.covariance(X), ST.low_order_moments(X), ST.pca(X)
    Xs = X.to_sparse_csr() if layout == "csr" else X.to_sparse()
    no_densify()
    cov = ST.covariance(Xs)
    assert rel(cov["covariance"], ref_cov["covariance"]) <= 1e-10 and rel(cov["mean"], ref_cov["mean"]) <= 1e-10
    _check_moments(ST.low_order_moments(Xs), ref_mom)
    _check_pca(ST.pca(Xs, method="correlation"), ref_pca)


def test_naive_bayes_exact_without_densifying(no_densify):
    X = sparse_block(600, 45, 0.15, 1, counts=True)
    y = torch.randint(0, 6, (600,), generator=torch.Generator().manual_seed(2))
    ref = NB.train(X, y, 6)
    ref_pred = NB.predict(X, ref)
    Xs = X.to_sparse_csr()
    no_densify()
    m = NB.train(Xs, y, 6)
    assert torch.equal(m["featureSums"], ref["featureSums"]) and torch.equal(m["classCounts"], ref["classCounts"])
    assert torch.equal(NB.predict(Xs, m), ref_pred)


def test_class_sums_rejects_bad_label():
    Xs = sparse_block(20, 5, 0.5, 3).to_sparse_csr()
    with pytest.raises(ValueError):
        CS.class_sums(Xs, torch.full((20,), 4), 4)


def test_unsorted_columns_give_the_same_result(no_densify):
    X = sparse_block(120, 33, 0.2, 4)
    Xs = X.to_sparse_csr()
    rp, ci, va = Xs.crow_indices(), Xs.col_indices().clone(), Xs.values().clone()
    for r in range(120):  # reverse every row's entries: same matrix, columns descending
        a, b = int(rp[r]), int(rp[r + 1])
        ci[a:b] = ci[a:b].flip(0)
        va[a:b] = va[a:b].flip(0)
    Xu = torch.sparse_csr_tensor(rp, ci, va, size=X.shape)
    ref = ST.covariance(X)
    ref_mom = ST.low_order_moments(X)
    no_densify()
    assert rel(ST.covariance(Xu)["covariance"], ref["covariance"]) <= 1e-10
    _check_moments(ST.low_order_moments(Xu), ref_mom)
    A = CS.to_csr_operand(Xu)
    assert CS._sorted_rows(A.rowptr, A.col) and CS.to_csr_operand(Xu) is A  # fixed once, cached


def test_references_from_csr_arrays():
    """The torch references themselves (the GPU tests' oracle) against dense formulas."""
    X = sparse_block(300, 2 * CS.GRAM_TILE + 1, 0.05, 5)
    A = CS.to_csr_operand(X.to_sparse_csr())
    assert rel(CS.gram_ref(A), torch.triu(X.t() @ X)) <= 1e-13
    G0 = torch.ones(A.d, A.d, dtype=torch.float64)
    assert rel(CS.gram(A, out=G0.clone()), torch.triu(X.t() @ X) + 1.0) <= 1e-13
    c = torch.rand(A.d, dtype=torch.float64)
    m = CS.with_implicit_zeros(CS.col_moments(A, c), A.n, c)
    assert rel(m["sum"], (X - c).sum(0)) <= 1e-12 and rel(m["sumsq"], ((X - c) ** 2).sum(0)) <= 1e-12
    assert torch.equal(m["min"], X.min(0).values) and torch.equal(m["max"], X.max(0).values)
    B = torch.rand(A.d, 7, dtype=torch.float64)
    b = torch.rand(7, dtype=torch.float64)
    assert rel(CS.spmm(A, B, b), X @ B + b) <= 1e-13
    assert torch.equal(CS.spmm(A, B, b, argmax=True), (X @ B + b).argmax(1))
    tie = torch.tensor([[1.0, 3.0, 3.0], [2.0, 2.0, 2.0]], dtype=torch.float64)
    assert CS._argmax_low(tie).tolist() == [1, 0]
    assert CS.gram_path(10 ** 6, 1000, 10 ** 6) == "direct" and CS.gram_path(10 ** 6, 1000, 5 * 10 ** 7) == "tiled"


def test_pca_svd_on_sparse_raises():
    with pytest.raises(ValueError, match="svd"):
        ST.pca(sparse_block(50, 6, 0.5, 6).to_sparse_csr(), method="svd")


def _two_rank_worker(comm, blocks):
    X = blocks[comm.rank].to_sparse_csr()
    cov = ST.covariance(X, comm)
    return {"cov": cov["covariance"], "mean": cov["mean"], "mom": ST.low_order_moments(X, comm),
            "pca": ST.pca(X, comm)}


def test_two_ranks_gloo():
    X = sparse_block(400, 30, 0.1, 7)
    blocks = [X[:150], X[150:]]  # uneven shards
    ref_cov, ref_mom, ref_pca = ST.covariance(X), ST.low_order_moments(X), ST.pca(X)
    for r in launch(_two_rank_worker, 2, args=(blocks,), timeout=300):
        assert rel(r["cov"], ref_cov["covariance"]) <= 1e-10 and rel(r["mean"], ref_cov["mean"]) <= 1e-10
        _check_moments(r["mom"], ref_mom)
        _check_pca(r["pca"], ref_pca)


def _write_daal_csr(path, X):
    """DAAL CSR text (1-based): row offsets, columns, values; as wide as its last used column."""
    Xs = X.to_sparse_csr()
    with open(path, "w") as f:
        f.write(",".join(str(int(v) + 1) for v in Xs.crow_indices()) + "\n")
        f.write(",".join(str(int(v) + 1) for v in Xs.col_indices()) + "\n")
        f.write(",".join(repr(float(v)) for v in Xs.values()) + "\n")


def test_cli_daal_cov_csr_round_trip(tmp_path, capsys):
    X = sparse_block(90, 12, 0.3, 8)
    X[:45, 9:] = 0.0  # the first file ends at column 9: the workers must agree on the width
    inp = tmp_path / "in"
    os.makedirs(inp)
    _write_daal_csr(inp / "block_1.csv", X[:45])
    _write_daal_csr(inp / "block_2.csv", X[45:])
    work = tmp_path / "out"
    assert cli.main(["daal", "cov", "2", "1", "0", "1", str(inp), str(work), "--format", "csr",
                     "--backend", "gloo"]) == 0
    assert json.loads(capsys.readouterr().out.strip().splitlines()[-1])["app"] == "daal"
    cov = np.loadtxt(work / "cov_covariance.csv", delimiter=",")
    assert rel(cov, np.cov(X.numpy(), rowvar=False)) <= 1e-10
    assert rel(np.loadtxt(work / "cov_mean.csv", delimiter=","), X.numpy().mean(0)) <= 1e-10
