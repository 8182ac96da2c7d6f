"""Native SVD on the CPU: the torch mirror of csrc/jsvd.hip behind ``stats.svd(engine="native")``
and ``stats.pca(method="svd", engine="native")``, its gloo form, the limits and the CLI.

Inputs, shared with tests/test_svd_gpu.py: seeded standard-normal blocks, a rank-d//2 block
``randn(3d, d//2) @ randn(d//2, d)``, and a column-graded square matrix ``B D`` (``B = I + 0.5 G /
|G|_2`` with unit columns, cond(B) about 2; ``D = 2^-k`` falling over 40 binades).

Bound: the project's 1e-12 on every invariant. The stopping rule leaves a normalised
off-diagonal of at most sqrt(128) 2^-53 = 1.3e-15 and rounding a few 1e-14 at d = 128; a dropped
row, a wrong partner or a stale read shows at 1e-3 or worse. All checks are sign-free.
"""
import numpy as np
import pytest
import torch

from harp_amd import cli
from harp_amd.models import stats as ST
from harp_amd.runtime.launcher import launch

TOL = 1e-12


def block(rows, d, seed=0):
    return torch.from_numpy(np.random.default_rng(seed).standard_normal((rows, d)))


def rank_deficient(d, seed=0):
    rng = np.random.default_rng(seed)
    return torch.from_numpy(rng.standard_normal((3 * d, d // 2)) @ rng.standard_normal((d // 2, d)))


def graded(d, seed=0):
    G = np.random.default_rng(seed).standard_normal((d, d))
    B = np.eye(d) + 0.5 * G / np.linalg.norm(G, 2)
    B /= np.linalg.norm(B, axis=0)
    return torch.from_numpy(B * 2.0 ** -np.round(40.0 * np.arange(d) / (d - 1)))


def check_factors(A, U, s, Vt, rank=None):
    """The invariants of A = U diag(s) V^T against numpy's singular values; U may be None."""
    A, s, Vt = (np.asarray(t.cpu() if torch.is_tensor(t) else t) for t in (A, s, Vt))
    d = A.shape[1]
    ref = np.linalg.svd(A, compute_uv=False)
    assert np.abs(s - ref).max() <= TOL * ref[0]
    assert (s[:-1] >= s[1:]).all()
    assert np.abs(Vt @ Vt.T - np.eye(d)).max() <= TOL
    if U is not None:
        U = np.asarray(U.cpu() if torch.is_tensor(U) else U)
        assert np.abs(U.T @ U - np.eye(d)).max() <= TOL
        assert np.linalg.norm((U * s) @ Vt - A) <= TOL * np.linalg.norm(A)
    if rank is not None:
        assert s[rank:].max() <= TOL * s[0]


def check_svd(X, out, rank=None):
    check_factors(X, out.get("leftSingularMatrix"), out["singularValues"], out["rightSingularMatrix"], rank)


@pytest.mark.parametrize("d", (1, 2, 7, 8, 9, 33, 65))
def test_native_engine_on_the_cpu(d):
    X = block(2 * d + 3, d, seed=d)
    check_svd(X, ST.svd(X, engine="native"))
    out = ST.svd(X, want_u=False, engine="native")
    assert "leftSingularMatrix" not in out
    check_svd(X, out)


def test_rank_deficient_block():
    X = rank_deficient(33)
    check_svd(X, ST.svd(X, engine="native"), rank=16)


def _worker(comm, shards):
    out = ST.svd(shards[comm.rank], comm, engine="native")
    return out["leftSingularMatrix"], out["singularValues"], out["rightSingularMatrix"]


def test_two_gloo_workers_equal_one():
    X = block(40, 9)
    one = ST.svd(X, engine="native")
    res = launch(_worker, 2, args=([X[:13], X[13:]],), timeout=300)
    for _, s, Vt in res:
        assert torch.equal(s, res[0][1]) and torch.equal(Vt, res[0][2])
        assert (s - one["singularValues"]).abs().max() <= TOL * s[0]
    check_factors(X, torch.cat([r[0] for r in res]), res[0][1], res[0][2])


def test_pca_svd_method_engines_agree():
    X = block(200, 9)
    nat, ref = ST.pca(X, method="svd", engine="native"), ST.pca(X, method="svd", engine="torch")
    ev, V = ref["eigenvalues"], nat["eigenvectors"]
    assert ((nat["eigenvalues"] - ev).abs() <= TOL * ev).all()
    assert (V @ V.T - torch.eye(9, dtype=torch.float64)).abs().max() <= TOL


def test_limits_and_engine_names():
    with pytest.raises(ValueError, match="torch"):
        ST.svd(torch.zeros((300, 129), dtype=torch.float64), engine="native")
    with pytest.raises(ValueError, match="torch"):
        ST.svd(torch.ones((5, 7), dtype=torch.float64), engine="native")
    with pytest.raises(ValueError, match="engine"):
        ST.svd(block(20, 3), engine="lapack")
    with pytest.raises(ValueError, match="engine"):
        ST.pca(block(20, 3), method="svd", engine="lapack")


def test_cli_daal_svd_native(tmp_path, capsys):
    X = block(30, 7)
    inp = tmp_path / "in"
    inp.mkdir()
    np.savetxt(inp / "block_1.csv", X.numpy(), delimiter=",", fmt="%.17g")
    work = tmp_path / "out"
    assert cli.main(["daal", "svd", "1", "1", "0", "1", str(inp), str(work), "--engine", "native",
                     "--backend", "gloo"]) == 0
    capsys.readouterr()
    U, s, Vt = (np.loadtxt(work / f"svd_{k}.csv", delimiter=",", ndmin=2)
                for k in ("leftSingularMatrix", "singularValues", "rightSingularMatrix"))
    check_factors(X, U, s.reshape(-1), Vt)
