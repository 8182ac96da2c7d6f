"""Native pivoted QR on the CPU: the torch mirror of csrc/pqr.hip behind
``stats.pivoted_qr(engine="native")``, its gloo form, the limits and the CLI.

Two inputs, shared with tests/test_pqr_gpu.py:

* planted order: ``X[:, pi] = Q0 R0`` with ``diag R0 = g^k`` falling to 1e-6 and an upper part of
  at most 0.02 of its column's diagonal, so that every pivot wins by a clear margin (best to
  second-best residual norm >= 1.11) and LAPACK returns exactly ``pi``;
* rank-deficient: ``A[300, d//2] @ B[d//2, d]`` with column 3 zeroed and column 5 a copy of
  column 4.

Bounds: those of tests/test_reference_fixtures.py (1e-12 on the factorisation and on
orthonormality, 1e-10 on |diag R|).
"""
import numpy as np
import pytest
import scipy.linalg
import torch

from harp_amd import cli
from harp_amd.models import stats as ST
from harp_amd.ops import pqr as PQ
from harp_amd.runtime.launcher import launch

from tests.test_reference_fixtures import rel


def planted(d, n, seed=0):
    """(X [n, d], pi, the diagonal g^k)."""
    rng = np.random.default_rng(seed)
    pi = rng.permutation(d)
    Q0 = np.linalg.qr(rng.standard_normal((n, d)))[0]
    dg = (1e-6 ** (1.0 / max(d - 1, 1))) ** np.arange(d)
    R0 = np.triu(0.02 * rng.uniform(-1, 1, (d, d)) * dg[None, :], 1) + np.diag(dg)
    X = np.empty((n, d))
    X[:, pi] = Q0 @ R0
    return torch.from_numpy(X), pi, dg


def rank_deficient(d, seed=0):
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((300, d // 2)) @ rng.standard_normal((d // 2, d))
    X[:, 3] = 0.0
    X[:, 5] = X[:, 4]
    return torch.from_numpy(X)


def exact_ties(d, seed=0):
    """[d, d]: column j is 2^-(j mod 3) times a unit vector (a random permutation of the rows),
    column 3 zeroed and column 5 a copy of column 4. Every reflector is then a signed row swap
    or the identity and every entry stays a power of two or zero, so norms tie exactly, at the
    end at zero (tau = 0), in any order of summation: only the tie rule decides the pivots."""
    A = np.zeros((d, d))
    A[np.random.default_rng(seed).permutation(d), np.arange(d)] = 0.5 ** (np.arange(d) % 3)
    A[:, 3:4] = 0.0
    A[:, 5:6] = A[:, 4:5]
    return torch.from_numpy(A)


def check_invariants(X, out, rank=None):
    A = X.cpu().numpy()
    Q, R, perm = (out[k].cpu().numpy() for k in ("Q", "R", "permutation"))
    d = A.shape[1]
    assert out["permutation"].dtype == torch.int64 and sorted(perm.tolist()) == list(range(d))
    assert rel(Q @ R, A[:, perm]) <= 1e-12
    assert np.abs(Q.T @ Q - np.eye(d)).max() <= 1e-12
    assert np.abs(np.tril(R, -1)).max() == 0
    dg = np.diag(R)
    assert (dg >= 0).all()
    assert (dg[:-1] >= dg[1:] - 1e-12 * dg[0]).all()
    if rank is not None:
        assert np.abs(dg[rank:]).max() <= 1e-12 * np.linalg.norm(A)


def check_planted(X, pi, dg, out):
    assert np.array_equal(scipy.linalg.qr(X.cpu().numpy(), mode="r", pivoting=True)[1], pi)
    assert np.array_equal(out["permutation"].cpu().numpy(), pi)
    assert rel(np.diag(out["R"].cpu().numpy()), dg) <= 1e-10
    check_invariants(X, out)


@pytest.mark.parametrize("d", (7, 64, 65, 128))
def test_native_engine_on_the_cpu(d):
    X, pi, dg = planted(d, 257)
    check_planted(X, pi, dg, ST.pivoted_qr(X, engine="native"))
    X = rank_deficient(d)
    check_invariants(X, ST.pivoted_qr(X, engine="native"), rank=d // 2)


def _worker(comm, shards):
    out = ST.pivoted_qr(shards[comm.rank], comm, engine="native")
    return out["Q"], out["R"], out["permutation"]


def test_two_gloo_workers_equal_one():
    X, pi, _ = planted(9, 40)
    one = ST.pivoted_qr(X, engine="native")
    res = launch(_worker, 2, args=([X[:5], X[5:]],), timeout=300)  # the first shard has fewer rows than columns
    for Q, R, perm in res:
        assert torch.equal(R, res[0][1]) and torch.equal(perm, res[0][2])
        assert np.array_equal(perm.numpy(), pi) and torch.equal(perm, one["permutation"])
        assert rel(R, one["R"]) <= 1e-10
    Q = torch.cat([r[0] for r in res])
    assert Q.shape == (40, 9)
    assert (Q.T @ Q - torch.eye(9, dtype=torch.float64)).abs().max() <= 1e-12


def test_limits_name_the_host_engine():
    with pytest.raises(ValueError, match="host"):
        ST.pivoted_qr(torch.zeros((300, 129), dtype=torch.float64), engine="native")
    with pytest.raises(ValueError, match="host"):
        ST.pivoted_qr(torch.ones((5, 7), dtype=torch.float64), engine="native")
    with pytest.raises(ValueError, match="host"):
        PQ.check_width(129)
    with pytest.raises(ValueError):
        ST.pivoted_qr(torch.ones((7, 5), dtype=torch.float64), comm=object(), engine="host")


def test_host_engine_is_unchanged():
    X = rank_deficient(9)
    Q, R, piv = scipy.linalg.qr(X.numpy(), mode="economic", pivoting=True)
    for out in (ST.pivoted_qr(X), ST.pivoted_qr(X, engine="host")):
        assert np.array_equal(out["Q"].numpy(), Q) and np.array_equal(out["R"].numpy(), R)
        assert np.array_equal(out["permutation"].numpy(), piv) and out["Q"].device.type == "cpu"


@pytest.mark.parametrize("algo", ("pqr", "pivoted_qr"))
def test_cli_daal_pqr(tmp_path, capsys, algo):
    X, pi, dg = planted(7, 30)
    inp = tmp_path / "in"
    inp.mkdir()
    np.savetxt(inp / "block_1.csv", X.numpy(), delimiter=",", fmt="%.17g")
    work = tmp_path / "out"
    assert cli.main(["daal", algo, "1", "1", "0", "1", str(inp), str(work), "--engine", "native",
                     "--backend", "gloo"]) == 0
    capsys.readouterr()
    out = {k: torch.from_numpy(np.loadtxt(work / f"pqr_{k}.csv", delimiter=",", ndmin=2))
           for k in ("Q", "R", "permutation")}
    out["permutation"] = out["permutation"].reshape(-1).long()
    check_planted(X, pi, dg, out)
