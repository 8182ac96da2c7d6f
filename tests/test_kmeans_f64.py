"""engine="native" of the dense fp64 K-means on CPU tensors: the torch formula with the direct
objective, so it has to reproduce engine="torch"."""
import os

import numpy as np
import pytest
import torch

from harp_amd import cli
from harp_amd.models import kmeans_csr as M
from harp_amd.ops import kmeans_f64 as KF


def _blobs(n, d, k, seed):
    """Quarter-integer rows: every cluster sum is exact whatever its order, so index_add_ and
    the torch engine's one-hot GEMM give the same bits."""
    g = torch.Generator().manual_seed(seed)
    centres = torch.randint(0, 40, (k, d), generator=g).double()
    return centres[torch.randint(0, k, (n,), generator=g)] + torch.randint(-8, 9, (n, d), generator=g) / 4.0


def test_native_on_cpu_equals_torch_engine():
    X = _blobs(500, 7, 5, 0)
    C0 = X[:5].clone()
    ref = M.kmeans_sparse(X, C0, 4)
    out = M.kmeans_sparse(X, C0, 4, engine="native")
    assert torch.equal(out["centroids"], ref["centroids"]) and torch.equal(out["labels"], ref["labels"])
    assert all(abs(a - b) <= 1e-12 * abs(b) for a, b in zip(out["objective"], ref["objective"]))
    assert sorted(out) == sorted(ref)


def test_bad_engine_and_width_raise():
    X = torch.zeros(4, KF.MAX_D + 1)
    with pytest.raises(ValueError, match="engine"):
        M.kmeans_sparse(X[:, :3], X[:2, :3].double(), 1, engine="hip")
    with pytest.raises(ValueError, match="engine=\"torch\""):
        M.kmeans_sparse(X, X[:2].double(), 1, engine="native")


def test_cli_engines_write_the_same_centroids(tmp_path, capsys):
    os.makedirs(tmp_path / "in")
    np.savetxt(tmp_path / "in" / "part0.csv", _blobs(200, 6, 4, 1).numpy(), delimiter=",")
    for engine in ("native", "torch"):
        assert cli.main(["daal", "kmeans", "1", "1", "0", "3", str(tmp_path / "in"), str(tmp_path / engine),
                         "--k", "4", "--engine", engine, "--backend", "gloo"]) == 0
        capsys.readouterr()
    a, b = (open(tmp_path / e / "kmeans_centroids.csv").read() for e in ("native", "torch"))
    assert a == b and len(a.splitlines()) == 4
