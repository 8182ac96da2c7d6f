"""The native optimization-solver engine on the CPU: ``engine="native"`` on CPU tensors runs the torch
formulas (the gloo path), so it must equal the torch engine bit for bit; the limits raise; ``daal
optim`` / ``daal mse`` round-trip through the CLI; row shards follow the one-worker trajectory. The
kernels themselves are checked in test_optim_gpu.py."""
import json

import numpy as np
import pytest
import torch

from harp_amd import cli
from harp_amd.models import optim as OP
from harp_amd.ops import glm as GL
from harp_amd.runtime.launcher import launch
from harp_amd.utils import datasets as DS

from tests.test_reference_fixtures import golden

OBJECTIVES = {"mse": OP.MSE, "logistic": OP.LogisticLoss}


def block(n=120, d=5, seed=1):
    g = torch.Generator().manual_seed(seed)
    X = torch.randn(n, d, generator=g, dtype=torch.float64)
    w = torch.randn(d, generator=g, dtype=torch.float64)
    return X, X @ w + 0.5, (X @ w > 0).double(), torch.randint(0, 3, (n,), generator=g)


@pytest.mark.parametrize("kind", ("mse", "logistic", "cross_entropy"))
def test_native_on_cpu_is_the_torch_engine(kind):
    X, yr, yb, yc = block()
    if kind == "cross_entropy":
        make = lambda e: OP.CrossEntropyLoss(X, yc, 3, l2=0.01, engine=e)  # noqa: E731
    else:
        make = lambda e: OBJECTIVES[kind](X, yr if kind == "mse" else yb, l2=0.01, engine=e)  # noqa: E731
    a, b = make("torch"), make("native")
    x = torch.linspace(-1, 1, a.dim, dtype=torch.float64)
    for idx in (None, torch.tensor([3, 3, 119, 0])):
        for p, q in zip(a.value_grad(x, idx), b.value_grad(x, idx)):
            assert torch.equal(p, q)
    for solver, kw in ((OP.sgd, dict(batch_size=4, momentum=0.5, learning_rate=0.05)),
                       (OP.adagrad, dict(batch_size=2)), (OP.lbfgs, dict(n_iterations=5))):
        kw = dict(dict(n_iterations=20, seed=3), **kw)
        ra, rb = solver(a, **kw), solver(b, **kw)
        assert torch.equal(ra.minimum, rb.minimum) and ra.n_iterations == rb.n_iterations and ra.value == rb.value


def test_bad_engine_and_limits():
    X, yr, _, yc = block(8, 3)
    with pytest.raises(ValueError, match="engine"):
        OP.MSE(X, yr, engine="hip")
    with pytest.raises(ValueError, match="engine"):
        OP.CrossEntropyLoss(X, yc, 3, engine="")
    wide = torch.zeros(2, GL.MAX_D + 1)
    with pytest.raises(ValueError, match=str(GL.MAX_D)):
        OP.LogisticLoss(wide, torch.zeros(2), engine="native")
    with pytest.raises(ValueError, match=str(GL.CE_MAX_D)):
        OP.CrossEntropyLoss(wide[:, :GL.CE_MAX_D + 1], torch.zeros(2), 3, engine="native")
    with pytest.raises(ValueError, match=str(GL.CE_MAX_K)):
        OP.CrossEntropyLoss(X, yc, GL.CE_MAX_K + 1, engine="native")
    with pytest.raises(ValueError, match=str(GL.SOLVER_MAX_BATCH)):
        GL.check_run("mse", 3, True, GL.SOLVER_MAX_BATCH + 1)
    OP.MSE(wide, torch.zeros(2))  # the torch engine has no limit


@pytest.mark.parametrize("engine", ("torch", "native"))
def test_cli_daal_optim_and_mse(tmp_path, capsys, engine):
    A = DS.load_dense_csv(golden("daal_optimization_solvers", "mse", "train", "mse.csv"))
    inp = golden("daal_optimization_solvers", "mse", "train")
    point = [8.0, 2.0, 1.0, 4.0]  # MSEDenseBatch's argument
    v, g = OP.MSE(A[:, :-1], A[:, -1]).value_grad(torch.tensor(point, dtype=torch.float64))
    assert cli.main(["daal", "mse", "1", "1", "0", "1", inp, str(tmp_path), "--engine", engine, "--backend", "gloo",
                     "--point", ",".join(map(str, point))]) == 0
    res = json.loads(capsys.readouterr().out.strip().splitlines()[-1])["result"]
    assert res["point_value"] == float(v) and res["point_gradient"] == g.tolist()
    assert np.array_equal(np.loadtxt(tmp_path / "mse_gradient.csv", delimiter=","), g.numpy())
    for solver, ref in (("minibatch", lambda o: OP.sgd(o, None, 50, 0.5, 4, 1e-7, seed=0)),
                        ("adagrad", lambda o: OP.adagrad(o, None, 50, 1.0, 1, accuracy_threshold=1e-7, seed=0))):
        assert cli.main(["daal", "optim", "1", "1", "0", "1", inp, str(tmp_path), "--solver", solver, "--iterations",
                         "50", "--engine", engine, "--backend", "gloo"]) == 0
        capsys.readouterr()
        r = ref(OP.MSE(A[:, :-1], A[:, -1]))
        assert np.array_equal(np.loadtxt(tmp_path / "optim_minimum.csv", delimiter=","), r.minimum.numpy())
        assert int(np.loadtxt(tmp_path / "optim_nIterations.csv")) == r.n_iterations


def test_cli_daal_optim_lbfgs(tmp_path, capsys):
    A = DS.load_dense_csv(golden("daal_optimization_solvers", "lbfgs", "train", "lbfgs.csv"))
    assert cli.main(["daal", "optim", "1", "1", "0", "1", golden("daal_optimization_solvers", "lbfgs", "train"),
                     str(tmp_path), "--solver", "lbfgs", "--iterations", "30", "--engine", "native", "--backend",
                     "gloo"]) == 0
    capsys.readouterr()
    r = OP.lbfgs(OP.MSE(A[:, :-1], A[:, -1]), None, 30, accuracy_threshold=1e-7)
    x = np.loadtxt(tmp_path / "optim_minimum.csv", delimiter=",")
    assert np.array_equal(x, r.minimum.numpy())
    # the fixture is an exact linear model: the minimum reproduces the targets
    assert np.abs(A[:, :-1].numpy() @ x[1:] + x[0] - A[:, -1].numpy()).max() < 1e-3 * A[:, -1].abs().max()


def _shard_sgd(comm, shards, idx):
    X, y = shards[comm.rank]
    return OP.sgd(OP.LogisticLoss(X, y, comm, l2=0.01, engine="native"), n_iterations=30, learning_rate=0.2,
                  batch_indices=idx).minimum


def test_sharded_sgd_equals_one_worker():
    X, _, yb, _ = block(80, 6, seed=5)
    idx = [[1, 7, 39], [0, 0, 12], [38, 2, 5]]  # local rows of each worker's 40-row shard
    both = [i + [40 + j for j in i] for i in idx]  # the same steps on the concatenated rows
    ref = OP.sgd(OP.LogisticLoss(X, yb, l2=0.01), n_iterations=30, learning_rate=0.2, batch_indices=both).minimum
    for x in launch(_shard_sgd, 2, args=([(X[:40], yb[:40]), (X[40:], yb[40:])], idx), timeout=300):
        assert float((x - ref).abs().max()) <= 1e-12 * float(ref.abs().max())
