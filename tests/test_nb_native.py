"""Native naive Bayes on the CPU: the torch mirror of csrc/nb.hip behind
``naive_bayes.train / predict(engine="native")``, its gloo form, the limits and the CLI."""
import numpy as np
import pytest
import torch

from harp_amd import cli
from harp_amd.models import naive_bayes as NB
from harp_amd.runtime.launcher import launch


def counts(n, d, C, seed=0):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, 8, (n, d), generator=g).double(), torch.randint(0, C, (n,), generator=g)


@pytest.mark.parametrize("n,d,C", [(1, 1, 1), (65, 3, 2), (300, 17, 5)])
def test_native_equals_torch_engine_on_the_mirror(n, d, C):
    X, y = counts(n, d, C, seed=n)
    nat, ref = NB.train(X, y, C, engine="native"), NB.train(X, y, C)
    for k in ref:  # integer counts: every fp64 sum is exact in either order
        assert torch.equal(nat[k], ref[k]), k
    lab = NB.predict(X, nat, engine="native")
    assert lab.dtype == torch.int64 and torch.equal(lab, NB.predict(X, ref))
    assert NB.predict(X[:0], nat, engine="native").shape == (0,)
    empty = NB.train(X[:0], y[:0], C, engine="native")
    assert not empty["featureSums"].any() and not empty["classCounts"].any()


def test_predict_tie_and_nan_rules():
    model = {"logTheta": torch.tensor([[float("nan")], [1.0], [1.0]], dtype=torch.float64),
             "logPrior": torch.zeros(3, dtype=torch.float64)}
    assert NB.predict(torch.ones(2, 1, dtype=torch.float64), model, engine="native").tolist() == [1, 1]
    model["logTheta"][:] = float("nan")
    assert NB.predict(torch.ones(2, 1, dtype=torch.float64), model, engine="native").tolist() == [0, 0]


def _worker(comm, shards):
    X, y = shards[comm.rank]
    return NB.train(X, y, 4, comm, engine="native")


def test_two_gloo_workers_one_empty_equal_one():
    X, y = counts(50, 6, 4)
    one = NB.train(X, y, 4, engine="native")
    for out in launch(_worker, 2, args=([(X, y), (X[:0], y[:0])],), timeout=300):
        for k in one:
            assert torch.equal(out[k], one[k]), k


def test_limits_and_engine_names():
    X, y = counts(70, 3, 65)
    with pytest.raises(ValueError, match="engine=\"torch\""):
        NB.train(X, y, 65, engine="native")
    with pytest.raises(ValueError, match="engine=\"torch\""):
        NB.train(X[:, ::2], y, 64, engine="native")  # column stride 2
    with pytest.raises(ValueError, match="engine"):
        NB.train(X, y, 65, engine="bogus")
    with pytest.raises(ValueError, match="engine"):
        NB.predict(X, {}, engine="bogus")
    y.clamp_(max=63)
    for wrong in (64, -1):
        y[5] = wrong
        with pytest.raises(ValueError, match="label outside"):
            NB.train(X, y, 64, engine="native")


def test_cli_daal_naive_native(tmp_path, capsys):
    X, y = counts(40, 5, 3)
    inp, tst, work = tmp_path / "in", tmp_path / "test", tmp_path / "out"
    for p, rows in ((inp, slice(0, 40)), (tst, slice(7, 19))):
        p.mkdir()
        np.savetxt(p / "block_1.csv", torch.cat([X, y[:, None].double()], 1)[rows].numpy(), delimiter=",", fmt="%.17g")
    assert cli.main(["daal", "naive", "1", "1", "0", "1", str(inp), str(work), "--engine", "native",
                     "--test-dir", str(tst), "--backend", "gloo"]) == 0
    capsys.readouterr()
    ref = NB.train(X, y, 3)
    assert np.array_equal(np.loadtxt(work / "naive_featureSums.csv", delimiter=",", ndmin=2), ref["featureSums"].numpy())
    assert np.array_equal(np.loadtxt(work / "naive_predictions.csv", delimiter=",").reshape(-1),
                          NB.predict(X[7:19], ref).double().numpy())
