"""Sparse kernel matrices and SVM on CSR input, CPU: kernel functions and the one-against-one
SVM on CSR / COO input equal the dense-input results without ever densifying the data
(ops/csr_kernel.py references; the GPU kernels are checked in test_csr_kernel_gpu.py)."""
import json
import os

import numpy as np
import pytest
import torch

from harp_amd import cli
from harp_amd.models import kernels as KF
from harp_amd.models import svm as SV
from harp_amd.ops import csr_kernel as CK
from tests.test_reference_fixtures import ROOT as REFERENCE_ROOT

REFERENCE = os.path.join(REFERENCE_ROOT, "daal_svm", "multicsr")  # the reference checkout's fixture, when present


def sparse_block(n, d, density, seed):
    """Seeded operand: every 17th row empty, one fully dense row."""
    g = torch.Generator().manual_seed(seed)
    X = torch.rand(n, d, generator=g, dtype=torch.float64) * 2.0 - 0.5
    keep = torch.rand(n, d, generator=g) < density
    keep[::17] = False
    if n > 5:
        keep[5, :] = True
    return X * keep


def integer_rows(n, d, classes, seed, per_row=6):
    """Integer-valued rows with a few nonzeros each, the class in the column pattern: every
    Gram entry is an exact integer whatever the order of the additions."""
    g = torch.Generator().manual_seed(seed)
    y = torch.randint(0, classes, (n,), generator=g)
    X = torch.zeros(n, d, dtype=torch.float64)
    span = d // classes
    for i in range(n):
        cols = int(y[i]) * span + torch.randperm(span, generator=g)[:per_row - 2]
        X[i, cols] = torch.randint(1, 6, (per_row - 2,), generator=g).double()
        X[i, torch.randint(0, d, (2,), generator=g)] = torch.randint(1, 4, (2,), generator=g).double()
    return X, y


def rel(a, b) -> float:
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300))


@pytest.fixture
def no_densify(monkeypatch):
    def boom(self, *a, **k):
        raise AssertionError("to_dense called on a sparse kernel path")

    def arm():
        monkeypatch.setattr(torch.Tensor, "to_dense", boom)

    return arm


@pytest.mark.parametrize("layout", ["csr", "coo"])
def test_kernel_functions_equal_dense_without_densifying(no_densify, layout):
    X, Y = sparse_block(300, 70, 0.08, 0), sparse_block(130, 70, 0.08, 1)
    ref = {"lin": KF.linear_kernel(X, Y, 0.5, 2.0), "sq": KF.sq_distances(X, Y), "rbf": KF.rbf_kernel(X, Y, 1.7),
           "self": KF.rbf_kernel(X, X, 0.9)}
    conv = (lambda A: A.to_sparse_csr()) if layout == "csr" else (lambda A: A.to_sparse())
    Xs, Ys = conv(X), conv(Y)
    no_densify()
    got = {"lin": KF.linear_kernel(Xs, Ys, 0.5, 2.0), "sq": KF.sq_distances(Xs, Ys), "rbf": KF.rbf_kernel(Xs, Ys, 1.7),
           "self": KF.rbf_kernel(Xs, Xs, 0.9)}
    for k in ref:
        assert got[k].layout == torch.strided and got[k].shape == ref[k].shape
        assert rel(got[k], ref[k]) <= 1e-12, k


def test_multiclass_svm_on_csr_equals_dense_fit(no_densify):
    X, y = integer_rows(300, 60, 4, 2)
    dense = SV.MultiClassSVM(4, C=1.0).fit(X, y)
    ref_pred = dense.predict(X)
    Xs = X.to_sparse_csr()
    no_densify()
    m = SV.MultiClassSVM(4, C=1.0).fit(Xs, y)
    pred_csr = m.predict(Xs)
    pred_dense = m.predict(X)  # a dense query against the CSR support vectors
    assert set(m.machines) == set(dense.machines) and len(m.machines) == 6
    for k, mm in m.machines.items():
        assert torch.equal(mm.alpha, dense.machines[k].alpha), k
        assert mm.sv.layout == torch.sparse_csr and mm.sv.shape[0] == mm.sv_index.numel()
    assert torch.equal(pred_csr, ref_pred) and torch.equal(pred_dense, ref_pred)
    assert (ref_pred == y).double().mean() > 0.9
    # the union of the support rows is stored once, with a zero-padded coefficient matrix
    assert m.sv_union.layout == torch.sparse_csr and m.sv_union.shape[0] == m.sv_train_index.numel()
    assert m.coef_matrix.shape == (m.sv_train_index.numel(), 6) and m.biases.shape == (6,)
    assert torch.equal(m.sv_union.to_sparse_coo().coalesce().values(),
                       Xs.to_sparse_coo().coalesce().values()[torch.isin(
                           Xs.to_sparse_coo().coalesce().indices()[0], m.sv_train_index)])


def test_binary_svm_decision_takes_csr_coo_and_dense_queries(no_densify):
    X, y = integer_rows(120, 40, 2, 3)
    ref = SV.BinarySVM(C=1.0, kernel="rbf", sigma=4.0).fit(X, y)
    want = ref.decision(X)
    Xs = X.to_sparse_csr()
    Xc = X.to_sparse()
    no_densify()
    m = SV.BinarySVM(C=1.0, kernel="rbf", sigma=4.0).fit(Xs, y)
    assert m.sv.layout == torch.sparse_csr
    for Q in (Xs, Xc, X):
        assert rel(m.decision(Q), want) <= 1e-9


def test_take_rows_and_row_ranges():
    X, Y = sparse_block(90, 33, 0.2, 4), sparse_block(41, 33, 0.2, 5)
    Xs = X.to_sparse_csr()
    idx = torch.tensor([5, 0, 17, 89, 5, 34])
    R = CK.take_rows(Xs, idx)
    assert R.layout == torch.sparse_csr and torch.equal(R.to_dense(), X[idx])
    assert CK.take_rows(Xs, torch.zeros(0, dtype=torch.long)).shape == (0, 33)
    assert torch.equal(CK.row_sqnorm(Xs), (X * X).sum(1)) or rel(CK.row_sqnorm(Xs), (X * X).sum(1)) <= 1e-15
    buf = torch.full((30, 50), -7.0, dtype=torch.float64)
    view = buf[3:3 + 25, 4:4 + 41]
    out = CK.kernel_block(Xs, Y.to_sparse_csr(), "linear", k=2.0, b=1.0, rows=(20, 45), out=view)
    assert out.data_ptr() == view.data_ptr()
    assert rel(view, 2.0 * X[20:45] @ Y.t() + 1.0) <= 1e-13
    mask = torch.ones_like(buf, dtype=torch.bool)
    mask[3:28, 4:45] = False
    assert bool((buf[mask] == -7.0).all())
    assert CK.kernel_block(Xs, Y.to_sparse_csr(), rows=(7, 7)).shape == (0, 41)
    assert CK.kernel_path(20000, 20000, 10000, 10 ** 7, 10 ** 7) == "slab"
    assert CK.kernel_path(4000, 4000, 10 ** 6, 200000, 200000) == "merge"
    with pytest.raises(ValueError):
        CK.kernel_block(Xs, sparse_block(5, 34, 0.5, 6).to_sparse_csr())


def _write_daal_csr(path, X):
    """DAAL CSR text (1-based): row offsets, columns, values."""
    Xs = X.to_sparse_csr()
    with open(path, "w") as f:
        f.write(",".join(str(int(v) + 1) for v in Xs.crow_indices()) + "\n")
        f.write(",".join(str(int(v) + 1) for v in Xs.col_indices()) + "\n")
        f.write(",".join(repr(float(v)) for v in Xs.values()) + "\n")


def _daal(algo, inp, work, *flags):
    return cli.main(["daal", algo, "1", "1", "0", "1", str(inp), str(work), "--backend", "gloo", *flags])


def test_cli_daal_kernel_csr_round_trip(tmp_path, capsys):
    X = sparse_block(40, 12, 0.3, 8)
    X[:, 11] = 0.0
    X[3, 11] = 1.5  # the file is as wide as its last used column
    inp = tmp_path / "in"
    os.makedirs(inp)
    _write_daal_csr(inp / "block.csv", X)
    assert _daal("kernel", inp, tmp_path / "out", "--format", "csr", "--kernel", "rbf", "--sigma", "2.5") == 0
    assert json.loads(capsys.readouterr().out.strip().splitlines()[-1])["app"] == "daal"
    got = np.loadtxt(tmp_path / "out" / "kernel_values.csv", delimiter=",")
    assert rel(got, KF.rbf_kernel(X, X, 2.5)) <= 1e-12
    np.savetxt(tmp_path / "dense.csv", X.numpy(), delimiter=",")
    dense_in = tmp_path / "din"
    os.makedirs(dense_in)
    os.replace(tmp_path / "dense.csv", dense_in / "dense.csv")
    assert _daal("kernel", dense_in, tmp_path / "out2", "--kernel", "linear") == 0
    assert rel(np.loadtxt(tmp_path / "out2" / "kernel_values.csv", delimiter=","), X @ X.t()) <= 1e-12


def _check_svm_outputs(work, model, y, pred_test):
    sv = np.loadtxt(work / "svm_sv_index.csv", delimiter=",").reshape(-1)
    coef = np.loadtxt(work / "svm_coef.csv", delimiter=",").reshape(-1, 4)
    bias = np.loadtxt(work / "svm_bias.csv", delimiter=",").reshape(-1, 3)
    want_rows = []
    for (a, b), m in model.machines.items():
        idx = torch.nonzero((y == a) | (y == b)).reshape(-1)[m.sv_index]
        want_rows += [(a, b, int(i), float(c)) for i, c in zip(idx, m.coef)]
    assert coef.shape[0] == len(want_rows) and rel(coef, np.array(want_rows)) <= 1e-12
    assert sorted(set(int(r[2]) for r in want_rows)) == [int(v) for v in sv]
    assert rel(bias[:, 2], [m.bias for m in model.machines.values()]) <= 1e-12
    pred = np.loadtxt(work / "svm_predictions.csv", delimiter=",").reshape(-1)
    assert (pred == pred_test.numpy()).all()


def test_cli_daal_svm_csr_round_trip(tmp_path, capsys):
    X, y = integer_rows(160, 30, 3, 9)
    tr, te = slice(0, 120), slice(120, 160)
    for name, block, lab in (("train", X[tr], y[tr]), ("test", X[te], y[te])):
        os.makedirs(tmp_path / name)
        os.makedirs(tmp_path / (name + "_lab"))
        _write_daal_csr(tmp_path / name / "block.csv", block)
        np.savetxt(tmp_path / (name + "_lab") / "labels.csv", lab.numpy(), fmt="%d")
    work = tmp_path / "out"
    assert _daal("svm", tmp_path / "train", work, "--format", "csr", "--labels", str(tmp_path / "train_lab"),
                 "--test-dir", str(tmp_path / "test"), "--test-labels", str(tmp_path / "test_lab"), "--k", "3",
                 "--c", "0.5") == 0
    res = json.loads(capsys.readouterr().out.strip().splitlines()[-1])["result"]
    model = SV.MultiClassSVM(3, C=0.5).fit(X[tr].to_sparse_csr(), y[tr])
    pred = model.predict(X[te].to_sparse_csr())
    _check_svm_outputs(work, model, y[tr], pred)
    assert res["n_sv"] == int(model.sv_train_index.numel())
    assert res["test_error"] == pytest.approx(float((pred != y[te]).double().mean()))
    assert res["train_error"] == pytest.approx(float((model.predict(X[tr]) != y[tr]).double().mean()))
    # dense input, last column = label: the same model
    for name, block, lab in (("dtrain", X[tr], y[tr]), ("dtest", X[te], y[te])):
        os.makedirs(tmp_path / name)
        np.savetxt(tmp_path / name / "rows.csv", torch.cat([block, lab.double()[:, None]], 1).numpy(), delimiter=",")
    work2 = tmp_path / "out2"
    assert _daal("svm", tmp_path / "dtrain", work2, "--test-dir", str(tmp_path / "dtest"), "--k", "3",
                 "--c", "0.5") == 0
    capsys.readouterr()
    _check_svm_outputs(work2, SV.MultiClassSVM(3, C=0.5).fit(X[tr], y[tr]), y[tr], pred)


@pytest.mark.skipif(not os.path.isdir(REFERENCE), reason="reference datasets not present")
def test_cli_daal_svm_reference_multicsr_fixture(tmp_path, capsys):
    """The reference's daal_svm/multicsr fixture (2,000 rows, 5 classes) with the mapper's
    defaults (linear kernel) through ``daal svm --format csr``, against the dense-input fit
    of the same rows."""
    from harp_amd.utils.datasets import load_daal_csr, load_dense_csv

    work = tmp_path / "out"
    assert _daal("svm", os.path.join(REFERENCE, "train"), work, "--format", "csr", "--labels",
                 os.path.join(REFERENCE, "trainTruth"), "--test-dir", os.path.join(REFERENCE, "test"),
                 "--test-labels", os.path.join(REFERENCE, "testTruth"), "--k", "5") == 0
    res = json.loads(capsys.readouterr().out.strip().splitlines()[-1])["result"]
    Xtr = load_daal_csr(os.path.join(REFERENCE, "train", "svm_multi_class_train_csr.csv"))
    Xte = load_daal_csr(os.path.join(REFERENCE, "test", "svm_multi_class_test_csr.csv"))
    ytr = load_dense_csv(os.path.join(REFERENCE, "trainTruth", "svm_multi_class_train_labels.csv")).reshape(-1).long()
    yte = load_dense_csv(os.path.join(REFERENCE, "testTruth", "svm_multi_class_test_labels.csv")).reshape(-1).long()
    d = max(Xtr.shape[1], Xte.shape[1])
    dense = lambda A: torch.cat([A.to_dense(), torch.zeros(A.shape[0], d - A.shape[1], dtype=torch.float64)], 1)  # noqa: E731
    ref = SV.MultiClassSVM(5, C=1.0).fit(dense(Xtr), ytr)
    ref_pred = ref.predict(dense(Xte))
    pred = torch.from_numpy(np.loadtxt(work / "svm_predictions.csv", delimiter=",").reshape(-1)).long()
    assert Xtr.shape[0] == 2000 and len(ref.machines) == 10
    # the Gram matrices agree to rounding, so the two SMO runs end at the same optimum up to
    # the stopping threshold (1e-3): the predictions differ only next to a decision boundary
    assert (pred == ref_pred).double().mean() >= 0.99
    assert abs(res["test_error"] - float((ref_pred != yte).double().mean())) <= 0.01
    coef = np.loadtxt(work / "svm_coef.csv", delimiter=",").reshape(-1, 4)
    n_ref = sum(m.sv_index.numel() for m in ref.machines.values())
    assert abs(coef.shape[0] - n_ref) <= 0.05 * n_ref
