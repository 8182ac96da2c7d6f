"""GPU CSR statistics kernels (csrc/csr_stats.hip) against the non-densifying fp64 torch
references of ops/csr_stats.py on the same data, and the library paths built on them."""
import functools
import os

import numpy as np
import pytest
import torch

from harp_amd.models import naive_bayes as NB
from harp_amd.models import stats as ST
from harp_amd.ops import csr_stats as CS
from harp_amd.ops import linalg as LA
from harp_amd.utils import datasets as DS

pytestmark = pytest.mark.gpu

T = CS.GRAM_TILE
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "datasets")
MOMENTS = ("minimum", "maximum", "sum", "sumSquares", "sumSquaresCentered", "mean", "secondOrderRawMoment",
           "variance", "standardDeviation", "variation")


def _pattern(n, d, density, g):
    """Every 17th row empty, one fully dense row (more than 64 nonzeros in one feature block
    once d > 64)."""
    keep = torch.rand(n, d, generator=g) < density
    keep[::17] = False
    keep[min(5, n - 1), :] = True
    return keep


def _operand(rows, cols, vals, n, d):
    """CSR operand from (row-sorted) coordinates, without a dense intermediate."""
    rowptr = torch.zeros(n + 1, dtype=torch.long)
    rowptr[1:] = torch.cumsum(torch.bincount(rows, minlength=n), 0)
    return CS.CSROperand(rowptr, cols.to(torch.int32), vals.double(), n, d)


@functools.lru_cache(maxsize=None)
def _case(n, d, kind):
    """(operand on the CPU, its reference upper-triangle Gram); computed once per shape."""
    g = torch.Generator().manual_seed(1000 * n + d)
    rows, cols = _pattern(n, d, 0.05 if d > 10 else 0.5, g).nonzero(as_tuple=True)
    if kind == "int":  # integers in (-2^20, 2^20): with n <= 4096 every partial sum is an integer < 2^53
        vals = torch.randint(-(2 ** 20) + 1, 2 ** 20, (rows.numel(),), generator=g).double()
    else:  # uniform in [-0.5, 1.5)
        vals = torch.rand(rows.numel(), generator=g, dtype=torch.float64) * 2.0 - 0.5
    A = _operand(rows, cols, vals, n, d)
    return A, CS.gram_ref(A)


def _to(A, dev):
    return CS.CSROperand(A.rowptr.to(dev), A.col.to(dev), A.val.to(dev), A.n, A.d)


SHAPES_D = [1, 10, T - 1, T, T + 1, 2 * T + 1, 300]
SHAPES_N = [1, 63, 4000]


@pytest.mark.parametrize("path", ["tiled", "direct"])
@pytest.mark.parametrize("n", SHAPES_N)
@pytest.mark.parametrize("d", SHAPES_D)
def test_gram_exact_on_integers(cuda, d, n, path):
    A, ref = _case(n, d, "int")
    G = CS.gram(_to(A, cuda), path=path)
    assert torch.equal(G.cpu(), ref)


def test_gram_exact_many_splits_accumulate_and_chooser(cuda):
    A, ref = _case(4000, 2 * T + 1, "int")
    Ad = _to(A, cuda)
    assert torch.equal(CS.gram(Ad, path="tiled", rows_per_split=64).cpu(), ref)  # 63 workgroups flush into a tile
    G0 = torch.arange(A.d * A.d, dtype=torch.float64).reshape(A.d, A.d)
    for path in ("tiled", "direct", None):
        G = G0.clone().to(cuda)
        assert CS.gram(Ad, out=G, path=path) is G
        assert torch.equal(G.cpu(), G0 + ref)
    assert torch.equal(LA.symmetrize_upper(CS.gram(Ad)).cpu(), LA.symmetrize_upper(ref))


def test_gram_no_rows_returns_zeros(cuda):
    A = CS.CSROperand(torch.zeros(1, dtype=torch.long, device=cuda), torch.zeros(0, dtype=torch.int32, device=cuda),
                      torch.zeros(0, dtype=torch.float64, device=cuda), 0, 7)
    for path in ("tiled", "direct"):
        G = CS.gram(A, path=path)
        assert G.shape == (7, 7) and not bool(G.any())
    assert A.blk is None  # nothing was launched, not even the offsets kernel


@pytest.mark.parametrize("path", ["tiled", "direct"])
@pytest.mark.parametrize("n,d", [(63, T + 1), (4000, 300)])
def test_gram_real_values_within_summation_bound(cuda, n, d, path):
    """|G - G_ref| <= 2 (n + 2) 2^-53 |X|^T |X| elementwise: the any-order summation bound,
    once for each side."""
    A, ref = _case(n, d, "real")
    absA = CS.CSROperand(A.rowptr, A.col, A.val.abs(), A.n, A.d)
    bound = 2.0 * (n + 2) * 2.0 ** -53 * CS.gram_ref(absA)
    G = CS.gram(_to(A, cuda), path=path).cpu()
    worst = float(((G - ref).abs() - bound).max())
    print(f"n={n} d={d} {path}: max |G - ref| = {float((G - ref).abs().max()):.3e}, max bound = {float(bound.max()):.3e}")
    assert worst <= 0.0


# ------------------------------------------------------------------ moments
def _moments_block(n, d, shift, seed):
    """Columns by kind, (j + shift) % 3: 0 fully stored and strictly positive, 1 all zero,
    2 sparse with negative values."""
    g = torch.Generator().manual_seed(seed)
    X = torch.rand(n, d, generator=g, dtype=torch.float64) * 2.0 - 0.5
    kind = (torch.arange(d) + shift) % 3
    X[:, kind == 0] = X[:, kind == 0].abs() + 0.25
    X[:, kind == 1] = 0.0
    sparse_cols = kind == 2
    drop = torch.rand(n, d, generator=g) < 0.7
    X[drop & sparse_cols] = 0.0
    if n > 1:
        X[0, sparse_cols] = -0.375  # a negative stored value in every sparse column
    return X


def _numpy_moments(A):
    n = A.shape[0]
    mean = A.mean(0)
    with np.errstate(all="ignore"):
        var = ((A - mean) ** 2).sum(0) / max(n - 1, 1)
        return {"minimum": A.min(0), "maximum": A.max(0), "sum": A.sum(0), "sumSquares": (A * A).sum(0),
                "sumSquaresCentered": ((A - mean) ** 2).sum(0), "mean": mean,
                "secondOrderRawMoment": (A * A).sum(0) / n, "variance": var, "standardDeviation": np.sqrt(var),
                "variation": np.sqrt(var) / mean}


def _assert_moments(got, ref):
    for k in MOMENTS:
        a, b = got[k].cpu().numpy(), ref[k]
        assert np.array_equal(np.isnan(a), np.isnan(b)), k  # 0 / 0 of an all-zero column on both sides
        ok = ~np.isnan(b)
        if ok.any():
            err = float(np.abs(a[ok] - b[ok]).max() / max(np.abs(b[ok]).max(), 1e-300))
            assert err <= 1e-10, (k, err)


@pytest.mark.parametrize("n", [1, 300])
@pytest.mark.parametrize("shift", [0, 1, 2])
@pytest.mark.parametrize("d", [1, 10, CS.MOM_LDS_MAX_D + 1])
def test_low_order_moments_match_numpy(cuda, d, shift, n):
    X = _moments_block(n, d, shift, 7 * d + shift)
    got = ST.low_order_moments(X.to_sparse_csr().to(cuda))
    _assert_moments(got, _numpy_moments(X.numpy()))
    if n > 1:
        pos = ((torch.arange(d) + shift) % 3) == 0
        assert bool((got["minimum"].cpu()[pos] > 0).all())  # a fully stored column's minimum is not the implicit 0


def test_col_moments_matches_reference(cuda):
    A, _ = _case(4000, 300, "real")
    c = torch.rand(A.d, dtype=torch.float64, generator=torch.Generator().manual_seed(3))
    ref = CS.col_moments_ref(A, c)
    got = CS.col_moments(_to(A, cuda), c.to(cuda))
    assert torch.equal(got["count"].cpu(), ref["count"])
    assert torch.equal(got["min"].cpu(), ref["min"]) and torch.equal(got["max"].cpu(), ref["max"])
    assert torch.allclose(got["sum"].cpu(), ref["sum"], rtol=1e-12, atol=1e-10)
    assert torch.allclose(got["sumsq"].cpu(), ref["sumsq"], rtol=1e-12, atol=1e-10)


# ------------------------------------------------------------------ class sums / spmm
@functools.lru_cache(maxsize=None)
def _counts_case():
    """Bag-of-words block: integer counts 1..9."""
    n, d = 4000, 300
    g = torch.Generator().manual_seed(11)
    rows, cols = _pattern(n, d, 0.05, g).nonzero(as_tuple=True)
    vals = torch.randint(1, 10, (rows.numel(),), generator=g).double()
    return _operand(rows, cols, vals, n, d)


CLASSES = [1, 2, 64, 65, 1500]


@pytest.mark.parametrize("C", CLASSES)
def test_class_sums_exact(cuda, C):
    A = _counts_case()
    y = torch.randint(0, C, (A.n,), generator=torch.Generator().manual_seed(C))
    ref_s, ref_c = CS.class_sums_ref(A, y, C)
    s, c = CS.class_sums(_to(A, cuda), y.to(cuda), C)
    assert torch.equal(s.cpu(), ref_s) and torch.equal(c.cpu(), ref_c)


def test_class_sums_bad_label_raises(cuda):
    A = _counts_case()
    y = torch.zeros(A.n, dtype=torch.long)
    y[77] = 3
    with pytest.raises(ValueError):
        CS.class_sums(_to(A, cuda), y.to(cuda), 3)


@pytest.mark.parametrize("C", CLASSES)
def test_spmm_scores_and_argmax(cuda, C):
    A = _counts_case()
    g = torch.Generator().manual_seed(100 + C)
    B = -torch.rand(A.d, C, generator=g, dtype=torch.float64) * 8.0  # log-probability-like
    bias = -torch.rand(C, generator=g, dtype=torch.float64)
    ref = CS.spmm_ref(A, B, bias)
    Ad = _to(A, cuda)
    assert torch.allclose(CS.spmm(Ad, B.to(cuda), bias.to(cuda)).cpu(), ref, rtol=1e-12, atol=1e-10)
    assert torch.allclose(CS.spmm(Ad, B.to(cuda)).cpu(), CS.spmm_ref(A, B), rtol=1e-12, atol=1e-10)
    lab = CS.spmm(Ad, B.to(cuda), bias.to(cuda), argmax=True).cpu()
    assert lab.dtype == torch.long and lab.shape == (A.n,)
    if C > 1:
        top = ref.topk(2, dim=1).values
        clear = (top[:, 0] - top[:, 1]) > 1e-9
    else:
        clear = torch.ones(A.n, dtype=torch.bool)
    assert int((~clear).sum()) <= A.n // 1000  # the seeded data leaves out none
    assert torch.equal(lab[clear], ref.argmax(1)[clear])
    empty = (A.rowptr[1:] == A.rowptr[:-1])
    assert int(empty.sum()) > 0 and bool((lab[empty] == int(bias.argmax())).all())


@pytest.mark.parametrize("C", [2, 65, 1500])
def test_spmm_argmax_ties_go_to_the_lowest_column(cuda, C):
    """Integer counts times integer weights: tied scores are bit-equal."""
    A = _counts_case()
    g = torch.Generator().manual_seed(C)
    B = torch.randint(0, 5, (A.d, C), generator=g).double()
    lo, hi = (0, 1) if C == 2 else (2, C - 3)
    B[:, lo] = B[:, hi] = 7.0  # both strictly above every other weight
    bias = torch.zeros(C, dtype=torch.float64)
    if C > 2:
        bias[1] = 0.5  # an empty row's argmax; a stored count of >= 1 outweighs it elsewhere
    lab = CS.spmm(_to(A, cuda), B.to(cuda), bias.to(cuda), argmax=True).cpu()
    empty = (A.rowptr[1:] == A.rowptr[:-1])
    assert bool((lab[~empty] == lo).all())
    assert bool((lab[empty] == (1 if C > 2 else 0)).all())
    assert torch.equal(lab, CS.spmm_ref(A, B, bias, argmax=True))


# ------------------------------------------------------------------ end to end
def _dense(A):
    X = torch.zeros(A.n, A.d, dtype=torch.float64)
    X[A.rows(), A.col.long()] = A.val
    return X


def test_naive_bayes_cuda_csr_equals_cpu_dense(cuda):
    A = _counts_case()
    X = _dense(A)
    y = torch.randint(0, 20, (A.n,), generator=torch.Generator().manual_seed(5))
    ref = NB.train(X, y, 20)
    Xs = torch.sparse_csr_tensor(A.rowptr, A.col.long(), A.val, size=(A.n, A.d)).to(cuda)
    m = NB.train(Xs, y.to(cuda), 20)
    assert torch.equal(m["featureSums"].cpu(), ref["featureSums"])
    assert torch.equal(m["classCounts"].cpu(), ref["classCounts"])
    scores = X @ ref["logTheta"].t() + ref["logPrior"]
    top = scores.topk(2, dim=1).values
    clear = (top[:, 0] - top[:, 1]) > 1e-9
    assert int((~clear).sum()) <= A.n // 1000
    assert torch.equal(NB.predict(Xs, m).cpu()[clear], scores.argmax(1)[clear])


def test_pca_cuda_csr_equals_cpu_dense(cuda):
    A, _ = _case(4000, 40, "real")
    X = _dense(A)
    ref = ST.pca(X)
    got = ST.pca(torch.sparse_csr_tensor(A.rowptr, A.col.long(), A.val, size=(A.n, A.d)).to(cuda))
    ev, vec = got["eigenvalues"].cpu(), got["eigenvectors"].cpu()
    assert float((ev - ref["eigenvalues"]).abs().max() / ref["eigenvalues"].abs().max()) <= 1e-10
    sign = torch.sign((vec * ref["eigenvectors"]).sum(1, keepdim=True))
    assert float((vec * sign - ref["eigenvectors"]).abs().max()) <= 1e-8


def test_reference_csr_fixture_covariance(cuda):
    """The reference's smallest CSR fixture (daal_cov/daal_cov_csr, file 1) on the GPU."""
    X = DS.load_daal_csr(os.path.join(GOLDEN, "daal_cov", "daal_cov_csr", "covcormoments_csr_1.csv"))
    r = ST.covariance(X.to(cuda))
    A = CS.to_csr_operand(X)
    D = _dense(A).numpy()
    ref = np.cov(D, rowvar=False)
    assert float(np.abs(r["covariance"].cpu().numpy() - ref).max() / np.abs(ref).max()) <= 1e-10
    assert float(np.abs(r["mean"].cpu().numpy() - D.mean(0)).max() / np.abs(D.mean(0)).max()) <= 1e-10


def test_covariance_memory_stays_far_below_a_dense_copy(cuda):
    """n = 250,000, d = 1024, 8 nonzeros per row: the peak rises by less than n * d bytes (a
    quarter of one fp32 dense copy); operand, block offsets and G together are under 60 MB."""
    n, d, m = 250_000, 1024, 8
    g = torch.Generator(device=cuda).manual_seed(0)
    rowptr = torch.arange(n + 1, device=cuda) * m
    col = ((torch.arange(n, device=cuda) % (d // m))[:, None] + (d // m) * torch.arange(m, device=cuda)).reshape(-1)
    val = torch.rand(n * m, generator=g, device=cuda, dtype=torch.float64)
    X = torch.sparse_csr_tensor(rowptr, col, val, size=(n, d))
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    r = ST.covariance(X)
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated() - before
    print(f"peak rise {rise / 2 ** 20:.1f} MiB (limit {n * d / 2 ** 20:.0f} MiB)")
    assert rise < n * d
    s = torch.zeros(d, dtype=torch.float64, device=cuda).index_add_(0, col, val)
    assert torch.allclose(r["mean"], s / n, rtol=1e-12, atol=0)
    sq = torch.zeros(d, dtype=torch.float64, device=cuda).index_add_(0, col, val * val)
    var = (sq - n * (s / n) ** 2) / (n - 1)
    assert torch.allclose(r["covariance"].diagonal(), var, rtol=1e-9, atol=0)
