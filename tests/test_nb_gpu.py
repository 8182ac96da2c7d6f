"""Native dense naive Bayes (csrc/nb.hip) against plain fp64 torch on the CPU."""
import pytest
import torch

from harp_amd.models import naive_bayes as NB
from harp_amd.ops import nb as NBK

pytestmark = pytest.mark.gpu
BF, F32, F64 = torch.bfloat16, torch.float32, torch.float64
EPS = 2.0 ** -52


def rows(n, d, C, dtype, extra, seed):
    """Integer counts 0..7 (exact in every dtype) in an [n, d + extra] buffer, and labels that
    leave class 1 empty when C > 2."""
    g = torch.Generator().manual_seed(seed)
    buf = torch.randint(0, 8, (n, d + extra), generator=g).to(dtype)
    y = torch.randint(0, C, (n,), generator=g)
    return buf, torch.where((y == 1) & (C > 2), 0, y)


def ref_sums(X, y, C):
    return (torch.zeros(C, X.shape[1], dtype=F64).index_add_(0, y, X.double()), torch.bincount(y, minlength=C).double())


# the last one: 3 column tiles, so 170 row splits, and 172 chunks of 256 rows with a ragged last
@pytest.mark.parametrize("n,d,C,dtype,extra", [
    (1, 1, 1, F32, 0), (63, 3, 2, BF, 1), (64, 255, 17, F64, 0), (65, 256, 64, F32, 1), (257, 257, 17, BF, 0),
    (257, 256, 2, F64, 1), (600, 513, 64, BF, 1), (43783, 513, 17, F32, 0)])
def test_class_sums_exact_on_counts(cuda, n, d, C, dtype, extra):
    buf, y = rows(n, d, C, dtype, extra, seed=n + d)
    S, cnt = NBK.class_sums(buf.to(cuda)[:, :d], y.to(cuda), C)
    S_ref, cnt_ref = ref_sums(buf[:, :d], y, C)
    assert torch.equal(S.cpu(), S_ref) and torch.equal(cnt.cpu(), cnt_ref)
    assert C <= 2 or cnt_ref[1] == 0


def test_class_sums_keep_what_fp32_accumulators_round(cuda):
    X = torch.full((18, 2), 2.0 ** 20)
    X[17] = 1.0
    S, cnt = NBK.class_sums(X.to(cuda), torch.ones(18, dtype=torch.long, device=cuda), 2)
    assert S.cpu().tolist() == [[0.0, 0.0], [17 * 2.0 ** 20 + 1] * 2] and cnt.cpu().tolist() == [0.0, 18.0]


def test_class_sums_real_values_bounded_and_repeatable(cuda):
    n, d, C = 3001, 300, 5
    g = torch.Generator().manual_seed(3)
    X, y = torch.randn(n, d, generator=g, dtype=F64), torch.randint(0, C, (n,), generator=g)
    S, _ = NBK.class_sums(X.to(cuda), y.to(cuda), C)
    absum = torch.zeros(C, d, dtype=F64).index_add_(0, y, X.abs())
    assert bool(((S.cpu() - ref_sums(X, y, C)[0]).abs() <= n * EPS * absum).all())
    assert torch.equal(S, NBK.class_sums(X.to(cuda), y.to(cuda), C)[0])


@pytest.mark.parametrize("n,d,C,dtype,extra", [
    (1, 1, 1, F32, 0), (15, 3, 2, BF, 1), (16, 4, 15, F64, 0), (17, 5, 16, F32, 3), (63, 63, 17, BF, 0),
    (64, 64, 33, F64, 1), (65, 65, 64, F32, 0), (129, 130, 64, F64, 1), (129, 130, 33, BF, 1)])
def test_predict_exact_on_quarter_integer_models(cuda, n, d, C, dtype, extra):
    """Counts times quarter-integers: every score is exact in fp64 in any order. Classes 0 and
    C - 1 are one model with the highest prior (a tie across MFMA tiles when C > 16) and win the
    all-zero rows 0, 3, .., which the prior alone decides; classes 2 and 5 (one tile) tie for the
    rows 1, 4, .. that hold only feature 0, where they alone have logTheta = 0."""
    buf, _ = rows(n, d, C, dtype, extra, seed=n + C)
    g = torch.Generator().manual_seed(C)
    lt = torch.randint(-40, -3, (C, d), generator=g).double() / 4
    lp = torch.randint(-20, -1, (C,), generator=g).double() / 4
    lt[C - 1], lp[0], lp[C - 1] = lt[0], 0.0, 0.0
    buf[::3, :d] = 0
    if C > 5:
        lt[2, 0], lt[5], lp[2], lp[5] = 0.0, lt[2], -0.25, -0.25
        lt[5, 0] = 0.0
        buf[1::3, :d] = 0
        buf[1::3, 0] = 7
    S = buf[:, :d].double() @ lt.t() + lp
    ref = torch.where(S == S.max(1, keepdim=True)[0], torch.arange(C), C).min(1)[0]
    assert int(ref[0]) == 0 and (C <= 5 or n < 2 or int(ref[1]) == 2)
    lab = NBK.predict(buf.to(cuda)[:, :d], lt.to(cuda), lp.to(cuda))
    assert lab.dtype == torch.int64 and torch.equal(lab.cpu(), ref)


def test_train_then_predict_matches_cpu_outside_the_rounding_gap(cuda):
    n, d, C = 4000, 70, 20
    g = torch.Generator().manual_seed(11)
    y = torch.randint(0, C, (n,), generator=g)
    X = (torch.randint(0, 4, (n, d), generator=g) + 4 * (torch.arange(d)[None, :] % C == y[:, None])).float()
    ref = NB.train(X.double(), y, C)
    model = NB.train(X.to(cuda), y.to(cuda), C, engine="native")
    assert torch.equal(model["featureSums"].cpu(), ref["featureSums"])
    S = X.double() @ ref["logTheta"].t() + ref["logPrior"]
    top = S.topk(2, dim=1)[0]
    sure = top[:, 0] - top[:, 1] > 4 * d * EPS * X.double().sum(1) * ref["logTheta"].abs().max()
    assert float((~sure).double().mean()) <= 0.01
    lab = NB.predict(X.to(cuda), model, engine="native").cpu()
    assert torch.equal(lab[sure], S.argmax(1)[sure])


def test_edges(cuda):
    lt, lp = torch.zeros(3, 5, dtype=F64, device=cuda), torch.zeros(3, dtype=F64, device=cuda)
    lt[0, 2] = float("nan")  # class 0 is NaN for every row: it never wins; row 4 is NaN throughout
    X = torch.ones(9, 5, device=cuda)
    X[4, 1] = float("nan")
    assert NBK.predict(X, lt, lp).tolist() == [1, 1, 1, 1, 0, 1, 1, 1, 1]
    assert NBK.predict(X[:0], lt, lp).shape == (0,) and not NBK.class_sums(X[:0], X[:0, 0].long(), 3)[0].any()
    with pytest.raises(ValueError, match="label outside"):
        NBK.class_sums(X, torch.full((9,), 3, device=cuda), 3)
    with pytest.raises(ValueError, match="engine=\"torch\""):
        NBK.class_sums(X, torch.zeros(9, dtype=torch.long, device=cuda), 65)


def test_no_tensor_proportional_to_n_times_c_or_d(cuda):
    n, d, C = 2 ** 18, 256, 20
    X = torch.rand(n, d, device=cuda, generator=torch.Generator(device=cuda).manual_seed(1))
    y = torch.randint(0, C, (n,), device=cuda)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.max_memory_allocated()
    NB.predict(X, NB.train(X, y, C, engine="native"), engine="native")
    torch.cuda.synchronize()
    assert torch.cuda.max_memory_allocated() - before < 16 * n + NBK.partial_bytes(d, C) + 2 ** 20
