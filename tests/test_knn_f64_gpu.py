"""Native fp64 kNN (csrc/knn_f64.hip) against a stable sort of plain fp64 distance rows on the CPU."""
import pytest
import torch

from harp_amd.models.kernels import KNNClassifier
from harp_amd.ops import knn_f64 as KF

pytestmark = pytest.mark.gpu
BF, F32, F64 = torch.bfloat16, torch.float32, torch.float64
ST = KF.stage_rows


def reference(T, Q, k):
    D = ((Q.double()[:, None, :] - T.double()[None, :, :]) ** 2).sum(-1)
    d, i = D.sort(dim=1, stable=True)
    return d[:, :k], i[:, :k]


def ints(n, d, dtype, extra, seed):
    """Integer coordinates in [0, 16) (exact in every dtype: every distance is an exact integer in
    fp64) in an [n, d + extra] buffer; every odd row repeats the row before it."""
    buf = torch.randint(0, 16, (n, d + extra), generator=torch.Generator().manual_seed(seed)).to(dtype)
    buf[1::2] = buf[0:n - 1:2]
    return buf


# widths 1 .. 256 (every step count form, one and two query tiles per wave), k 1 .. 32 (every list
# length), training rows around one and two LDS stages, partial query tiles and more than one
# workgroup, splits beyond the number of stages; extra > 0: unaligned rows, the scalar-load path
@pytest.mark.parametrize("N,d,k,M,dtype,extra,splits", [
    (3, 1, 5, 1, F64, 0, 1), (17, 5, 1, 17, F32, 0, 1), (ST(33) - 1, 33, 4, 65, BF, 0, 1),
    (ST(100) + 1, 100, 9, 130, F32, 0, 2), (2 * ST(129) + 1, 129, 17, 65, F64, 0, 5),
    (2 * ST(256) + 1, 256, 32, 17, BF, 0, 2), (2 * ST(5) + 1, 5, 32, 130, F32, 2, 1),
    (ST(33) + 1, 33, 17, 130, F64, 2, 5), (2 * ST(1) + 1, 1, 9, 130, BF, 2, 2), (ST(100) - 1, 100, 5, 1, F64, 1, 1)])
def test_exact_on_integer_rows(cuda, N, d, k, M, dtype, extra, splits):
    T, Q = ints(N, d, dtype, extra, N + d), ints(M, d, dtype, extra, M + k)
    dist, idx = KF.knn_search(T.to(cuda)[:, :d], Q.to(cuda)[:, :d], k, splits=splits)
    rd, ri = reference(T[:, :d], Q[:, :d], k)
    assert dist.dtype == F64 and idx.dtype == torch.int64 and dist.shape == (M, min(k, N))
    assert torch.equal(dist.cpu(), rd) and torch.equal(idx.cpu(), ri)


@pytest.mark.parametrize("k,splits", [(10, 1), (32, 1), (10, 3), (32, 3)])
def test_ties_across_tiles_stages_and_splits(cuda, k, splits):
    g = torch.Generator().manual_seed(k)
    T = torch.randint(0, 16, (6, 5), generator=g).double()[torch.randint(0, 6, (700,), generator=g)]
    Q = torch.randint(0, 16, (17, 5), generator=g).double()
    dist, idx = KF.knn_search(T.to(cuda), Q.to(cuda), k, splits=splits)
    rd, ri = reference(T, Q, k)
    assert torch.equal(dist.cpu(), rd) and torch.equal(idx.cpu(), ri)


@pytest.mark.parametrize("d,k,splits", [(33, 5, 1), (129, 17, 2)])
def test_real_rows_within_the_derived_bound(cuda, d, k, splits):
    """Queries are training rows near 1e3, so the expansion cancels. Bound: gamma_d sum |q_i t_i|
    for the d-term dot product in any order with 2 |q.t| <= |q|^2 + |t|^2, the two norms, three adds."""
    N, M = 300, 65
    T = 1e3 + torch.randn(N, d, dtype=F64, generator=torch.Generator().manual_seed(d))
    Q = T[:M].clone()
    dist, idx = (t.cpu() for t in KF.knn_search(T.to(cuda), Q.to(cuda), k, splits=splits))
    assert not dist.isnan().any() and bool((dist >= 0).all()) and bool((dist[:, 1:] >= dist[:, :-1]).all())
    assert bool(((idx >= 0) & (idx < N)).all())
    named = T[idx]  # [M, k, d]
    true = ((Q[:, None, :] - named) ** 2).sum(-1)
    bound = (2 * d + 8) * 2.0 ** -53 * ((Q * Q).sum(1)[:, None] + (named * named).sum(-1))
    assert bool(((dist - true).abs() <= bound).all())


def test_repeatable_and_cached_operand(cuda):
    g = torch.Generator().manual_seed(2)
    T, Q = torch.randn(1000, 20, generator=g).to(cuda), torch.randn(70, 20, generator=g).to(cuda)
    first = KF.knn_search(T, Q, 7)
    for again in (KF.knn_search(T, Q, 7), KF.knn_search(T, Q, 7, operand=KF.prepare(T))):
        assert torch.equal(first[0], again[0]) and torch.equal(first[1], again[1])


def test_no_buffer_proportional_to_m_times_n(cuda):
    M, N, d, k = 4096, 65536, 32, 16
    g = torch.Generator(device=cuda).manual_seed(1)
    T, Q = torch.rand(N, d, device=cuda, generator=g), torch.rand(M, d, device=cuda, generator=g)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.max_memory_allocated()
    out = KF.knn_search(T, Q, k)
    torch.cuda.synchronize()
    operand = 8 * (-(-N // ST(d)) * ST(d) // 16) * (64 * KF.padded_width(d) // 4 + 16)
    assert torch.cuda.max_memory_allocated() - before < operand + M * k * (8 + 4 + 8) + 16 * 2 ** 20
    assert out[0].shape == (M, k)  # the distance tile alone would be 2 GB


def test_classifier_native_on_gpu_equals_torch_on_cpu(cuda):
    g = torch.Generator().manual_seed(4)
    centres = 20.0 * torch.eye(4, 6, dtype=F64)
    y = torch.randint(0, 4, (400,), generator=g)
    X = centres[y] + torch.randn(400, 6, dtype=F64, generator=g)
    Q = centres[y[:90]] + torch.randn(90, 6, dtype=F64, generator=g)
    nat = KNNClassifier(5, engine="native").fit(X.to(cuda), y.to(cuda)).predict(Q.to(cuda))
    assert torch.equal(nat.cpu(), KNNClassifier(5, engine="torch").fit(X, y).predict(Q))
