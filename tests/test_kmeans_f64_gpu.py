"""Native dense fp64 K-means step (csrc/kmeans_f64.hip) against plain fp64 torch on the CPU."""
import pytest
import torch

from harp_amd.models import kmeans_csr as M
from harp_amd.ops import kmeans_f64 as KF

pytestmark = pytest.mark.gpu
BF, F32, F64 = torch.bfloat16, torch.float32, torch.float64
EPS = 2.0 ** -52


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _ref_labels(X, C):
    """argmin of cn - 2 x.c in fp64, ties to the lowest index (spelled out, not left to argmin)."""
    D = (C * C).sum(1)[None, :] - 2 * X.double() @ C.t()
    K = C.shape[0]
    return torch.where(D == D.min(1, keepdim=True)[0], torch.arange(K), K).min(1)[0]


# (d, K as a function of the stage size, n as a function of the workgroup's points, dtype, row stride - d)
_ASSIGN = [
    (1, lambda s: 1, lambda p: 1, F32, 0),
    (1, lambda s: 2 * s + 1, lambda p: p + 1, F64, 0),
    (3, lambda s: 15, lambda p: p - 1, BF, 0),
    (4, lambda s: 16, lambda p: p + 1, F64, 0),
    (5, lambda s: 17, lambda p: 5 * p + 3, F32, 0),
    (100, lambda s: s + 1, lambda p: 5 * p + 3, F32, 0),
    (100, lambda s: 17, lambda p: p + 1, F32, 3),  # X[:, :d] of a wider buffer: rows off 16 bytes
    (128, lambda s: 2 * s + 1, lambda p: p + 1, BF, 0),
    (128, lambda s: 16, lambda p: 5 * p + 3, F64, 64),  # a strided view that keeps the vector loads
    (129, lambda s: s + 1, lambda p: p - 1, F64, 0),
    (256, lambda s: 2 * s + 1, lambda p: 5 * p + 3, F64, 0),
    (256, lambda s: s + 1, lambda p: p + 1, BF, 0),
]


@pytest.mark.parametrize("d,kf,nf,dtype,extra", _ASSIGN)
def test_exact_labels_on_integer_data(cuda, d, kf, nf, dtype, extra):
    """Integers in [-8, 8]: every dot product and norm is exact in fp64 in any order, so the
    labels have to equal the reference's, duplicated centroids resolved to the lowest index."""
    K, n = kf(KF.stage_centroids(d)), nf(KF.points_per_workgroup(d))
    g = _gen(d * 1000 + K)
    C = torch.randint(-8, 9, (K, d), generator=g).double()
    if K > 1:
        C[K - 1] = C[0]  # only the lowest-index rule separates them
        C[K // 2] = C[(K - 1) // 3]
    buf = torch.randint(-8, 9, (n, d + extra), generator=g).to(dtype)
    buf[::3, :d] = C[torch.randint(0, K, ((n + 2) // 3,), generator=g)].to(dtype)  # points on centroids
    X = buf.to(cuda)[:, :d]
    lab = KF.assign(X, C.to(cuda))
    assert lab.dtype == torch.int32 and torch.equal(lab.cpu().long(), _ref_labels(buf[:, :d], C))
    assert torch.equal(lab, KF.assign(X, C.to(cuda)))  # repeatable


def test_real_valued_labels_are_optimal_for_every_row(cuda):
    """The reference distance at the kernel's label is within the fp64 dot-product bound of the
    reference minimum (the bound once for the kernel, once for the reference)."""
    n, d, K = 1000, 100, 300
    X = torch.rand(n, d, generator=_gen(1)) * 1000
    C = torch.rand(K, d, generator=_gen(2), dtype=F64) * 1000
    lab = KF.assign(X.to(cuda), C.to(cuda)).cpu().long()
    assert int(lab.min()) >= 0 and int(lab.max()) < K
    Xd = X.double()
    cn = (C * C).sum(1)
    D = cn[None, :] - 2 * Xd @ C.t()
    slack = 4 * (d + 2) * EPS * ((Xd * Xd).sum(1) + cn.max())
    assert bool((D[torch.arange(n), lab] <= D.min(1)[0] + slack).all())


@pytest.mark.parametrize("d,dtype,exact", [(37, F32, True), (5, BF, True), (256, F64, True), (100, F32, False),
                                           (16, F64, False)])
def test_sums_counts_objective(cuda, d, dtype, exact):
    """One cluster owns 90 % of the rows and three are empty. Quarter-integer points and integer
    centroids make every sum exact: bit equality. Real values: the bounds of a length-n_k sum."""
    n, K = 3001, 9
    g = _gen(d)
    C = torch.randint(-6, 7, (K, d), generator=g).double()
    C[6:] += 100.0  # no point comes near: empty clusters
    own = torch.where(torch.rand(n, generator=g) < 0.9, 0, torch.randint(1, 6, (n,), generator=g))
    noise = torch.randint(-4, 5, (n, d), generator=g) / 4.0 if exact else torch.randn(n, d, generator=g) * 0.7
    X = (C[own] + noise).to(dtype)
    lab, S, cnt, wss = (t.cpu() for t in KF.assign_accumulate(X.to(cuda), C.to(cuda)))
    lab, Xd = lab.long(), X.double()
    if exact:
        assert torch.equal(lab, _ref_labels(X, C))
    S_ref = torch.zeros(K, d, dtype=F64).index_add_(0, lab, Xd)
    w_ref = torch.zeros(K, dtype=F64).index_add_(0, lab, ((Xd - C[lab]) ** 2).sum(1))
    n_k = torch.bincount(lab, minlength=K).double()
    assert torch.equal(cnt, n_k) and float(n_k[0]) > 0.85 * n and int((n_k == 0).sum()) >= 3
    if exact:
        assert torch.equal(S, S_ref) and torch.equal(wss, w_ref)
    else:
        absum = torch.zeros(K, d, dtype=F64).index_add_(0, lab, Xd.abs())
        assert bool(((S - S_ref).abs() <= n_k[:, None] * EPS * absum).all())
        assert bool(((wss - w_ref).abs() <= (n_k * d + 8) * EPS * w_ref).all())


def test_edges(cuda):
    C = torch.rand(9, 40, generator=_gen(2), dtype=F64).to(cuda)
    lab, S, cnt, wss = KF.assign_accumulate(torch.zeros(0, 40, device=cuda), C)
    assert lab.numel() == 0 and S.shape == (9, 40) and not S.any() and not cnt.any() and not wss.any()
    X = torch.rand(300, 40, generator=_gen(3))
    X[7, 3] = float("nan")
    lab, S, cnt, wss = KF.assign_accumulate(X.to(cuda), C)
    assert int(lab.min()) >= 0 and int(lab.max()) < 9 and int(lab[7]) == 0 and float(cnt.sum()) == 300.0
    with pytest.raises(ValueError, match="engine=\"torch\""):
        KF.assign(torch.zeros(4, 257, device=cuda), torch.zeros(2, 257, dtype=F64, device=cuda))


def test_kmeans_native_gpu_equals_cpu_torch(cuda):
    g = _gen(7)
    centres = torch.rand(12, 64, generator=g, dtype=F64) * 8 + 1
    X = (centres[torch.randint(0, 12, (3000,), generator=g)] + torch.randn(3000, 64, generator=g, dtype=F64) * 0.3)
    X = X.clamp(0, 10 - 1e-9)
    C0 = X[:12].clone()
    ref = M.kmeans_sparse(X, C0, 6)
    out = M.kmeans_sparse(X.to(cuda), C0, 6, engine="native")
    assert torch.allclose(out["centroids"].cpu(), ref["centroids"], atol=1e-10)
    assert all(abs(a - b) <= 1e-9 * abs(b) for a, b in zip(out["objective"], ref["objective"]))
    assert out["labels"].dtype == torch.int64 and torch.equal(out["labels"].cpu(), ref["labels"])


def test_no_tensor_proportional_to_n_times_k(cuda):
    n, K, d = 2 ** 17, 1024, 16
    X = torch.rand(n, d, device=cuda, generator=torch.Generator(device=cuda).manual_seed(1))
    C0 = X[:K].double()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.max_memory_allocated()
    M.kmeans_sparse(X, C0, 1, engine="native")
    torch.cuda.synchronize()
    assert torch.cuda.max_memory_allocated() - before < n * K * 8 // 8
