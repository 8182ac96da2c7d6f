"""GPU kNN (csrc/knn.hip: hipBLASLt Q T^T + fused distance / top-k selection) vs an fp64
torch reference of the same search."""
import pytest
import torch

from harp_amd.models.kernels import KNNClassifier
from harp_amd.ops import knn as KN

pytestmark = pytest.mark.gpu


def _ref(train, queries, k):
    D = torch.cdist(queries.double(), train.double()) ** 2
    return torch.topk(D, k, dim=1, largest=False)


@pytest.mark.parametrize("k", [1, 5, 16, 32])
@pytest.mark.parametrize("n,t_tile", [(3001, 1 << 16), (20000, 4096), (37, 1 << 16)])
def test_knn_matches_reference(cuda, k, n, t_tile):
    g = torch.Generator().manual_seed(k * 7 + n)
    d = 24
    train = torch.randn(n, d, generator=g)
    queries = torch.randn(1000, d, generator=g)
    kk = min(k, n)
    rd, ri = _ref(train, queries, kk)
    od, oi = KN.knn_search(train.to(cuda), queries.to(cuda), k, q_tile=384, t_tile=t_tile)
    od, oi = od.cpu().double(), oi.cpu()
    assert od.shape == (1000, kk) and oi.dtype == torch.int64
    assert (od[:, 1:] >= od[:, :-1]).all()
    assert torch.allclose(od, rd, rtol=1e-4, atol=1e-3)
    # indices agree wherever the reference's neighbours are separated from the next one
    exact = (train[oi] - queries[:, None, :]).double().pow(2).sum(-1)
    assert torch.allclose(exact, rd, rtol=1e-4, atol=1e-3)
    assert (oi.sort(1).values == ri.sort(1).values).float().mean() > 0.99


def test_knn_ties_resolve_to_lower_index(cuda):
    train = torch.zeros(700, 8)
    train[::2] += 1.0  # 350 rows at distance 0 from the origin query, 350 at distance 8
    od, oi = KN.knn_search(train.to(cuda), torch.ones(3, 8, device=cuda), 10)
    assert torch.equal(oi.cpu(), torch.arange(0, 20, 2).expand(3, 10))
    assert od.abs().max().item() == 0.0


def test_knn_classifier_on_gpu(cuda):
    g = torch.Generator().manual_seed(3)
    centers = torch.randn(4, 16, generator=g) * 6
    y = torch.randint(0, 4, (4000,), generator=g)
    X = centers[y] + torch.randn(4000, 16, generator=g)
    clf = KNNClassifier(k=7).fit(X[:3000].to(cuda), y[:3000].to(cuda))
    pred = clf.predict(X[3000:].to(cuda)).cpu()
    ref = KNNClassifier(k=7).fit(X[:3000], y[:3000]).predict(X[3000:])
    assert (pred == ref).float().mean() > 0.995
    assert (pred == y[3000:]).float().mean() > 0.97


def test_knn_rejects_unsupported(cuda):
    t = torch.randn(100, 4, device=cuda)
    with pytest.raises(ValueError):
        KN.knn_search(t, t, 33)
    with pytest.raises(TypeError):
        KN.knn_search(t.double(), t.double(), 3)


# ---------------------------------------------------------------------------------------
# Exact data: integer coordinates in [0, 16) stored as fp32, d <= 64. Every product, norm
# and GEMM sum is an integer below 2^24, exact in fp32 in any order, so the kernel's
# distances equal the fp64 distances bit for bit and its indices equal a stable ascending
# sort of the fp64 distance rows entry for entry: no tolerance, no agreement fraction. The
# data is full of duplicates and equal distances, so the tie rule (lower train index) is
# checked on every row.
def _int_points(n, d, g):
    return torch.randint(0, 16, (n, d), generator=g).float()


def _assert_exact(cuda, train, queries, k, q_tile, t_tile):
    D = (queries.double()[:, None, :] - train.double()[None, :, :]).pow(2).sum(-1)
    rd, ri = torch.sort(D, dim=1, stable=True)
    kk = min(k, train.shape[0])
    od, oi = KN.knn_search(train.to(cuda), queries.to(cuda), k, q_tile=q_tile, t_tile=t_tile)
    assert od.shape == oi.shape == (queries.shape[0], kk) and oi.dtype == torch.int64
    assert torch.equal(od.double().cpu(), rd[:, :kk])
    assert torch.equal(oi.cpu(), ri[:, :kk])


# (train rows, t_tile): train-tile widths 64 + 1, 64 + 63, 320 + 65, 256 + 255, 257 + 257,
# 256 + 256 + 1 (the 4-way loop with and without a tail, the tail alone), and 1000 and
# 1023, where the fourth trip of the 4-way loop is entered by some lanes of a wave only
@pytest.mark.parametrize("n,t_tile", [(65, 64), (127, 64), (385, 320), (511, 256), (514, 257), (513, 256),
                                      (1000, 1024), (2023, 1023)])
@pytest.mark.parametrize("k", [4, 8, 9, 17, 32])
def test_knn_exact_list_lengths_and_tile_widths(cuda, k, n, t_tile):
    g = torch.Generator().manual_seed(31 * n + k)
    train, queries = _int_points(n, 5, g), _int_points(5, 5, g)
    _assert_exact(cuda, train, queries, k, 4, t_tile)  # the second query tile: one row at an offset


def test_knn_exact_merge_into_empty_slots(cuda):
    """The first train tiles are shorter than k, so the running state carries index -1 slots
    into the next merges; and fewer train rows than k return that many columns."""
    g = torch.Generator().manual_seed(77)
    _assert_exact(cuda, _int_points(40, 64, g), _int_points(5, 64, g), 16, 4, 5)
    _assert_exact(cuda, _int_points(3, 7, g), _int_points(5, 7, g), 5, 4, 1 << 16)
    _assert_exact(cuda, _int_points(3, 7, g), _int_points(5, 7, g), 5, 4, 2)


@pytest.mark.parametrize("k", [10, 32])
def test_knn_exact_ties_across_train_tiles(cuda, k):
    g = torch.Generator().manual_seed(5)
    points = _int_points(6, 8, g)
    train = points[torch.randint(0, 6, (700,), generator=g)]
    queries = torch.cat([points[:3], _int_points(2, 8, g)])
    _assert_exact(cuda, train, queries, k, 4, 256)


def test_knn_cancellation_is_clamped(cuda):
    """Queries are copies of train rows with coordinates near 1e3: |q|^2 + |t|^2 - 2 q.t
    cancels seven digits. Own-distances come out clamped at >= 0, nothing is NaN, and every
    returned distance is within 2 d 2^-24 (|q|^2 + |t|^2) of the fp64 distance to the row it
    names (the worst-case rounding of a d-term fp32 dot product plus the three additions)."""
    g = torch.Generator().manual_seed(8)
    d, n, M, k = 16, 300, 64, 8
    train = 1e3 + torch.randn(n, d, generator=g)
    queries = train[torch.randperm(n, generator=g)[:M]].clone()
    od, oi = KN.knn_search(train.to(cuda), queries.to(cuda), k, q_tile=48, t_tile=128)
    od, oi = od.double().cpu(), oi.cpu()
    assert not torch.isnan(od).any() and (od >= 0).all() and (od[:, 1:] >= od[:, :-1]).all()
    assert ((oi >= 0) & (oi < n)).all()
    exact = (train[oi].double() - queries.double()[:, None, :]).pow(2).sum(-1)
    qq, tt = queries.double().pow(2).sum(1), train.double().pow(2).sum(1)
    bound = 2 * d * 2.0 ** -24 * (qq[:, None] + tt[oi])
    assert ((od - exact).abs() <= bound).all(), ((od - exact).abs() / bound).max()
