"""K-means tail in one span-ordered pass: one counting sort by (span, 32-row group), one resolve
launch over the whole permutation that leaves each point's row in sorted order, and one streaming
pass that gathers the rows into the labels (csrc/segsum.hip harp_bucket_labels_spans,
csrc/kmeans_resolve.hip). A span is an ordering of the sort, so small spans (RESOLVE_SPAN forced
to 1024 .. 4096) put span edges inside 32-point windows and inside 2048-entry runs at tiny sizes.
Oracle as in test_kmeans_keyless_gpu.py: small-integer operands are exact in bf16 / fp32, so labels
must equal the fp64 first-occurrence argmin and the sums must be exact. Runs only on a MI355X box."""
import pytest
import torch

from harp_amd.ops import kmeans as K
from harp_amd.ops import segment

pytestmark = pytest.mark.gpu

KEYLESS, KEYED = 16, 15
SPANS = [1024, 2048, 4096]


@pytest.fixture(autouse=True)
def _keep_global_rng():
    with torch.random.fork_rng(devices=[0] if torch.cuda.is_available() else []):
        yield


def _run(X, op, variant, **kw):
    sums = torch.zeros((op.Cm2.shape[0], X.shape[1]), dtype=torch.float32, device=X.device)
    lab, obj = K.assign(X, op, sums=sums, variant=variant, **kw)
    torch.cuda.synchronize()
    return lab.long(), obj, sums


def _first_argmin(dist):
    k = dist.shape[1]
    idx = torch.arange(k, device=dist.device)[None, :].expand_as(dist)
    return torch.where(dist == dist.min(1, keepdim=True).values, idx, k).min(1).values


def _g(X, c_bf, d):
    return (c_bf.double() ** 2).sum(1)[None, :] - 2.0 * (X[:, :d].double() @ c_bf.double().t())


def _check_exact(x, c):
    cuda = x.device
    n, d = x.shape
    X = K.pack_points(x, cuda)
    op = K.prepare(c, X.shape[1])
    lab, _, sums = _run(X, op, KEYLESS)
    ref = _first_argmin(_g(X, c, d))
    assert torch.equal(lab, ref), (lab != ref).nonzero()[:8].flatten().tolist()
    exact = torch.zeros((sums.shape[0], d + 1), dtype=torch.float64, device=cuda)
    exact.index_add_(0, ref, X[:, : d + 1].double())
    assert torch.equal(sums[:, : d + 1].double(), exact)
    return lab


# a last span shorter than the others, a span edge inside a 32-point window (n = 1025 .. at span
# 1024 the window [1024, 1056) starts a span; 33 / 31 / 1 are single short windows) and inside a
# 2048-entry run (every n > 1024 at span 1024)
@pytest.mark.parametrize("span", SPANS)
@pytest.mark.parametrize("d", [12, 100, 124])
@pytest.mark.parametrize("k", [10, 33, 300, 1000])
@pytest.mark.parametrize("n", [1, 31, 33, 1023, 1024, 1025, 2047, 2049, 3 * 2048, 3 * 2048 + 1, 5000])
def test_exact_integer_data_small_spans(cuda, monkeypatch, n, k, d, span):
    monkeypatch.setattr(K, "RESOLVE_SPAN", span)
    g = torch.Generator().manual_seed(n * 7919 + k * 31 + d)
    x = torch.randint(0, 16, (n, d), generator=g).float().to(cuda)
    c = torch.randint(0, 16, (k, d), generator=g).float().to(cuda)
    _check_exact(x, c)


@pytest.mark.parametrize("span", SPANS)
@pytest.mark.parametrize("row", [3, 299])
def test_exact_every_point_in_one_group(cuda, monkeypatch, span, row):
    """First group / last group: every other bucket of every span is empty."""
    monkeypatch.setattr(K, "RESOLVE_SPAN", span)
    g = torch.Generator().manual_seed(11)
    c = torch.randint(0, 16, (300, 100), generator=g).float()
    x = c[row].repeat(5000, 1)
    lab = _check_exact(x.to(cuda), c.to(cuda))
    assert bool((lab // 32 == row // 32).all())


@pytest.mark.parametrize("span", SPANS)
def test_exact_group_empty_in_one_span_full_in_next(cuda, monkeypatch, span):
    """Span s holds only points of group s % 4 (so each group is empty in three spans of four and
    owns the whole fourth), then a mixed tail: the same group in neighbouring non-empty buckets
    of different spans, and bucket walks over many empty buckets."""
    monkeypatch.setattr(K, "RESOLVE_SPAN", span)
    g = torch.Generator().manual_seed(12)
    k, d = 128, 12
    c = torch.stack([torch.tensor([(i >> (4 * j)) & 15 for j in range(d)]) for i in range(1, k + 1)]).float()
    parts = [torch.randint(32 * (s % 4), 32 * (s % 4) + 32, (span,), generator=g) for s in range(5)]
    parts.append(torch.randint(0, k, (777,), generator=g))
    own = torch.cat(parts)
    x = c[own]  # every point sits on its (distinct) centroid
    X = K.pack_points(x.to(cuda), cuda)
    op = K.prepare(c.to(cuda), X.shape[1])
    lab, _, _ = _run(X, op, KEYLESS)
    assert torch.equal(lab.cpu(), own)
    _check_exact(x.to(cuda), c.to(cuda))


@pytest.mark.parametrize("span", SPANS)
def test_exact_duplicate_centroids_lowest_index(cuda, monkeypatch, span):
    monkeypatch.setattr(K, "RESOLVE_SPAN", span)
    g = torch.Generator().manual_seed(5)
    n, k, d = 5000, 300, 60
    c = torch.randint(0, 16, (k, d), generator=g).float()
    c[40] = c[5]      # same 32-row group
    c[200] = c[5]     # another group
    c[299] = c[150]
    x = torch.randint(0, 16, (n, d), generator=g).float()
    x[900:1400] = c[5]    # exactly on the duplicated row, across the first edge of a 1024 span
    x[4000:4200] = c[150]
    X = K.pack_points(x.to(cuda), cuda)
    op = K.prepare(c.to(cuda), X.shape[1])
    lab, _, _ = _run(X, op, KEYLESS)
    assert bool((lab[900:1400] == 5).all()) and bool((lab[4000:4200] == 150).all())
    _check_exact(x.to(cuda), c.to(cuda))


# bucketing alone. (n, NG, span): the K-means knobs; then chunks above the 4096 floor with two
# column-scan segments per span (128 chunks per span), at chunk 4096 and at chunk 8192
BUCKET_CASES = [(n, ng, s) for s in SPANS for ng in (1, 10, 313)
                for n in (1, 31, 1023, 1024, 1025, 2049, 3 * 2048 + 1, 5000)]
BUCKET_CASES += [(3 * (1 << 19) + 5, 313, 1 << 19), (12_600_000, 40, 1 << 20), (70_001, 7, 1 << 16)]


@pytest.mark.parametrize("n,ng,span", BUCKET_CASES)
def test_bucket_labels_spans(cuda, n, ng, span):
    g = torch.Generator().manual_seed(n + ng + span)
    lab = torch.randint(0, ng, (n,), generator=g, dtype=torch.int32).to(cuda)
    if n > 4096:
        lab[span // 2: span // 2 + 3000] = ng - 1  # a skewed stretch
    perm, start, rank, rowof = segment.bucket_labels_spans(lab, ng, span, want_rank=True)
    torch.cuda.synchronize()
    nspans = (n + span - 1) // span
    ar = torch.arange(n, device=cuda)
    assert perm.numel() == n and start.numel() == nspans * ng + 1 and rowof.numel() == n
    assert torch.equal(perm.long().sort().values, ar)          # a permutation of 0..n-1
    assert torch.equal(rank.long()[perm.long()], ar)            # rank[perm[j]] == j
    key = ar // span * ng + lab.long()                          # bucket of every point
    ref = torch.zeros(nspans * ng + 1, dtype=torch.int64, device=cuda)
    ref[1:] = torch.cumsum(torch.bincount(key, minlength=nspans * ng), 0)
    assert torch.equal(start.long(), ref) and int(start[-1]) == n and bool((start[1:] >= start[:-1]).all())
    # every perm[start[q]:start[q+1]] lies in span q // NG and has group q % NG
    q = torch.repeat_interleave(torch.arange(nspans * ng, device=cuda), ref[1:] - ref[:-1])
    assert torch.equal(key[perm.long()], q)
    # without rank: the same sort (it reuses the workspace, so compare with the reference again)
    perm2, start2 = segment.bucket_labels_spans(lab, ng, span)
    torch.cuda.synchronize()
    assert torch.equal(start2.long(), ref) and torch.equal(key[perm2.long()], q)


def test_bucket_labels_spans_rejects_bad_span(cuda):
    lab = torch.zeros(5000, dtype=torch.int32, device=cuda)
    for span in (512, 3000):
        with pytest.raises(ValueError):
            segment.bucket_labels_spans(lab, 4, span)


@pytest.mark.parametrize("off", [0, 1])  # 1: not 16-byte aligned, the scalar kernel
@pytest.mark.parametrize("n", [1, 3, 4, 5, 1027, 4096])
def test_finish_labels(cuda, n, off):
    g = torch.Generator().manual_seed(n)
    group = torch.randint(0, 313, (n,), generator=g, dtype=torch.int32)
    rank = torch.randperm(n, generator=g).to(torch.int32)
    rowof = torch.randint(0, 32, (n,), generator=g, dtype=torch.uint8)
    want = 32 * group.long() + rowof.long()[rank.long()]
    lab = torch.full((n + 2,), -7, dtype=torch.int32, device=cuda)
    rk = torch.zeros(n + 2, dtype=torch.int32, device=cuda)
    lab[off:off + n] = group.to(cuda)
    rk[off:off + n] = rank.to(cuda)
    segment.finish_labels(lab[off:off + n], rk[off:off + n], rowof.to(cuda))
    torch.cuda.synchronize()
    assert torch.equal(lab[off:off + n].long().cpu(), want)
    assert bool((lab[:off] == -7).all()) and bool((lab[off + n:] == -7).all())  # nothing written outside


def test_random_matches_oracle_and_keyed_small_span(cuda, monkeypatch):
    """n = 200,000 in 49 spans of 4096 against the keyed variant 15: differing labels are near
    ties (the bound of test_kmeans_keyless_gpu.py), untouched clusters' sums agree."""
    monkeypatch.setattr(K, "RESOLVE_SPAN", 4096)
    n, d, k = 200000, 100, 2000
    torch.manual_seed(0)
    x = torch.rand(n, d, device=cuda) * 1000
    X = K.pack_points(x, cuda)
    c = torch.rand(k, d, device=cuda) * 1000
    op = K.prepare(c, X.shape[1])
    lab, obj, sums = _run(X, op, KEYLESS)
    lab15, obj15, sums15 = _run(X, op, KEYED)
    c_bf = c.to(torch.bfloat16).float()
    dist = _g(X, c_bf, d)
    rlab = dist.argmin(1)
    assert int(lab.min()) >= 0 and int(lab.max()) < k
    chosen = dist.gather(1, lab[:, None])[:, 0]
    best = dist.gather(1, rlab[:, None])[:, 0]
    xs = (X[:, :d].double() ** 2).sum(1)
    scale = xs + (c_bf.double() ** 2).sum(1).max()
    assert bool(((chosen - best) <= 1e-5 * scale).all())
    assert (lab == rlab).float().mean().item() > 0.99
    diff = lab != lab15
    ga = chosen[diff]
    gb = dist.gather(1, lab15[:, None])[:, 0][diff]
    print(f"labels differing from variant 15: {int(diff.sum())} of {n}")
    assert bool(((ga - gb).abs() <= 2.0 ** -17 * ga.abs()).all())
    touched = torch.zeros(sums.shape[0], dtype=torch.bool, device=cuda)
    touched[lab[diff]] = True
    touched[lab15[diff]] = True
    assert torch.allclose(sums[~touched][:, : d + 1], sums15[~touched][:, : d + 1], rtol=1e-5, atol=1e-2)
    ref = torch.zeros_like(sums, dtype=torch.float64)
    ref[:, : d + 1].index_add_(0, lab, X[:, : d + 1].double())
    assert torch.allclose(sums[:, : d + 1].double(), ref[:, : d + 1], rtol=1e-5, atol=1e-2)
    assert int(sums[:, d].sum().item()) == n
    assert abs(obj.item() - obj15.item()) <= 1e-4 * abs(obj15.item()) + 1e-3


def test_span_size_does_not_change_labels(cuda, monkeypatch):
    """Random data: the span only orders the sort, so labels are equal for every span and the
    sums agree to rounding."""
    n, d, k = 50000, 100, 700
    torch.manual_seed(4)
    X = K.pack_points(torch.rand(n, d, device=cuda) * 1000, cuda)
    op = K.prepare(torch.rand(k, d, device=cuda) * 1000, X.shape[1])
    out = {}
    for span in (1024, 4096, 1 << 23):
        monkeypatch.setattr(K, "RESOLVE_SPAN", span)
        lab, _, sums = _run(X, op, KEYLESS)
        out[span] = (lab, sums)
    for span in (1024, 4096):
        assert torch.equal(out[span][0], out[1 << 23][0])
        assert torch.allclose(out[span][1], out[1 << 23][1], rtol=1e-5, atol=1e-2)


def test_chunked_side_stream_matches_single_pass_small_span(cuda, monkeypatch):
    monkeypatch.setattr(K, "RESOLVE_SPAN", 4096)
    n, d, k = 1024 * 256 * 2 + 777, 100, 500
    torch.manual_seed(1)
    X = K.pack_points(torch.rand(n, d, device=cuda) * 1000, cuda)
    op = K.prepare(torch.rand(k, d, device=cuda) * 1000, X.shape[1])
    out = {}
    for c in (1, 2):
        monkeypatch.setenv("HARP_KMEANS_CHUNKS", str(c))
        lab, obj, sums = _run(X, op, KEYLESS)
        out[c] = (lab.clone(), sums)
    assert K.pipeline_chunks(n, 1024) == 2
    a, b = out[1], out[2]
    assert int(a[0].max()) < k and torch.equal(a[0], b[0])
    assert torch.allclose(a[1], b[1], rtol=1e-5, atol=1e-2)
    assert int(b[1][:, d].sum().item()) == n


def test_hip_graph_iteration_matches_eager_small_span(cuda, monkeypatch):
    from harp_amd.models.kmeans import KMeansCollectiveMapper, KMeansConfig
    from harp_amd.parallel.comm import Communicator
    from harp_amd.runtime.mapper import KeyValReader

    monkeypatch.setattr(K, "RESOLVE_SPAN", 2048)
    out = {}
    for graph in (False, True):
        cfg = KMeansConfig(num_points=50000, num_centroids=300, dim=100, iterations=1, strategy="allreduce",
                           objective_every=0, graph=graph, variant=KEYLESS)
        m = KMeansCollectiveMapper(Communicator(None, cuda), cfg)
        m.init_model(KeyValReader([]))
        m.step(0)
        torch.cuda.synchronize()
        out[graph] = (m.c[:300].clone(), m.lab.clone())
    assert torch.equal(out[True][1], out[False][1])
    assert torch.allclose(out[True][0], out[False][0], rtol=1e-5, atol=1e-3)
