"""Keyless K-means assign (variant 16): the sweep finds the winning 32-row centroid group, the
bucketed gather-sum pass resolves the row inside it (csrc/kmeans_resolve.hip). Exact integer
data must give the fp64 first-occurrence argmin bit for bit; random data may differ from the
keyed kernel (variant 15) only at near ties. Runs only on a MI355X box."""
import pytest
import torch

from harp_amd.ops import kmeans as K

pytestmark = pytest.mark.gpu

KEYLESS, KEYED = 16, 15


@pytest.fixture(autouse=True)
def _keep_global_rng():
    """These tests seed the global generators (the data of test_assign_matches_torch); put the
    generators back afterwards, so tests later in the suite that draw unseeded data see the
    stream they saw before this file existed."""
    with torch.random.fork_rng(devices=[0] if torch.cuda.is_available() else []):
        yield


def _run(X, op, variant, **kw):
    sums = torch.zeros((op.Cm2.shape[0], X.shape[1]), dtype=torch.float32, device=X.device)
    lab, obj = K.assign(X, op, sums=sums, variant=variant, **kw)
    torch.cuda.synchronize()
    return lab.long(), obj, sums


def _first_argmin(dist):
    """First-occurrence argmin, spelled out (lowest index among the exact minima)."""
    k = dist.shape[1]
    idx = torch.arange(k, device=dist.device)[None, :].expand_as(dist)
    return torch.where(dist == dist.min(1, keepdim=True).values, idx, k).min(1).values


def _g(X, c_bf, d):
    """g = ||c||^2 - 2 x.c in fp64 from the bf16-rounded operands."""
    return (c_bf.double() ** 2).sum(1)[None, :] - 2.0 * (X[:, :d].double() @ c_bf.double().t())


def _check_exact(x, c):
    """Small-integer operands: every product and sum is exact in bf16 / fp32."""
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


@pytest.mark.parametrize("d", [1, 12, 60, 100, 124])
@pytest.mark.parametrize("k", [10, 33, 129, 300, 1000])
@pytest.mark.parametrize("n", [1, 33, 1025, 5000])
def test_exact_integer_data(cuda, n, k, d):
    g = torch.Generator().manual_seed(n * 7919 + k * 31 + d)
    x = torch.randint(0, 16, (n, d), generator=g).float().to(cuda)
    c = torch.randint(0, 16, (k, d), generator=g).float().to(cuda)
    _check_exact(x, c)


def test_exact_duplicate_centroids_lowest_index(cuda):
    g = torch.Generator().manual_seed(5)
    n, k, d = 3000, 300, 60
    c = torch.randint(0, 16, (k, d), generator=g).float()
    c[40] = c[5]      # same 32-row group
    c[200] = c[5]     # another group
    c[299] = c[150]
    x = torch.randint(0, 16, (n, d), generator=g).float()
    x[:500] = c[5]    # exactly on the duplicated row
    x[500:700] = c[150]
    X = K.pack_points(x.to(cuda), cuda)
    op = K.prepare(c.to(cuda), X.shape[1])
    lab, _, _ = _run(X, op, KEYLESS)
    assert bool((lab[:500] == 5).all()) and bool((lab[500:700] == 150).all())
    _check_exact(x.to(cuda), c.to(cuda))


def test_exact_all_points_identical(cuda):
    g = torch.Generator().manual_seed(6)
    n, k, d = 5000, 300, 100
    c = torch.randint(0, 16, (k, d), generator=g).float()
    x = c[77].repeat(n, 1)  # one group (and one row) gets every point
    _check_exact(x.to(cuda), c.to(cuda))


def test_exact_group_boundary_inside_chunk(cuda):
    """Two groups: the first gets 45 points (its boundary falls inside the second 32-point
    chunk), the second 2100, so the second also crosses into the next wave's run of the
    sorted permutation (2048 entries per wave)."""
    g = torch.Generator().manual_seed(7)
    k, d = 64, 12
    c = torch.stack([torch.tensor([(i >> (4 * j)) & 15 for j in range(d)]) for i in range(1, k + 1)]).float()
    own = torch.cat([torch.randint(0, 32, (45,), generator=g), torch.randint(32, 64, (2100,), generator=g)])
    own = own[torch.randperm(own.numel(), generator=g)]
    x = c[own]  # every point sits on its (distinct) centroid
    X = K.pack_points(x.to(cuda), cuda)
    op = K.prepare(c.to(cuda), X.shape[1])
    lab, _, sums = _run(X, op, KEYLESS)
    assert torch.equal(lab.cpu(), own)
    assert int(sums[:32, d].sum().item()) == 45 and int(sums[32:64, d].sum().item()) == 2100
    _check_exact(x.to(cuda), c.to(cuda))


def test_exact_several_spans(cuda, monkeypatch):
    """The bucket + resolve pass runs over spans of points (RESOLVE_SPAN); here three, the
    last one shorter, sharing one workspace."""
    monkeypatch.setattr(K, "RESOLVE_SPAN", 2048)
    g = torch.Generator().manual_seed(8)
    x = torch.randint(0, 16, (5000, 100), generator=g).float().to(cuda)
    c = torch.randint(0, 16, (300, 100), generator=g).float().to(cuda)
    _check_exact(x, c)


RANDOM_SHAPES = [(5000, 100, 300), (777, 10, 10), (4099, 31, 129), (2048, 127, 1000), (1500, 250, 200),
                 (200000, 100, 2000)]


@pytest.mark.parametrize("n,d,k", RANDOM_SHAPES)
def test_random_matches_oracle_and_keyed(cuda, n, d, k):
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
    agree = (lab == rlab).float().mean().item()
    print(f"agreement with the fp64 argmin: {agree:.6f}")
    assert agree > 0.99
    robj = (best + xs).sum().item()
    assert abs(obj.item() - robj) <= 1e-4 * abs(robj) + 1e-3
    # against the keyed kernel: every differing label is a near tie (two 2^-19 key
    # perturbations plus fp32 accumulation slack)
    diff = lab != lab15
    ga = chosen[diff]
    gb = dist.gather(1, lab15[:, None])[:, 0][diff]
    print(f"labels differing from variant 15: {int(diff.sum())} of {n}; max |dg|/|g| = "
          f"{((ga - gb).abs() / ga.abs()).max().item() if diff.any() else 0.0:.3e}")
    assert bool(((ga - gb).abs() <= 2.0 ** -17 * ga.abs()).all())
    # sums rows of clusters that no differing point touches agree with the keyed path
    touched = torch.zeros(sums.shape[0], dtype=torch.bool, device=cuda)
    touched[lab[diff]] = True
    touched[lab15[diff]] = True
    assert torch.allclose(sums[~touched][:, : d + 1], sums15[~touched][:, : d + 1], rtol=1e-5, atol=1e-2)
    ref = torch.zeros_like(sums, dtype=torch.float64)
    ref[:, : d + 1].index_add_(0, lab, X[:, : d + 1].double())
    assert torch.allclose(sums[:, : d + 1].double(), ref[:, : d + 1], rtol=1e-5, atol=1e-2)
    assert int(sums[:, d].sum().item()) == n
    assert abs(obj.item() - obj15.item()) <= 1e-4 * abs(obj15.item()) + 1e-3


def test_objective_and_min_dist_match_keyed(cuda):
    n, d, k = 20000, 100, 700
    torch.manual_seed(3)
    X = K.pack_points(torch.rand(n, d, device=cuda) * 1000, cuda)
    op = K.prepare(torch.rand(k, d, device=cuda) * 1000, X.shape[1])
    out = {}
    for v in (KEYED, KEYLESS):
        md = torch.empty(n, dtype=torch.float32, device=cuda)
        _, obj, _ = _run(X, op, v)                    # the bucketed path (keyless sweep + resolve at 16)
        lab_md, obj_md, _ = _run(X, op, v, min_dist=md)  # min_dist: both run the keyed kernel
        _, obj_ns = K.assign(X, op, variant=v)        # no sums
        torch.cuda.synchronize()
        out[v] = (obj.item(), obj_md.item(), obj_ns.item(), md, lab_md)
    a, b = out[KEYED], out[KEYLESS]
    for i in range(3):
        assert abs(a[i] - b[i]) <= 1e-4 * abs(a[i]) + 1e-3
    assert torch.allclose(a[3].double(), b[3].double(), rtol=1e-4, atol=1.0)
    assert int(b[4].min()) >= 0 and int(b[4].max()) < k


def test_chunked_side_stream_matches_single_pass(cuda, monkeypatch):
    n, d, k = 1024 * 256 * 4 + 777, 100, 500
    torch.manual_seed(1)
    X = K.pack_points(torch.rand(n, d, device=cuda) * 1000, cuda)
    op = K.prepare(torch.rand(k, d, device=cuda) * 1000, X.shape[1])
    out = {}
    for c in (1, 4):
        monkeypatch.setenv("HARP_KMEANS_CHUNKS", str(c))
        lab, obj, sums = _run(X, op, KEYLESS)
        out[c] = (lab.clone(), obj.item(), sums)
    assert K.pipeline_chunks(n, 1024) == 4
    a, b = out[1], out[4]
    assert int(a[0].max()) < k and torch.equal(a[0], b[0])
    assert b[1] == pytest.approx(a[1], rel=1e-9)
    assert torch.allclose(a[2], b[2], rtol=1e-5, atol=1e-2)
    assert int(b[2][:, d].sum().item()) == n


def test_hip_graph_iteration_matches_eager(cuda):
    from harp_amd.models.kmeans import KMeansCollectiveMapper, KMeansConfig
    from harp_amd.parallel.comm import Communicator
    from harp_amd.runtime.mapper import KeyValReader

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


def test_kmeans_model_gpu_matches_cpu_keyless(cuda):
    from harp_amd.models.kmeans import KMeansConfig, run_kmeans
    from harp_amd.parallel.comm import Communicator

    assert K.DEFAULT_VARIANT == KEYLESS
    g = torch.Generator().manual_seed(1)
    x = torch.rand(20000, 20, generator=g) * 10
    c0 = torch.rand(16, 20, generator=g) * 10
    cfg = KMeansConfig(num_points=20000, num_centroids=16, dim=20, iterations=20, strategy="allreduce",
                       variant=KEYLESS)
    gpu = run_kmeans(Communicator(None, cuda), cfg, points=x, init_centroids=c0)
    cpu = run_kmeans(Communicator(None, torch.device("cpu")), cfg, points=x, init_centroids=c0)
    md_g = torch.cdist(x, gpu["centroids"]).min(1).values.mean()
    md_c = torch.cdist(x, cpu["centroids"]).min(1).values.mean()
    assert abs(md_g - md_c) / md_c < 5e-3, (md_g, md_c)
    obj = gpu["objective"]
    assert obj[-1] <= obj[0]
