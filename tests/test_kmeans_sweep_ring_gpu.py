"""The ring form of the keyless sweep (csrc/kmeans.hip, variant 16): three LDS slots, one barrier
inside each stage, the pieces of the tile two stages ahead requested one per item, and the item
pipeline carried over the stage edge. Small-integer data (values in [0,16)) makes every product
and sum exact in bf16 / fp32, so labels, sums, distances and the objective must equal the fp64
first-occurrence argmin bit for bit. Runs only on a MI355X box."""
import pytest
import torch

from harp_amd.ops import kmeans as K

pytestmark = pytest.mark.gpu

KEYLESS = 16


@pytest.fixture(autouse=True)
def _keep_global_rng():
    with torch.random.fork_rng(devices=[0] if torch.cuda.is_available() else []):
        yield


def _first_argmin(dist):
    k = dist.shape[1]
    idx = torch.arange(k, device=dist.device)[None, :].expand_as(dist)
    return torch.where(dist == dist.min(1, keepdim=True).values, idx, k).min(1).values


def _reference(X, c, d):
    """fp64: (first-occurrence argmin, ||c||^2 - 2 x.c of every pair)."""
    g = (c.double() ** 2).sum(1)[None, :] - 2.0 * (X[:, :d].double() @ c.double().t())
    return _first_argmin(g), g


def _run_exact(x, c, **kw):
    """Labels of the keyless path; asserts labels and sums against the fp64 reference. Returns
    (labels, objective, reference labels, reference squared distances to the chosen centroid)."""
    cuda = x.device
    n, d = x.shape
    X = K.pack_points(x, cuda)
    op = K.prepare(c, X.shape[1])
    sums = torch.zeros((op.Cm2.shape[0], X.shape[1]), dtype=torch.float32, device=cuda)
    kw.setdefault("want_objective", False)
    lab, obj = K.assign(X, op, sums=sums, variant=KEYLESS, **kw)
    torch.cuda.synchronize()
    lab = lab.long()
    ref, g = _reference(X, c, d)
    assert torch.equal(lab, ref), (lab != ref).nonzero()[:8].flatten().tolist()
    exact = torch.zeros((sums.shape[0], d + 1), dtype=torch.float64, device=cuda)
    exact.index_add_(0, ref, X[:, : d + 1].double())
    assert torch.equal(sums[:, : d + 1].double(), exact)
    dist = g.gather(1, ref[:, None])[:, 0] + (X[:, :d].double() ** 2).sum(1)
    return lab, obj, ref, dist


# d -> k-steps 1, 1, 7, 8 (8 keeps the two-slot body); k -> tail groups only, no full stage; one
# stage, nothing to prefetch; two stages: the request past the last tile; exactly three stages:
# every slot used once; three stages + one tail group; four stages: the first slot reuse; five
# stages; seven stages + two tail groups: each slot reused twice, then the tail; n -> one point,
# a partial group, one workgroup, one workgroup and a partial group of the next
@pytest.mark.parametrize("d", [1, 12, 100, 124])
@pytest.mark.parametrize("k", [96, 128, 256, 384, 416, 512, 640, 960])
@pytest.mark.parametrize("n", [1, 31, 1024, 1057])
def test_exact_integer_data(cuda, n, k, d):
    g = torch.Generator().manual_seed(n * 7919 + k * 31 + d)
    x = torch.randint(0, 16, (n, d), generator=g).float().to(cuda)
    c = torch.randint(0, 16, (k, d), generator=g).float().to(cuda)
    _run_exact(x, c)


@pytest.mark.parametrize("d", [20, 100])
@pytest.mark.parametrize("k", [416, 640])
def test_planted_winner_every_group_and_item(cuda, k, d):
    """Every 32-point block sits exactly on one centroid; over the 24 full waves every 32-row
    group j meets every point group g of a wave, so also the item whose epilogue crosses a stage
    edge (row group 3, g = 3: its epilogue runs behind the first chain of the next stage) and the
    first item of a stage (row group 0, g = 0: its chain starts in front of that edge). The
    planted row has an identical copy at a higher index (in the next group; for the last group,
    later in the same one): the label must be the lower of the two. A dropped or early epilogue
    at the edge gives another row."""
    gen = torch.Generator().manual_seed(k * 131 + d)
    groups = k // 32
    c = torch.randint(0, 16, (k, d), generator=gen).float()
    planted = [32 * j + (5 * j + 1) % 32 for j in range(groups)]
    expect = []
    for j, row in enumerate(planted):
        if j + 1 < groups:
            dup = 32 * (j + 1) + ((5 * (j + 1) + 1) % 32 + 16) % 32  # not the next group's planted row
        else:
            dup = 32 * j + ((5 * j + 1) % 32 + 8) % 32  # nor the copy the group before put here
        c[dup] = c[row]
        expect.append(min(row, dup))
    assert len(set(planted)) == groups and torch.unique(c, dim=0).shape[0] == k - groups  # only the planted copies
    n = 3 * 1024 + 33
    blocks = (n + 31) // 32
    own = torch.empty(n, dtype=torch.long)
    seen = set()
    for b in range(blocks):
        wave, g = b // 4, b % 4
        j = (wave + 3 * g) % groups
        own[32 * b: 32 * b + 32] = j
        if b < 96:
            seen.add((j, g))
    assert len(seen) == 4 * groups  # every (row group, point group) pair occurs in a full workgroup
    x = c[torch.tensor(planted)[own]]
    lab = _run_exact(x.to(cuda), c.to(cuda))[0]
    assert torch.equal(lab.cpu(), torch.tensor(expect)[own])


def _epilogue_case(cuda):
    # five stages and a tail group at 7 k-steps; a workgroup, and a partial group of the next.
    # The seed is one at which no point has two centroids at its smallest distance: on a tie the
    # keyed kernel takes the lower index only inside a 32 x 32 tile, not across tiles
    g = torch.Generator().manual_seed(4266)
    x = torch.randint(0, 16, (1057, 100), generator=g).float().to(cuda)
    c = torch.randint(0, 16, (672, 100), generator=g).float().to(cuda)
    dist = (c.double() ** 2).sum(1)[None, :] - 2.0 * (x.double() @ c.double().t())
    assert int(((dist == dist.min(1, keepdim=True).values).sum(1) > 1).sum()) == 0
    return x, c


def test_objective_exact(cuda):
    """want_objective: the keyless kernel's epilogue adds ||x||^2 to the winning value. Every
    workgroup partial is a sum of integers that stays below 2^24, so fp32 adds it exactly."""
    x, c = _epilogue_case(cuda)
    _, obj, _, dist = _run_exact(x, c, want_objective=True)
    assert float(dist[:1024].sum()) < 2 ** 24  # the precondition of an exact fp32 partial
    print("objective", float(obj), "exact", float(dist.sum()))
    assert float(obj) == float(dist.sum())


def test_min_dist_exact(cuda):
    """min_dist set: the call runs the keyed variant 15 (the same kernel template and epilogue);
    labels, sums and every squared distance are exact."""
    x, c = _epilogue_case(cuda)
    md = torch.full((x.shape[0],), -1.0, dtype=torch.float32, device=cuda)
    _, _, _, dist = _run_exact(x, c, min_dist=md)
    err = (md.double() - dist).abs()
    print("min_dist largest error", float(err.max()), "points off", int((err > 0).sum()))
    assert torch.equal(md.double(), dist)
