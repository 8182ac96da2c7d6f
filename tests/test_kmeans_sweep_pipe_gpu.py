"""Hand-over points of the keyless sweep's software pipeline (csrc/kmeans.hip, variant 16): the
MFMA chain of item i+1 starts ahead of the min epilogue of item i, and the epilogue's min chain
starts from the running best itself. Small-integer data (values in [0,16)) makes every product
and sum exact in bf16 / fp32, so labels and sums must equal the fp64 first-occurrence argmin
bit for bit. Runs only on a MI355X box."""
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


def _run_exact(x, c):
    """Labels of the keyless path; asserts labels and sums against the fp64 reference."""
    cuda = x.device
    n, d = x.shape
    X = K.pack_points(x, cuda)
    op = K.prepare(c, X.shape[1])
    sums = torch.zeros((op.Cm2.shape[0], X.shape[1]), dtype=torch.float32, device=cuda)
    lab, _ = K.assign(X, op, sums=sums, variant=KEYLESS)
    torch.cuda.synchronize()
    lab = lab.long()
    g = (c.double() ** 2).sum(1)[None, :] - 2.0 * (X[:, :d].double() @ c.double().t())
    ref = _first_argmin(g)
    assert torch.equal(lab, ref), (lab != ref).nonzero()[:8].flatten().tolist()
    exact = torch.zeros((sums.shape[0], d + 1), dtype=torch.float64, device=cuda)
    exact.index_add_(0, ref, X[:, : d + 1].double())
    assert torch.equal(sums[:, : d + 1].double(), exact)
    return lab


# d -> k-steps 1, 1, 2, 7, 8 (from chains of one MFMA to the longest the default tiling runs);
# k -> tail only; one full stage, no next DMA; full stage + one tail group; two full stages;
# two full stages + three tail groups; n -> one point, a partial group, one workgroup, one
# workgroup and a partial group of the next
@pytest.mark.parametrize("d", [1, 12, 20, 100, 124])
@pytest.mark.parametrize("k", [32, 128, 160, 256, 352])
@pytest.mark.parametrize("n", [1, 31, 1024, 1057])
def test_exact_integer_data(cuda, n, k, d):
    g = torch.Generator().manual_seed(n * 7919 + k * 31 + d)
    x = torch.randint(0, 16, (n, d), generator=g).float().to(cuda)
    c = torch.randint(0, 16, (k, d), generator=g).float().to(cuda)
    _run_exact(x, c)


@pytest.mark.parametrize("d", [12, 20, 100, 124])
@pytest.mark.parametrize("k", [128, 352])
def test_planted_winner_every_group_and_item(cuda, k, d):
    """Every 32-point block sits exactly on one centroid; over the 24 full waves every
    32-row group j meets every point group g of a wave, so also the first (row group 0, g = 0)
    and the last (row group 3, g = 3) item of a stage. The planted row has an identical copy
    at a higher index (in the next group; for the last group, later in the same one): the label
    must be the lower of the two. An epilogue that reads an accumulator before its chain has
    finished, or a dropped epilogue at the pipeline drain, gives another row."""
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
    lab = _run_exact(x.to(cuda), c.to(cuda))
    assert torch.equal(lab.cpu(), torch.tensor(expect)[own])
