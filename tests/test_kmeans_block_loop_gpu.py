"""The resident grid of the narrow assign kernels (csrc/kmeans.hip): at most as many workgroups
as the device holds at once, each looping over the point blocks b, b + grid, ... The grid is
forced to 1, 2 and 3 workgroups, so that a workgroup runs several blocks in a row at sizes a test
can afford, and left on auto. Small-integer data (values in [0,16)) makes every product and sum
exact in bf16 / fp32, so labels, sums, distances and the objective must equal the fp64
first-occurrence argmin bit for bit. Runs only on a MI355X box."""
import functools

import pytest
import torch

from harp_amd.ops import kmeans as K

pytestmark = pytest.mark.gpu

KEYLESS, KEYED = 16, 15
GRIDS = [1, 2, 3, 0]  # 0: the resident grid


@pytest.fixture(autouse=True)
def _reset_grid():
    with torch.random.fork_rng(devices=[0] if torch.cuda.is_available() else []):
        yield
    K.set_resident_blocks(0)


@pytest.fixture(scope="module", autouse=True)
def _drop_cases():
    yield
    _case.cache_clear()
    _carried_case.cache_clear()


def _first_argmin(dist):
    k = dist.shape[1]
    idx = torch.arange(k, device=dist.device)[None, :].expand_as(dist)
    return torch.where(dist == dist.min(1, keepdim=True).values, idx, k).min(1).values


def _exact_sums(X, lab, rows, d):
    exact = torch.zeros((rows, d + 1), dtype=torch.float64, device=X.device)
    exact.index_add_(0, lab, X[:, : d + 1].double())
    return exact


@functools.lru_cache(maxsize=None)
def _case(n, k, d):
    """Seeded integer points and centroids with their fp64 reference, computed once per shape and
    shared by every grid: (X, operand, g = ||c||^2 - 2 x.c of every pair, first-occurrence
    argmin, exact sums of that labelling)."""
    cuda = torch.device("cuda", 0)
    gen = torch.Generator().manual_seed(n * 7919 + k * 31 + d)
    x = torch.randint(0, 16, (n, d), generator=gen).float().to(cuda)
    c = torch.randint(0, 16, (k, d), generator=gen).float().to(cuda)
    return _with_reference(x, c)


def _with_reference(x, c):
    d = x.shape[1]
    X = K.pack_points(x, x.device)
    op = K.prepare(c, X.shape[1])
    g = (c.double() ** 2).sum(1)[None, :] - 2.0 * (x.double() @ c.double().t())
    ref = _first_argmin(g)
    return X, op, g, ref, _exact_sums(X, ref, op.Cm2.shape[0], d)


def _assign_keyless(X, op, **kw):
    sums = torch.zeros((op.Cm2.shape[0], X.shape[1]), dtype=torch.float32, device=X.device)
    kw.setdefault("want_objective", False)
    lab, obj = K.assign(X, op, sums=sums, variant=KEYLESS, **kw)
    torch.cuda.synchronize()
    return lab.long(), obj, sums


# n -> one point; a block short of one point, one block, a block and a point; 4 blocks, the last
# ragged; 8 blocks, the last of one point (with a grid of 3 they run 3 / 3 / 2). k -> tail groups
# only; one stage; three stages + a tail tile, which sits in the LDS slot the next block's first
# tile overwrites; five stages. d -> 1, 7 and 8 k-steps (8 keeps the two-slot body)
@pytest.mark.parametrize("grid", GRIDS)
@pytest.mark.parametrize("d", [12, 100, 124])
@pytest.mark.parametrize("k", [96, 128, 416, 640])
@pytest.mark.parametrize("n", [1, 1023, 1024, 1025, 3 * 1024 + 31, 7 * 1024 + 1])
def test_exact_integer_data(cuda, n, k, d, grid):
    X, op, _, ref, exact = _case(n, k, d)
    K.set_resident_blocks(grid)
    lab, _, sums = _assign_keyless(X, op)
    assert torch.equal(lab, ref), (lab != ref).nonzero()[:8].flatten().tolist()
    assert torch.equal(sums[:, : d + 1].double(), exact)


@functools.lru_cache(maxsize=None)
def _carried_case():
    """Blocks 0 and 4 of 8 hold copies of centroid 5 = (15, ..., 15): their winning value
    ||c||^2 - 2 x.c = -22500 is far below anything the other blocks' points reach (copies of
    random rows of the groups 1 .., about -7750). Behind block 0 or 4 a workgroup of a grid of
    1, 2 or 3 runs one of the other blocks; a minimum carried over the block edge would keep
    group 0 for every point of it."""
    cuda = torch.device("cuda", 0)
    gen = torch.Generator().manual_seed(97)
    k, d, n = 416, 100, 7 * 1024 + 1
    c = torch.randint(0, 16, (k, d), generator=gen).float()
    c[5] = 15.0
    own = torch.randint(32, k, (n,), generator=gen)
    blk = torch.arange(n) // 1024
    own[(blk % 4) == 0] = 5
    return (own.to(cuda),) + _with_reference(c[own].to(cuda), c.to(cuda))


@pytest.mark.parametrize("grid", GRIDS)
def test_minimum_not_carried_over_a_block_edge(cuda, grid):
    own, X, op, _, ref, exact = _carried_case()
    assert torch.equal(ref, own)  # the rows are distinct: every point's nearest row is its own
    K.set_resident_blocks(grid)
    lab, _, sums = _assign_keyless(X, op)
    assert torch.equal(lab, ref), (lab != ref).nonzero()[:8].flatten().tolist()
    assert torch.equal(sums[:, :101].double(), exact)


@pytest.mark.parametrize("grid", GRIDS)
def test_keyless_objective_per_block(cuda, grid):
    """want_objective in the keyless kernel: one partial per point block, written at the block's
    own index by whichever workgroup ran it. Every partial is a sum of integers below 2^24."""
    X, op, g, ref, _ = _case(7 * 1024 + 1, 416, 100)
    dist = g.gather(1, ref[:, None])[:, 0] + (X[:, :100].double() ** 2).sum(1)
    assert float(dist.view(-1)[: 7 * 1024].view(7, 1024).sum(1).max()) < 2 ** 24
    K.set_resident_blocks(grid)
    _, obj, _ = _assign_keyless(X, op, want_objective=True)
    assert float(obj) == float(dist.sum())


def _keyed_checks(X, op, g, lab, d):
    """The keyed kernel takes the lower index on a tie only inside a 32 x 32 tile: where the
    minimum is unique the label is the reference's, everywhere it is a row at the minimum."""
    gmin = g.min(1).values
    assert torch.equal(g.gather(1, lab[:, None])[:, 0], gmin)
    unique = (g == gmin[:, None]).sum(1) == 1
    assert torch.equal(lab[unique], _first_argmin(g)[unique])
    return gmin + (X[:, :d].double() ** 2).sum(1)


@pytest.mark.parametrize("grid", GRIDS)
@pytest.mark.parametrize("n,k,d", [(7 * 1024 + 1, 416, 100), (3 * 1024 + 31, 640, 124), (7 * 1024 + 1, 96, 12)])
def test_keyed_objective_and_min_dist(cuda, n, k, d, grid):
    """min_dist set: the call runs variant 15 (the same template, the two-slot body). Labels, the
    bucketed sums, every squared distance and the objective (one partial per block, at the
    block's index) are exact."""
    X, op, g, _, _ = _case(n, k, d)
    K.set_resident_blocks(grid)
    sums = torch.zeros((op.Cm2.shape[0], X.shape[1]), dtype=torch.float32, device=cuda)
    md = torch.full((n,), -1.0, dtype=torch.float32, device=cuda)
    lab, obj = K.assign(X, op, sums=sums, variant=KEYLESS, want_objective=True, min_dist=md)
    torch.cuda.synchronize()
    lab = lab.long()
    dist = _keyed_checks(X, op, g, lab, d)
    assert torch.equal(sums[:, : d + 1].double(), _exact_sums(X, lab, sums.shape[0], d))
    assert torch.equal(md.double(), dist)
    nfull = n // 1024
    assert float(dist[: nfull * 1024].view(nfull, 1024).sum(1).max()) < 2 ** 24  # exact fp32 partials
    print("objective", float(obj), "exact", float(dist.sum()))
    assert float(obj) == float(dist.sum())


@pytest.mark.parametrize("grid", GRIDS)
@pytest.mark.parametrize("n,k,d", [(7 * 1024 + 1, 416, 100), (3 * 1024 + 31, 128, 12)])
def test_atomic_sums_exact(cuda, n, k, d, grid):
    """accumulate="atomic": the keyed kernel adds every block's rows itself, behind the block's
    epilogue; integer sums are exact in any order."""
    X, op, g, _, _ = _case(n, k, d)
    K.set_resident_blocks(grid)
    sums = torch.zeros((op.Cm2.shape[0], X.shape[1]), dtype=torch.float32, device=cuda)
    lab, _ = K.assign(X, op, sums=sums, variant=KEYED, want_objective=False, accumulate="atomic")
    torch.cuda.synchronize()
    lab = lab.long()
    _keyed_checks(X, op, g, lab, d)
    assert torch.equal(sums[:, : d + 1].double(), _exact_sums(X, lab, sums.shape[0], d))


def test_one_block_more_than_the_resident_grid(cuda):
    """Auto grid, one full and one ragged block more than it holds: workgroups 0 and 1 run a
    second block, every other one a single block."""
    k, d = 96, 12
    resident = K.resident_blocks(KEYLESS, K.padded_dim(d))
    assert resident >= 1
    n = (resident + 1) * 1024 + 5
    gen = torch.Generator().manual_seed(n)
    x = torch.randint(0, 16, (n, d), generator=gen).float().to(cuda)
    c = torch.randint(0, 16, (k, d), generator=gen).float().to(cuda)
    X, op, _, ref, exact = _with_reference(x, c)  # about 0.5 M points: not kept
    lab, _, sums = _assign_keyless(X, op)
    assert torch.equal(lab, ref), (lab != ref).nonzero()[:8].flatten().tolist()
    assert torch.equal(sums[:, : d + 1].double(), exact)


def test_resident_blocks_query(cuda):
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    for variant in (4, 13, 14, 15, 16):
        for ks in range(1, 9):
            r = K.resident_blocks(variant, 16 * ks)
            assert r >= cus and r % cus == 0, (variant, ks, r)
    assert K.resident_blocks(KEYLESS, 112) == cus  # 256 VGPRs, 84 KB of LDS: one workgroup per CU
    assert K.resident_blocks(99, 112) == -1 and K.resident_blocks(KEYLESS, 16 * 9) == -1
