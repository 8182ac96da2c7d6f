"""Radix-select kernels (``csrc/quantile.hip``) against their torch mirror in
``harp_amd/ops/quantile.py`` (run on CPU tensors): every pass's integer histogram and every pick
must be equal, with prefixes taken from a real select run; then select against a device sort,
quantiles against ``torch.quantile`` on the device, a block above torch's size limit, the
promised memory bound and repeatability."""
import pytest
import torch

from harp_amd.models import stats as ST
from harp_amd.ops import quantile as QT

pytestmark = pytest.mark.gpu

DTYPES = (torch.bfloat16, torch.float32, torch.float64)
IDS = ("bf16", "fp32", "fp64")
CHUNK = QT.CHUNK
NS = (1, CHUNK - 1, CHUNK, CHUNK + 1, 3 * CHUNK + 7)
Q = (0, 0.1, 0.25, 0.5, 0.75, 0.9, 0.999, 1)


def widths(dtype):
    C = QT.COLUMN_GROUP[dtype]
    return (1, C - 1, C, C + 1, 65)


def data(n, d, dtype, seed=0):
    """(W, c): the block is W[:, c:c + d]. Quarter-integer normals (ties, so the later passes still
    match rows), a constant column, a two-valued column, both zeros, an infinity. With an odd
    ``seed`` W is 5 columns wider than the block (row stride > d)."""
    g = torch.Generator().manual_seed(seed * 7919 + n * 31 + d)
    c = 3 if seed % 2 else 0
    W = ((torch.randn(n, d + 5 if seed % 2 else d, generator=g, dtype=torch.float64) * 4).round() / 4).to(dtype)
    X = W[:, c:c + d]
    X[X == 0.5] = -0.0
    X[:, d // 2] = -2.75
    if d > 2:
        X[:, d - 1] = torch.where(torch.rand(n, generator=g) < 0.5, 1.0, 1.0 + 2.0 ** -6).to(dtype)
    if n > 5:
        X[5, :] = float("inf")
    return W, c


def spread(n, T):
    return [n // 2] if T == 1 else [(n - 1) * k // (T - 1) for k in range(T)]


def mirror_run(X, ranks):
    """The CPU select, pass by pass: [(prefix before the pass, hist, nan, prefix after, remaining
    after)] and the values."""
    d, T = X.shape[1], len(ranks)
    prefix = torch.zeros((d, T), dtype=torch.int64)
    remaining = torch.tensor(ranks, dtype=torch.int64).repeat(d, 1)
    steps, nan0, out = [], None, None
    for p in range(QT.passes(X.dtype)):
        before = prefix.clone()
        hist, nan = QT.digit_histogram(X, prefix, p)
        nan0 = nan if p == 0 else nan0
        out = QT.pick(hist, prefix, remaining, p, X.dtype, nan0)
        steps.append((before, hist, nan, prefix.clone(), remaining.clone()))
    return steps, out


def check_against_mirror(cuda, W, c, d, ranks, flags=0):
    """W[:, c:c + d] on the device (sliced there: the view keeps W's row stride) against the
    mirror on the CPU."""
    X = W[:, c:c + d]
    steps, want = mirror_run(X, ranks)
    Xd = W.to(cuda)[:, c:c + d]
    assert Xd.stride() == X.stride()
    nan0 = out = None
    for p, (before, hist, nan, prefix_after, remaining_after) in enumerate(steps):
        got, got_nan = QT.digit_histogram(Xd, before.to(cuda), p, flags)
        assert got.dtype == torch.int64 and torch.equal(got.cpu(), hist), (p, tuple(X.shape))
        if p == 0:
            assert torch.equal(got_nan.cpu(), nan)
            nan0 = got_nan
            remaining = torch.tensor(ranks, dtype=torch.int64, device=cuda).repeat(X.shape[1], 1)
        prefix = before.to(cuda)
        out = QT.pick(got, prefix, remaining, p, X.dtype, nan0)
        assert torch.equal(prefix.cpu(), prefix_after) and torch.equal(remaining.cpu(), remaining_after), p
    bits = {torch.bfloat16: torch.int16, torch.float32: torch.int32, torch.float64: torch.int64}[X.dtype]
    assert torch.equal(out.cpu().view(bits), want.view(bits))  # bit for bit: -0.0 is not +0.0, NaN equals NaN


@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_kernel_equals_mirror(cuda, dtype, n):
    """Every pass, every tile edge: rows around the chunk, columns around the column group,
    contiguous and strided, one target and a full sweep."""
    for k, d in enumerate(widths(dtype)):
        for T in ((1, QT.MAX_TARGETS) if n == NS[-1] else ((1, QT.MAX_TARGETS)[k % 2],)):
            W, c = data(n, d, dtype, seed=k)
            assert (W.shape[1] > d) == bool(k % 2)
            check_against_mirror(cuda, W, c, d, spread(n, T))


def test_strided_view_of_a_wider_matrix(cuda):
    W, _ = data(CHUNK + 1, 40, torch.float32)
    X = W[:, 3:3 + 17]
    assert X.stride(0) == 40 and not X.is_contiguous()
    check_against_mirror(cuda, W, 3, 17, spread(CHUNK + 1, QT.MAX_TARGETS))


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_shared_digit_path(cuda, dtype):
    """One constant in every column (every lane of every wave shares its digit in every pass),
    constant columns that differ (a wave's lanes agree per column only), and columns of two
    values laid out in runs (whole waves of one value, waves that straddle a change; one column
    alternates row by row, so its column group never shares): exact counts with the path on
    and off."""
    n, d = 3 * CHUNK + 7, QT.COLUMN_GROUP[dtype] + 1
    same = torch.full((n, d), 1.5, dtype=torch.float64)
    const = same.clone()
    const[:, 1] = -3.0
    run = (torch.arange(n) // 200) % 2
    two = torch.where(run == 0, 1.0, 1.0 + 2.0 ** -6).double()[:, None].repeat(1, d)
    two[:, 2] = torch.where(torch.arange(n) % 2 == 0, -1.0, 2.0).double()
    for X in (same, const, two):
        for flags in (0, QT.SHARED_DIGIT):
            check_against_mirror(cuda, X.to(dtype), 0, d, spread(n, QT.MAX_TARGETS), flags)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_select_and_quantiles_on_device(cuda, dtype):
    n, d = 2 * CHUNK + 77, 33
    W, c = data(n, d, dtype, seed=1)
    X = W.to(cuda)[:, c:c + d]
    ranks = sorted(set(spread(n, 19) + [1, n - 2]))  # three sweeps
    assert torch.equal(ST.order_statistics(X, ranks), torch.sort(X, 0).values[ranks])
    Xf = torch.randn(n, d, generator=torch.Generator().manual_seed(3), dtype=torch.float64).to(dtype).to(cuda)
    got = ST.quantiles(Xf, Q, engine="native")
    assert got.dtype == torch.float64 and got.device.type == "cuda"
    assert torch.equal(got, torch.quantile(Xf.double(), torch.tensor(Q, dtype=torch.float64, device=cuda), dim=0))


def test_nan_column_on_device(cuda):
    n, d = CHUNK + 1, 20
    X = torch.randn(n, d, generator=torch.Generator().manual_seed(4))
    X[7, 4] = float("nan")
    X[CHUNK, 4] = float("nan")
    check_against_mirror(cuda, X, 0, d, spread(n, 3))
    got = ST.quantiles(X.to(cuda), Q, engine="native")
    assert bool(got[:, 4].isnan().all()) and int(got.isnan().sum()) == len(Q)
    ref = torch.quantile(X.to(cuda).double(), torch.tensor(Q, dtype=torch.float64, device=cuda), dim=0)
    assert torch.allclose(got, ref, rtol=0, atol=0, equal_nan=True)


def test_above_the_torch_limit_on_device(cuda):
    n = (1 << 24) + 1
    X = torch.randn(n, 1, generator=torch.Generator().manual_seed(5)).to(cuda)
    with pytest.raises(ValueError, match='engine="native"'):
        ST.quantiles(X, (0.5,))
    got = ST.quantiles(X, (0.5,), engine="native")  # n is odd: the median is an element
    assert torch.equal(got, torch.sort(X, 0).values[n // 2].double()[None])


def test_extra_memory_is_the_histograms(cuda):
    n, d, q = 1 << 22, 8, (0.1, 0.5, 0.9)
    X = torch.randn(n, d, generator=torch.Generator().manual_seed(6)).to(cuda)
    T = 2 * len(q)
    # the module docstring's bound: two histograms (a pass's and the next one's, or the
    # all-reduce buffer), and 64 KiB for the [d, T] prefixes and ranks, the [T, d] output and its
    # fp64 interpolation, each rounded up to the allocator's 512-byte blocks
    bound = 2 * d * T * QT.BINS * 8 + (64 << 10)
    assert bound < X.numel() * X.element_size() // 16
    ST.quantiles(X[:CHUNK], q, engine="native")  # load the kernels outside the measured window
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats(cuda)
    base = torch.cuda.memory_allocated(cuda)
    got = ST.quantiles(X, q, engine="native")
    torch.cuda.synchronize()
    extra = torch.cuda.max_memory_allocated(cuda) - base
    print(f"extra bytes {extra} bound {bound} input {X.numel() * X.element_size()}")
    assert extra <= bound
    ref = torch.quantile(X[:, 0].double(), torch.tensor(q, dtype=torch.float64, device=cuda))
    assert got.shape == (3, d) and torch.equal(got[:, 0], ref)


def test_repeatable(cuda):
    X = data(3 * CHUNK + 7, 65, torch.float32)[0].to(cuda)
    prefix = torch.zeros((65, 1), dtype=torch.int64, device=cuda)
    a, _ = QT.digit_histogram(X, prefix, 0)
    b, _ = QT.digit_histogram(X, prefix, 0)
    assert torch.equal(a, b)
    r1 = ST.quantiles(X, Q, engine="native")
    r2 = ST.quantiles(X, Q, engine="native")
    assert torch.equal(r1.view(torch.int64), r2.view(torch.int64))
