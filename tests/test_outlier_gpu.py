"""The outlier kernels (csrc/outlier.hip) against their fp64 torch mirror (ops/outlier.py,
``reference_pass``), on the device.

Exact: ``count``, ``changed`` and the mask bytes on every shape, on data that keeps every row
further than relative 1e-9 from the threshold (asserted from the mirror's distances before the
comparison); ``dist2``, ``sum`` and ``gram`` bit for bit on quarter-integer data with an integer
shift and the identity P, where every product and every sum is representable, so no order of
operations can change a bit; the univariate weights on every element.

Toleranced, on real-valued data, with the scales the mirror computes over absolute values:
``|S_gpu - S_ref| <= 4 n 2^-53 sum |terms|`` per statistic (both sides add n terms in some order:
2 (n - 1) u sum|terms| covers both to first order) and ``|dist2_gpu - dist2_ref| <= 8 d 2^-53
(|P| |x - c|)^2`` per row (each z_i is a d-term dot product, (d + 1) u |P_i| |y| on either side,
squared and summed)."""
import math

import pytest
import torch

from harp_amd.models import stats as ST
from harp_amd.ops import outlier as OL

pytestmark = pytest.mark.gpu

DTYPES = (torch.bfloat16, torch.float32, torch.float64)
WIDTHS = (1, 3, 4, 5, 16, 33, 63, 64)
ROWS = (1, 63, 64, 65, OL.CHUNK - 1, OL.CHUNK, OL.CHUNK + 1, OL.GRID * OL.CHUNK + 7)  # the last: second chunks
U = 2.0 ** -53
MARGIN = 1e-9


def real_block(n: int, d: int, dtype, seed: int = 0) -> torch.Tensor:
    g = torch.Generator().manual_seed(seed * 7919 + n * 131 + d)
    return (torch.randn(n, d, generator=g, dtype=torch.float64) * 2 + 0.5).to(dtype)


def model(d: int, seed: int = 0):
    """A centre and the packed whitening matrix of a well-conditioned covariance."""
    g = torch.Generator().manual_seed(1000 + seed * 64 + d)
    A = torch.randn(d, d, generator=g, dtype=torch.float64)
    cov = 4.0 * (A @ A.t() / d + torch.eye(d, dtype=torch.float64))
    c = torch.randn(d, generator=g, dtype=torch.float64) * 0.3 + 0.5
    return c, OL.whiten(cov)


def threshold_in_a_gap(d2: torch.Tensor, frac: float) -> float:
    """A threshold that admits about ``frac`` of the rows and lies further than MARGIN (relative)
    from every distance: the middle of the gap between two neighbouring sorted distances that is
    wide enough and nearest to that rank (low-precision data repeats values, so the neighbours at
    the rank itself may be equal); above all rows if there is no such gap."""
    s = torch.sort(d2).values
    n = s.numel()
    k = min(n, max(0, int(round(frac * n))))
    wide = torch.nonzero(s[1:] - s[:-1] > 8 * MARGIN * s[1:]).flatten() + 1  # cuts between k - 1 and k
    if k == 0:
        t = float(s[0]) * 0.5
    elif k == n or wide.numel() == 0:
        t = float(s[-1]) * 2.0
    else:
        k = int(wide[(wide - k).abs().argmin()])
        t = 0.5 * (float(s[k - 1]) + float(s[k]))
    assert float(((d2 - t).abs() / t).min()) > MARGIN, "a row lies on the threshold: take another seed"
    return t


def run_both(X, c, P, t2, s, mask0, strict, cuda, want_dist=True, flags=0):
    mref = None if mask0 is None else mask0.clone()
    ref = OL.reference_pass(X, c, P, t2, s, mref, want_dist, strict, bounds=True)
    mgpu = None if mask0 is None else mask0.to(cuda)
    got = OL.mahalanobis_pass(X.to(cuda), c.to(cuda), None if P is None else P.to(cuda), t2, s.to(cuda), mask=mgpu,
                              want_dist=want_dist, strict=strict, flags=flags)
    torch.cuda.synchronize()
    return ref, got, mref, mgpu


def assert_counts_equal(ref, got, mref, mgpu):
    assert int(got["count"]) == int(ref["count"])
    assert int(got["changed"]) == int(ref["changed"])
    if mref is not None:
        assert torch.equal(mgpu.cpu(), mref)


def assert_within_bounds(ref, got, n, d, tag=""):
    es = (got["sum"].cpu() - ref["sum"]).abs()
    eg = (got["gram"].cpu() - ref["gram"]).abs()
    bs, bg = 4 * n * U * ref["abs_sum"], 4 * n * U * ref["abs_gram"]
    ed = (got["dist2"].cpu() - ref["dist2"]).abs()
    bd = 8 * d * U * ref["dist2_scale"]
    print(f"{tag} n={n} d={d}: sum err {float(es.max()):.2e} (bound {float(bs.max()):.2e}), gram err "
          f"{float(eg.max()):.2e} (bound {float(bg.max()):.2e}), dist2 err {float(ed.max()):.2e} "
          f"(bound {float(bd.max()):.2e})")
    assert bool((es <= bs).all()) and bool((eg <= bg).all()) and bool((ed <= bd).all())


# ------------------------------------------------------------------ the shape grid
@pytest.mark.parametrize("n", ROWS)
@pytest.mark.parametrize("d", WIDTHS)
def test_pass_shape_grid(cuda, d, n):
    """Every width and row count, the three dtypes: Mahalanobis distances, a mixed mask, the
    compare mode alternating; counts and mask exact, sums and distances within their bounds."""
    c, P = model(d)
    for i, dtype in enumerate(DTYPES):
        X = real_block(n, d, dtype, seed=i)
        d2 = OL.reference_pass(X, c, P, 0.0, c, want_dist=True, want_stats=False)["dist2"]
        t2 = threshold_in_a_gap(d2, 0.6)
        mask0 = (torch.rand(n, generator=torch.Generator().manual_seed(n + d)) < 0.5).to(torch.uint8)
        s = c + 0.125
        ref, got, mref, mgpu = run_both(X, c, P, t2, s, mask0, strict=(i + d) % 2 == 0, cuda=cuda)
        assert_counts_equal(ref, got, mref, mgpu)
        assert_within_bounds(ref, got, n, d, str(dtype))


@pytest.mark.parametrize("flags", (0, OL.VECTOR_STATS), ids=("mfma", "vector"))
@pytest.mark.parametrize("n", (1, 65, OL.CHUNK + 1, OL.GRID * OL.CHUNK + 7))
@pytest.mark.parametrize("d", WIDTHS)
def test_exact_on_quarter_integers(cuda, d, n, flags):
    """Quarter-integer data, an integer shift and centre, the identity P: every product and sum
    is exact, so dist2, sum and gram must equal the mirror bit for bit, in both statistics forms.
    A threshold equal to one row's distance separates the two compare modes."""
    g = torch.Generator().manual_seed(n * 67 + d)
    Xq = torch.randint(-32, 33, (n, d), generator=g).double() / 4
    c = torch.randint(-2, 3, (d,), generator=g).double()
    s = torch.randint(-2, 3, (d,), generator=g).double()
    d2 = ((Xq - c) ** 2).sum(1)
    t2 = float(torch.sort(d2).values[n // 2])
    for dtype in DTYPES:
        X = Xq.to(dtype)
        assert torch.equal(X.double(), Xq)
        for strict in (True, False):
            mask0 = torch.zeros(n, dtype=torch.uint8)
            ref, got, mref, mgpu = run_both(X, c, None, t2, s, mask0, strict, cuda, flags=flags)
            assert torch.equal(ref["dist2"], d2)
            assert_counts_equal(ref, got, mref, mgpu)
            assert torch.equal(got["dist2"].cpu(), ref["dist2"])
            assert torch.equal(got["sum"].cpu(), ref["sum"]) and torch.equal(got["gram"].cpu(), ref["gram"])
            assert torch.equal(got["record"].cpu(), ref["record"])
        below, upto = int((d2 < t2).sum()), int((d2 <= t2).sum())
        assert upto > below  # the row at t2 itself tells `<` from `<=`


@pytest.mark.parametrize("dtype", DTYPES, ids=("bf16", "fp32", "fp64"))
def test_strided_block_masks_and_extreme_thresholds(cuda, dtype):
    """A column slice of a wider matrix (row stride > d) read in place; identity and whitened
    distances; both compare modes; masks that start all 0, all 1 and mixed; thresholds that admit
    no row and every row; no mask at all."""
    n, d = 2 * OL.CHUNK + 37, 5
    W = real_block(n, 11, dtype, seed=3)
    Wg = W.to(cuda)
    X, Xg = W[:, 3:3 + d], Wg[:, 3:3 + d]
    assert Xg.stride(0) == 11 and not Xg.is_contiguous()
    c, Pw = model(d, seed=1)
    mixed = (torch.arange(n) % 3 == 0).to(torch.uint8)
    for P in (None, Pw):
        d2 = OL.reference_pass(X, c, P, 0.0, c, want_dist=True, want_stats=False)["dist2"]
        for t2 in (threshold_in_a_gap(d2, 0.5), 0.0, math.inf):
            for strict in (True, False):
                for mask0 in (torch.zeros(n, dtype=torch.uint8), torch.ones(n, dtype=torch.uint8), mixed, None):
                    mref = None if mask0 is None else mask0.clone()
                    ref = OL.reference_pass(X, c, P, t2, c, mref, True, strict, bounds=True)
                    mgpu = None if mask0 is None else mask0.to(cuda)
                    got = OL.mahalanobis_pass(Xg, c.to(cuda), None if P is None else P.to(cuda), t2, c.to(cuda),
                                              mask=mgpu, want_dist=True, strict=strict)
                    assert_counts_equal(ref, got, mref, mgpu)
                    assert_within_bounds(ref, got, n, d)
                    if t2 == 0.0:
                        assert int(got["count"]) == 0 and not bool(got["record"][2:].any())
                    if t2 == math.inf:
                        assert int(got["count"]) == n
    assert torch.equal(Wg.cpu(), W)  # the block itself is untouched


def test_nonfinite_rows_are_no_members(cuda):
    n, d = 300, 6
    X = real_block(n, d, torch.float32, seed=5)
    X[7, 2], X[100, 0], X[299, 5] = float("nan"), float("inf"), float("-inf")
    c, P = model(d)
    mask = torch.ones(n, dtype=torch.uint8, device=cuda)
    got = OL.mahalanobis_pass(X.to(cuda), c.to(cuda), P.to(cuda), 1e300, c.to(cuda), mask=mask, strict=False)
    assert int(got["count"]) == n - 3 and int(got["changed"]) == 3
    assert mask.cpu()[[7, 100, 299]].sum() == 0 and bool(torch.isfinite(got["record"][2:]).all())
    keep = torch.ones(n, dtype=torch.bool)
    keep[[7, 100, 299]] = False
    ref = OL.reference_pass(X[keep], c, P, 1e300, c, strict=False, bounds=True, want_dist=True)
    assert bool(((got["gram"].cpu() - ref["gram"]).abs() <= 4 * n * U * ref["abs_gram"]).all())


def test_without_stats_the_sums_are_zero(cuda):
    X = real_block(700, 9, torch.float64).to(cuda)
    c, P = model(9)
    a = OL.mahalanobis_pass(X, c.to(cuda), P.to(cuda), 9.0, c.to(cuda), want_stats=False)
    b = OL.mahalanobis_pass(X, c.to(cuda), P.to(cuda), 9.0, c.to(cuda))
    assert int(a["count"]) == int(b["count"]) > 0 and not bool(a["record"][2:].any()) and bool(b["gram"].any())


# ------------------------------------------------------------------ repeatability
@pytest.mark.parametrize("dtype", DTYPES, ids=("bf16", "fp32", "fp64"))
def test_two_runs_give_identical_records(cuda, dtype):
    n, d = 3 * OL.GRID * OL.CHUNK + 11, 33
    X = real_block(n, d, dtype, seed=8).to(cuda)
    c, P = model(d)
    c, P = c.to(cuda), P.to(cuda)
    runs = [OL.mahalanobis_pass(X, c, P, 30.0, c, want_dist=True) for _ in range(2)]
    assert 0 < int(runs[0]["count"]) < n
    assert torch.equal(runs[0]["record"].view(torch.int64), runs[1]["record"].view(torch.int64))
    assert torch.equal(runs[0]["dist2"], runs[1]["dist2"])


# ------------------------------------------------------------------ univariate
@pytest.mark.parametrize("dtype", DTYPES, ids=("bf16", "fp32", "fp64"))
def test_univariate_equals_torch_engine(cuda, dtype):
    n, d = 5 * 4096 // 7 + 3, 7  # several workgroups, the last one partial, rows cut by the spans
    W = real_block(n, 9, dtype, seed=2)
    W[3, 1], W[4, 2], W[5, 3] = float("nan"), float("inf"), float("-inf")
    W[6, 4], W[7, 4] = 0.0, -0.0
    W[:, 5] = 1.5
    Xg = W.to(cuda)[:, 1:1 + d]
    loc = Xg.double().nan_to_num(0, 0, 0).mean(0)
    sc = Xg.double().nan_to_num(0, 0, 0).std(0)
    sc[4] = 0.0
    for thr in (0.0, 1.0, 3.0):
        ref = ST.outliers_univariate(Xg, thr, init="given", location=loc, scatter=sc)
        got = ST.outliers_univariate(Xg, thr, init="given", location=loc, scatter=sc, engine="native")
        assert got.dtype == dtype and got.shape == (n, d) and torch.equal(got, ref)
        cpu = ST.outliers_univariate(Xg.cpu(), thr, init="given", location=loc.cpu(), scatter=sc.cpu())
        assert torch.equal(got.cpu(), cpu)
    Xd = real_block(3000, 64, dtype).to(cuda)
    assert torch.equal(ST.outliers_univariate(Xd, 1.0, init="default", engine="native"),
                       ST.outliers_univariate(Xd, 1.0, init="default"))


# ------------------------------------------------------------------ end to end
def planted(n: int, d: int, dtype, seed: int) -> torch.Tensor:
    g = torch.Generator().manual_seed(seed)
    X = torch.randn(n, d, generator=g, dtype=torch.float64) @ torch.randn(d, d, generator=g, dtype=torch.float64)
    bad = torch.randperm(n, generator=g)[:n // 100]
    X[bad] += 30.0 * torch.sign(torch.randn(len(bad), d, generator=g, dtype=torch.float64))
    return X.to(dtype)


def test_bacon_on_the_device_equals_the_mirror(cuda):
    """20,000 x 8 fp32 with 1 % planted outliers: the same weights and iteration count as the CPU
    mirror, after asserting that the mirror's run keeps every row off every threshold."""
    n, d = 20000, 8
    X = planted(n, d, torch.float32, seed=12)
    trace = []
    ref = ST.bacon_native(X, trace=trace)
    m = min(n, max(4 * d, d + 1))
    for i, (center, P, t2, strict) in enumerate(trace):
        d2 = OL.reference_pass(X, center, P, t2, center, want_dist=True, want_stats=False)["dist2"]
        if i == 0:
            s = torch.sort(d2).values
            assert float(s[m - 1]) == t2 and float(s[m] - s[m - 1]) > MARGIN * float(s[m])
            assert float(s[m - 1] - s[m - 2]) > MARGIN * float(s[m - 1])
        else:
            assert float(((d2 - t2).abs() / t2).min()) > MARGIN
    got = ST.bacon_native(X.to(cuda))
    assert got["iterations"] == ref["iterations"] >= 2
    assert torch.equal(got["weights"].cpu(), ref["weights"])
    assert 0.9 * n < float(ref["weights"].sum()) <= 0.99 * n
    assert torch.equal(ST.outliers_bacon(X.to(cuda), engine="native"), got["weights"])


def test_multivariate_native_equals_torch_on_the_device(cuda):
    for dtype in (torch.float32, torch.float64):
        X = planted(5000, 6, dtype, seed=3).to(cuda)
        for thr in (None, 4.0):
            r = ST.covariance(X)
            d2 = ST.mahalanobis_sq(X, r["mean"].to(cuda), r["covariance"].to(cuda))
            from scipy.stats import chi2

            t = thr if thr is not None else float(chi2.ppf(0.999, 6))
            assert float(((d2 - t).abs() / t).min()) > MARGIN
            got = ST.outliers_multivariate(X, thr, engine="native")
            assert got.dtype == dtype and torch.equal(got, ST.outliers_multivariate(X, thr))


# ------------------------------------------------------------------ memory
def test_bacon_allocates_no_copy_of_the_block(cuda):
    """n = 2^18, d = 16, fp32: the peak above the baseline stays within 16 n bytes (mask, initial
    distances, the returned weights) plus the block partials plus 8 MiB of allocator rounding. An
    fp64 copy of the block alone would take 32 MiB."""
    n, d = 1 << 18, 16
    X = planted(n, d, torch.float32, seed=4).to(cuda)
    ST.bacon_native(X[:4096])  # load the library, warm the allocator's small pools
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats(cuda)
    base = torch.cuda.memory_allocated(cuda)
    out = ST.bacon_native(X)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated(cuda) - base
    partial = OL.GRID * OL.record_len(d) * 8
    print(f"peak above baseline {peak / 2**20:.2f} MiB, limit {(16 * n + partial + (8 << 20)) / 2**20:.2f} MiB")
    assert out["iterations"] >= 1
    assert peak <= 16 * n + partial + (8 << 20) < n * d * 8
