"""EM-GMM HIP kernels (csrc/gmm.hip) vs the PyTorch fp64 E-step / statistics."""
import math
import time

import pytest
import torch

from harp_amd.models import kernels as KF
from harp_amd.ops import gmm as GM

pytestmark = pytest.mark.gpu


def _mixture(n, d, K, seed):
    g = torch.Generator().manual_seed(seed)
    mu = torch.randn(K, d, generator=g, dtype=torch.float64) * 3
    A = torch.randn(K, d, d, generator=g, dtype=torch.float64) * 0.3
    cov = A @ A.transpose(1, 2) + torch.eye(d, dtype=torch.float64)
    w = torch.rand(K, generator=g, dtype=torch.float64) + 0.5
    w = w / w.sum()
    z = torch.randint(0, K, (n,), generator=g)
    L = torch.linalg.cholesky(cov)
    X = mu[z] + (L[z] @ torch.randn(n, d, 1, generator=g, dtype=torch.float64)).squeeze(-1)
    return X, w, mu, cov


def _torch_estep(X, w, mu, cov, covariance):
    logp = KF._log_gauss(X, mu, cov, covariance) + torch.log(w)[None, :]
    lse = torch.logsumexp(logp, 1)
    return torch.exp(logp - lse[:, None]), lse.sum()


@pytest.mark.parametrize("d,K,cov_kind", [(5, 3, "full"), (16, 10, "full"), (32, 64, "full"), (40, 7, "full"), (64, 5, "full"),
                                          (12, 9, "diag")])
def test_estep_and_stats_match_torch(cuda, d, K, cov_kind):
    X, w, mu, cov = _mixture(20000, d, K, d * 100 + K)
    if cov_kind == "diag":
        cov = torch.diagonal(cov, dim1=1, dim2=2).contiguous()
    Xg, wg, mug, covg = (t.to(cuda) for t in (X, w, mu, cov))
    R, ll = GM.estep(Xg, wg, mug, covg, cov_kind)
    Rt, llt = _torch_estep(Xg, wg, mug, covg, cov_kind)
    assert (R - Rt).abs().max().item() < 1e-6
    assert abs(ll.item() - llt.item()) <= 1e-9 * abs(llt.item())
    Nk, S1, S2 = GM.stats(Xg, R, cov_kind)
    assert torch.allclose(Nk, Rt.sum(0), rtol=1e-9, atol=1e-6)
    assert torch.allclose(S1, Rt.t() @ Xg, rtol=1e-9, atol=1e-6)
    S2t = torch.einsum("nk,ni,nj->kij", Rt, Xg, Xg) if cov_kind == "full" else Rt.t() @ (Xg * Xg)
    assert torch.allclose(S2, S2t, rtol=1e-9, atol=1e-5)
    Nk2, _, S22 = GM.stats(Xg, Rt.contiguous(), cov_kind)  # a row-major R is accepted too
    assert torch.allclose(Nk2, Nk, rtol=1e-9, atol=1e-6) and torch.allclose(S22, S2t, rtol=1e-9, atol=1e-5)


def test_em_gmm_native_matches_torch_path(cuda):
    X, w, mu, cov = _mixture(30000, 6, 4, 1)
    init = {"weights": w, "means": mu + 0.5, "covariances": cov}
    a = KF.em_gmm(X.to(cuda), 4, n_iterations=25, accuracy_threshold=0, init=init)
    b = KF.em_gmm(X.to(cuda), 4, n_iterations=25, accuracy_threshold=0, init=init, estep="torch")
    assert torch.allclose(a["means"], b["means"], rtol=1e-8, atol=1e-8)
    assert torch.allclose(a["covariances"], b["covariances"], rtol=1e-8, atol=1e-8)
    assert abs(float(a["loglik"]) - float(b["loglik"])) < 1e-9 * abs(float(b["loglik"]))


def test_em_iteration_1e6(cuda):
    """N = 1e6, d = 32, K = 64: one EM iteration (E-step + statistics) matches the torch
    path; the timing is printed (the >= 10x gate lives in scripts/bench_speedups.py)."""
    X, w, mu, cov = _mixture(1_000_000, 32, 64, 5)
    Xg, wg, mug, covg = (t.to(cuda) for t in (X, w, mu, cov))

    def native():
        R, ll = GM.estep(Xg, wg, mug, covg, "full")
        return GM.stats(Xg, R, "full")

    def ref():
        Rt, _ = _torch_estep(Xg, wg, mug, covg, "full")
        return Rt.sum(0), Rt.t() @ Xg, torch.einsum("nk,ni,nj->kij", Rt, Xg, Xg)

    (nk, sx, sxx), (rk, rx, rxx) = native(), ref()
    for got, want in ((nk, rk), (sx, rx), (sxx, rxx)):
        assert float((got - want).abs().max()) <= 1e-5 * float(want.abs().max()), (got - want).abs().max()
    out = {}
    for name, fn, reps in (("native", native, 5), ("torch", ref, 2)):
        fn()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(reps):
            fn()
        torch.cuda.synchronize()
        out[name] = (time.perf_counter() - t0) / reps
    print(f"EM iteration N=1e6 d=32 K=64: native {out['native'] * 1e3:.2f} ms, torch {out['torch'] * 1e3:.1f} ms, "
          f"{out['torch'] / out['native']:.1f}x")  # ratio asserted in scripts/bench_speedups.py


# ---------------------------------------------------------------------------------------
# Edge shapes: every E-step width on both sides of a switch, the partial 32-point LDS stage,
# the second component tile (K = 65), the second pair tile of both statistics kernels, and
# the input layouts. The references are fp64 torch on the CPU, computed once per
# configuration; the statistics tests take R from the reference E-step, so a failure there
# points at the statistics kernel.
_REF = {}


def _case(n, d, K, cov_kind):
    key = (n, d, K, cov_kind)
    if key not in _REF:
        X, w, mu, cov = _mixture(n, d, K, 7 + n + 1000 * d + 100000 * K)
        if cov_kind == "diag":
            cov = torch.diagonal(cov, dim1=1, dim2=2).contiguous()
        Rt, llt = _torch_estep(X, w, mu, cov, cov_kind)
        _REF[key] = (X, w, mu, cov, Rt, llt)
    return _REF[key]


def _assert_estep(R, ll, Rt, llt):
    assert R.shape == Rt.shape and torch.isfinite(R).all()
    assert (R.cpu() - Rt).abs().max().item() < 1e-6
    assert abs(ll.item() - llt.item()) <= 1e-9 * abs(llt.item())


def _assert_stats(got, X, Rt, cov_kind):
    Nk, S1, S2 = (t.cpu() for t in got)
    assert torch.allclose(Nk, Rt.sum(0), rtol=1e-9, atol=1e-6)
    assert torch.allclose(S1, Rt.t() @ X, rtol=1e-9, atol=1e-6)
    if cov_kind == "full":
        S2t = (Rt.t()[:, None, :] * X.t()[None, :, :]) @ X  # [K, d, n] @ [n, d]
        assert torch.equal(S2, S2.transpose(1, 2))  # the wrapper mirrors the upper triangle
    else:
        S2t = Rt.t() @ (X * X)
    assert S2.shape == S2t.shape
    assert torch.allclose(S2, S2t, rtol=1e-9, atol=1e-5)


@pytest.mark.parametrize("n,K", [(1, 1), (255, 3), (257, 65)])
@pytest.mark.parametrize("d", [1, 8, 9, 17, 33, 63])
def test_estep_widths_and_tails(cuda, d, n, K):
    X, w, mu, cov, Rt, llt = _case(n, d, K, "full")
    R, ll = GM.estep(X.to(cuda), w.to(cuda), mu.to(cuda), cov.to(cuda), "full")
    _assert_estep(R, ll, Rt, llt)


@pytest.mark.parametrize("n", [1, 33, 1000])
@pytest.mark.parametrize("K", [3, 65])
@pytest.mark.parametrize("d,cov_kind", [(15, "full"), (33, "diag"), (64, "diag")])
def test_pair_list_stats_second_pair_tile(cuda, d, cov_kind, K, n):
    assert d < GM.BLOCK_STATS_MIN_D or cov_kind == "diag"  # the pair-list kernel: 136, 67 and 129 pairs
    X, _, _, _, Rt, _ = _case(n, d, K, cov_kind)
    _assert_stats(GM.stats(X.to(cuda), Rt.to(cuda), cov_kind), X, Rt, cov_kind)


@pytest.mark.parametrize("n", [33, 1000])
@pytest.mark.parametrize("K", [3, 65])
@pytest.mark.parametrize("d", [16, 19, 20, 63, 64])
def test_block_stats_coordinate_edges(cuda, d, K, n):
    assert d >= GM.BLOCK_STATS_MIN_D
    X, _, _, _, Rt, _ = _case(n, d, K, "full")
    _assert_stats(GM.stats(X.to(cuda), Rt.to(cuda), "full"), X, Rt, "full")


def test_estep_outliers_keep_the_running_maximum(cuda):
    """50 of 300 points lie at least 60 standard deviations from every mean: every log p of
    theirs is below -1000, and a softmax without the running maximum is 0 / 0."""
    n, d, K, far = 300, 8, 5, 50
    X, w, mu, cov = _mixture(n, d, K, 41)
    g = torch.Generator().manual_seed(42)
    u = torch.randn(far, d, generator=g, dtype=torch.float64)
    X[:far] = 120.0 * u / u.norm(dim=1, keepdim=True)
    logp = KF._log_gauss(X, mu, cov, "full")
    maha = -2 * logp[:far] - torch.linalg.slogdet(cov)[1][None, :] - d * math.log(2 * math.pi)
    assert maha.min().item() >= 60.0 ** 2 and logp[:far].max().item() < -1000
    Rt, llt = _torch_estep(X, w, mu, cov, "full")
    R, ll = GM.estep(X.to(cuda), w.to(cuda), mu.to(cuda), cov.to(cuda), "full")
    assert torch.isfinite(R).all() and math.isfinite(ll.item())
    assert (R.sum(1) - 1).abs().max().item() <= 1e-12
    _assert_estep(R, ll, Rt, llt)


def _all_results(Xg, w, mu, cov, Rg, cov_kind, K):
    R, ll = GM.estep(Xg, w, mu, cov, cov_kind)
    out = [R, ll, *GM.stats(Xg, Rg, cov_kind)]
    em = KF.em_gmm(Xg, K, n_iterations=3, accuracy_threshold=0, covariance=cov_kind,
                   init={"weights": w, "means": mu, "covariances": cov})
    return out + [em["weights"], em["means"], em["covariances"], em["loglik"]]


@pytest.mark.parametrize("layout", ["wide_slice", "column_stride", "transposed"])
@pytest.mark.parametrize("d,cov_kind", [(5, "full"), (20, "full"), (12, "diag")])
def test_input_layouts_equal_the_contiguous_copy(cuda, d, cov_kind, layout):
    """n = 100 is one point block in every kernel, so nothing depends on the order of the
    fp64 atomics and a view must give its contiguous copy's results bit for bit:
    ``Xw[:, 3:3 + d]`` (unit inner stride, ldx > d) as it is, ``Xw[:, ::2]`` and ``Y.t()``
    (inner stride != 1) through a copy."""
    n, K = 100, 3
    X, w, mu, cov, Rt, _ = _case(n, d, K, cov_kind)
    g = torch.Generator().manual_seed(d)
    if layout == "wide_slice":
        Xw = torch.randn(n, d + 7, generator=g, dtype=torch.float64)
        Xw[:, 3:3 + d] = X
        view = Xw.to(cuda)[:, 3:3 + d]
        assert view.stride() == (d + 7, 1)
    elif layout == "column_stride":
        Xw = torch.randn(n, 2 * d, generator=g, dtype=torch.float64)
        Xw[:, ::2] = X
        view = Xw.to(cuda)[:, ::2]
        assert view.stride() == (2 * d, 2)
    else:
        view = X.t().contiguous().to(cuda).t()
        assert view.stride() == (1, n)
    assert GM.usable(view) and not view.is_contiguous() and torch.equal(view.cpu(), X)
    wg, mug, covg, Rg = (t.to(cuda) for t in (w, mu, cov, Rt))
    got = _all_results(view, wg, mug, covg, Rg, cov_kind, K)
    want = _all_results(view.contiguous(), wg, mug, covg, Rg, cov_kind, K)
    for name, a, b in zip(("R", "ll", "Nk", "S1", "S2", "weights", "means", "covariances", "loglik"), got, want):
        assert torch.equal(a, b), name
    _assert_estep(got[0], got[1], Rt, _case(n, d, K, cov_kind)[5])
    _assert_stats(got[2:5], X, Rt, cov_kind)


def test_single_transposed_row(cuda):
    """``Y.t()`` of a [d, 1] tensor is one row whose row stride is 1 < d: valid input."""
    X, w, mu, cov, Rt, llt = _case(1, 9, 1, "full")
    view = X.reshape(9, 1).to(cuda).t()
    assert view.shape == (1, 9) and view.stride(0) < 9
    R, ll = GM.estep(view, w.to(cuda), mu.to(cuda), cov.to(cuda), "full")
    _assert_estep(R, ll, Rt, llt)
    _assert_stats(GM.stats(view, Rt.to(cuda), "full"), X, Rt, "full")
