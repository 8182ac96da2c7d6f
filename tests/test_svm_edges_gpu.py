"""Step-exact SMO: every reachable form of the device kernels (csrc/svm.hip) against the
PyTorch loop of harp_amd/models/svm.py on the same GPU Gram matrix.

The kernel header promises that products and sums are rounded one by one so that the
trajectory follows the oracle's; the assertion is therefore exact: equal ``n_iterations``,
``torch.equal`` alphas and ``torch.equal`` gradients (the gradient covers every element, so
every register slot's update is checked, not only the rows that were picked). Most runs
stop at a step cap, which sizes the run and excludes nothing.

Kernel forms (one-workgroup kernel: elements per thread x threads; "diag" = the kernel
diagonal staged in LDS, which needs 8 n bytes, or 12 n with a column list, within 159 KB):
  1 x 1024 .. 24 x 1024 for n <= 1024, 2048, 4096, 8192, 16384, 24576; 64 x 512 above;
  diag up to n = 20352 (identity) / 13568 (column list);
  cooperative kernel: ceil(n / (1024 NB)) <= 4 elements per thread over NB workgroups.
"""
import warnings

import pytest
import torch

from harp_amd.models import svm as S
from harp_amd.models.svm import BinarySVM, MultiClassSVM, coop_workgroups, smo_device

pytestmark = pytest.mark.gpu

EPS, TAU = 1e-3, 1e-6
FELL_BACK = "cooperative SMO did not run"


# ------------------------------------------------------------------------------- inputs
def _labels(n):
    y = torch.ones(n, dtype=torch.float64)
    y[1::2] = -1.0
    return y


def grid(n):
    """Integer points of a 5 x 5 grid, labels alternating: duplicate rows with opposite
    labels give K_ii + K_jj - 2 K_ij == 0 exactly (the tau branch), and the integer scores
    tie."""
    g = torch.Generator().manual_seed(1000 + n)
    return torch.randint(-2, 3, (n, 2), generator=g).double(), _labels(n)


def hard_tail(n, hard=600):
    """Two separated blobs whose last ``hard`` rows sit near the margin: the support is the
    first row and rows of the tail, i.e. the top register slots and the top mask bits."""
    g = torch.Generator().manual_seed(2000 + n)
    y = _labels(n)
    X = 0.5 * torch.randn(n, 2, generator=g, dtype=torch.float64)
    X[:, 0] += 4 * y
    X[-hard:, 0] -= 3.7 * y[-hard:]
    return X, y


def oracle_trace(K, yv, C, eps, tau, cap):
    """A copy of the loop of ``BinarySVM.fit`` with bookkeeping: steps that took the tau
    branch, steps whose delta was clipped to the box, steps with tied i or j candidates."""
    n = yv.numel()
    Kd = torch.diagonal(K).clone()
    a = torch.zeros(n, dtype=torch.float64, device=K.device)
    G = -torch.ones(n, dtype=torch.float64, device=K.device)
    pos = yv > 0
    steps = n_tau = n_clip = n_tie = 0
    for _ in range(cap):
        mg = -yv * G
        up = (pos & (a < C)) | (~pos & (a > 0))
        low = (pos & (a > 0)) | (~pos & (a < C))
        mu = torch.where(up, mg, torch.full_like(mg, -float("inf")))
        i = int(mu.argmax())
        m = float(mu[i])
        Mv = float(torch.where(low, mg, torch.full_like(mg, float("inf"))).min())
        if m - Mv < eps:
            break
        bt = m - mg
        raw = Kd[i] + Kd - 2 * K[i]
        at = torch.where(raw > 0, raw, torch.full_like(raw, tau))
        score = torch.where(low & (mg < m), -(bt * bt) / at, torch.full_like(bt, float("inf")))
        j = int(score.argmin())
        n_tie += int(int((mu == m).sum()) > 1 or int((score == score[j]).sum()) > 1)
        n_tau += int(not float(raw[j]) > 0)
        yi, yj = float(yv[i]), float(yv[j])
        free = float(bt[j]) / float(at[j])
        ai, aj = float(a[i]), float(a[j])
        delta = max(0.0, min(free, C - ai if yi > 0 else ai, aj if yj > 0 else C - aj))
        n_clip += int(delta != free)
        dai, daj = yi * delta, -yj * delta
        a[i] += dai
        a[j] += daj
        G += yv * (yi * dai * K[i] + yj * daj * K[j])
        steps += 1
    return a, G, steps, dict(tau=n_tau, clipped=n_clip, tied=n_tie)


# --------------------------------------------------------------------------- comparison
def _kw(C, cap, tau=TAU):
    return dict(C=C, kernel="linear", accuracy_threshold=EPS, tau=tau, max_iterations=cap)


def _oracle(X, y, K, C, cap, tau=TAU):
    m = BinarySVM(solver="torch", **_kw(C, cap, tau)).fit(X, y, K)
    return m.alpha, m.grad, m.n_iterations


def _device_runs(monkeypatch):
    """Records what ``smo_device`` returned, so no case passes on the PyTorch loop unnoticed."""
    seen = []
    real = S.smo_device

    def spy(*a, **k):
        r = real(*a, **k)
        seen.append(r is not None)
        return r

    monkeypatch.setattr(S, "smo_device", spy)
    return seen


def _run(fn, nb, monkeypatch):
    """``fn()`` with HARP_SVM_COOP_NB = nb (None: unset). A cooperative launch that fell back
    to the one-workgroup kernel is a skip with the warning's text, never a silent pass."""
    if nb is None:
        monkeypatch.delenv("HARP_SVM_COOP_NB", raising=False)
    else:
        monkeypatch.setenv("HARP_SVM_COOP_NB", str(nb))
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        out = fn()
    for w in rec:
        if FELL_BACK in str(w.message):
            pytest.skip(str(w.message))
    return out, [str(w.message) for w in rec]


def _fit_device(X, y, K, C, cap, nb, monkeypatch, tau=TAU):
    seen = _device_runs(monkeypatch)
    m, _ = _run(lambda: BinarySVM(**_kw(C, cap, tau)).fit(X, y, K), nb, monkeypatch)
    assert seen == [True], seen
    return m.alpha, m.grad, m.n_iterations


def _same(dev, ref, what):
    (a, g, it), (ra, rg, rit) = dev, ref
    assert it == rit, (what, it, rit)
    for name, u, v in (("alpha", a, ra), ("grad", g, rg)):
        if not torch.equal(u, v):
            bad = torch.nonzero(u != v).reshape(-1)
            raise AssertionError(f"{what}: {name} differs at {bad.numel()} of {u.numel()} elements (first "
                                 f"{bad[:4].tolist()}), largest difference {float((u - v).abs().max()):.3e}")


# ---------------------------------------------- 1: wave, block and first-tier edges (identity)
_GRID = {}


def _grid_ref(dev, n, C, tau):
    if (n, C, tau) not in _GRID:
        X, y = grid(n)
        X, y = X.to(dev), y.to(dev)
        K = X @ X.T
        ref = _oracle(X, y, K, C, 400, tau)
        if n >= 64:
            a, G, steps, seen = oracle_trace(K, y, C, EPS, tau, 400)
            # the bookkeeping copy is the oracle, and the run has what the case is about
            assert torch.equal(a, ref[0]) and torch.equal(G, ref[1]) and steps + 1 == ref[2]
            assert seen["tau"] >= 1 and seen["clipped"] >= 1 and seen["tied"] >= 1, (n, C, tau, seen)
        _GRID[n, C, tau] = (X, y, K, ref)
    return _GRID[n, C, tau]


@pytest.mark.parametrize("nb", [0, 1, 16])
@pytest.mark.parametrize("tau", [TAU, 1.0])
@pytest.mark.parametrize("C", [0.01, 1.0])
@pytest.mark.parametrize("n", [1, 2, 3, 63, 64, 65, 1023, 1024, 1025])
def test_grid_edges_match_oracle(cuda, monkeypatch, n, C, tau, nb):
    """1 and 2 elements per thread of the one-workgroup kernel (nb = 0) and of the
    cooperative kernel on one workgroup and on 16, most of which own nothing: idle owners,
    the clamped gather (n - 1), reductions over empty lanes, ties, tau steps, clipped steps.
    With tau = 1e-6 a pair of zero curvature wins the selection and its step ends clipped
    whatever tau is (a kernel that divided by zero instead passes); with tau = 1 such a pair
    competes with pairs of true curvature 1 and its step need not be clipped, so the value
    matters."""
    X, y, K, ref = _grid_ref(cuda, n, C, tau)
    assert coop_workgroups(n) == 0  # (the default choice at these sizes)
    _same(_fit_device(X, y, K, C, 400, nb, monkeypatch, tau), ref, (n, C, tau, nb))


# -------------------------------------------- 2: every one-workgroup tier and its neighbour
def _tail_support(alpha, n):
    sup = torch.nonzero(alpha != 0).reshape(-1)
    assert bool((sup == 0).any()) and bool((sup >= n - 512).any()), sup.tolist()


@pytest.mark.parametrize("n,C", [(n, 1.0) for n in (2048, 2049, 4096, 4097, 8192, 8193, 16384, 16385, 20352, 20353,
                                                    24576, 24577, 32768)] + [(24577, 0.05), (32768, 0.05)])
def test_one_workgroup_tiers_match_oracle(cuda, monkeypatch, n, C):
    """Identity path, cooperative kernel off: 2, 4, 8, 16 and 24 elements per thread at 1024
    threads, each at its last size and one past it; 20352 / 20353: the last size whose
    diagonal fits in LDS and the first that gathers it; 24577 and 32768: 64 elements per
    thread at 512 threads with 64-bit box masks, 32768 filling every slot. The support
    holds row 0 and rows of the last 512, so the top slots and mask bits are selected."""
    X, y = hard_tail(n)
    X, y = X.to(cuda), y.to(cuda)
    K = X @ X.T
    ref = _oracle(X, y, K, C, 60)
    _tail_support(ref[0], n)
    _same(_fit_device(X, y, K, C, 60, 0, monkeypatch), ref, (n, C))
    del K
    torch.cuda.empty_cache()


# ------------------------------------------------------------- 3: the column-list path
_COLS = {}


def _cols_case(dev, n):
    """One machine of ``hard_tail(n)`` rows scattered, unsorted, over a Gram matrix of
    n + 37 rows; the oracle solves the gathered n x n block."""
    N = n + 37
    g = torch.Generator().manual_seed(3000 + n)
    idx = torch.randperm(N, generator=g)[:n]
    Xm, y = hard_tail(n)
    Xf = torch.randn(N, 2, generator=g, dtype=torch.float64)
    Xf[idx] = Xm
    Xf, idx, y = Xf.to(dev), idx.to(dev), y.to(dev)
    K = Xf @ Xf.T
    if n not in _COLS:
        _COLS[n] = _oracle(Xf[idx], y, K[idx][:, idx], 1.0, 60)
        _tail_support(_COLS[n][0], n)
    return K, idx, y, _COLS[n]


@pytest.mark.parametrize("nb", [0, 16])
@pytest.mark.parametrize("n", [5, 1025, 13568, 13569, 24577])
def test_column_list_matches_oracle(cuda, monkeypatch, n, nb):
    """``smo_device`` on unsorted ids, with K contiguous and with K a column slice of a wider
    buffer (ldk != N): column list in LDS with the diagonal (up to 13568 rows) and without,
    24577 on the 512-thread form; nb = 16: the cooperative kernel's indirection."""
    K, idx, y, ref = _cols_case(cuda, n)
    N = K.shape[0]
    buf = torch.full((N, N + 24), float("nan"), dtype=torch.float64, device=cuda)
    buf[:, 11:11 + N] = K
    for name, Kx in (("contiguous", K), ("padded", buf[:, 11:11 + N])):
        assert Kx.stride(1) == 1 and (Kx.stride(0) == N) == (name == "contiguous")
        res, _ = _run(lambda: smo_device(Kx, [(idx, y)], 1.0, EPS, TAU, 60), nb, monkeypatch)
        assert res is not None and len(res) == 1
        a, g, steps = res[0]
        _same((a, g, steps + 1), ref, (n, nb, name))
    del K, buf
    torch.cuda.empty_cache()


# ---------------------------------------------------------------- 4, 5: many machines
def _multiclass(dev, counts, seed):
    g = torch.Generator().manual_seed(seed)
    y = torch.cat([torch.full((c,), k, dtype=torch.long) for k, c in enumerate(counts)])
    y = y[torch.randperm(y.numel(), generator=g)]
    centers = 1.5 * torch.randn(len(counts), 3, generator=g, dtype=torch.float64)
    X = centers[y] + torch.randn(y.numel(), 3, generator=g, dtype=torch.float64)
    return X.to(dev), y.to(dev)


def _fit_multiclass(X, y, classes, cap, nb, monkeypatch, **kernel):
    kw = dict(C=1.0, accuracy_threshold=EPS, tau=TAU, max_iterations=cap, **kernel)
    ref = MultiClassSVM(classes, solver="torch", **kw).fit(X, y)
    seen = _device_runs(monkeypatch)
    dev, _ = _run(lambda: MultiClassSVM(classes, **kw).fit(X, y), nb, monkeypatch)
    assert seen == [True], seen
    assert list(dev.machines) == list(ref.machines)
    for key, m in dev.machines.items():
        r = ref.machines[key]
        _same((m.alpha, m.grad, m.n_iterations), (r.alpha, r.grad, r.n_iterations), (key, nb))
    assert torch.equal(dev.predict(X), ref.predict(X))
    return dev


@pytest.mark.parametrize("nb", [0, 4, 16])
def test_unequal_machines_match_oracle(cuda, monkeypatch, nb):
    """Class counts [3000, 40, 1, 0]: machines of 3040, 3001, 3000, 41, 40 and 1 rows in one
    launch (4 elements per thread at nb = 0; one each on the cooperative kernel, whose
    participants mostly own nothing in the small machines). The machines of 3000, 40 and
    1 rows have one class only: no step, alpha 0, gradient -1."""
    X, y = _multiclass(cuda, [3000, 40, 1, 0], 41)
    dev = _fit_multiclass(X, y, 4, 100, nb, monkeypatch, kernel="rbf", sigma=2.0)
    assert {k: m.alpha.numel() for k, m in dev.machines.items()} == {(0, 1): 3040, (0, 2): 3001, (0, 3): 3000,
                                                                     (1, 2): 41, (1, 3): 40, (2, 3): 1}
    for key in ((0, 3), (1, 3), (2, 3)):
        m = dev.machines[key]
        assert m.n_iterations == 1 and bool((m.alpha == 0).all()) and bool((m.grad == -1).all()), key
    assert all(dev.machines[key].n_iterations > 1 for key in ((0, 1), (0, 2), (1, 2)))


def test_more_than_16_machines_match_oracle(cuda, monkeypatch):
    """21 machines, the largest of 4200 rows: past 16 machines the one-workgroup kernel is the
    default choice although the rows would qualify for the cooperative one (8 elements per
    thread, column lists and diagonals in LDS)."""
    X, y = _multiclass(cuda, [2100, 2100, 50, 50, 50, 50, 50], 43)
    monkeypatch.delenv("HARP_SVM_COOP_NB", raising=False)
    assert coop_workgroups(4200, 21) == 0 and coop_workgroups(4200, 16) == 16
    dev = _fit_multiclass(X, y, 7, 60, None, monkeypatch, kernel="linear")
    assert len(dev.machines) == 21 and max(m.alpha.numel() for m in dev.machines.values()) == 4200


# ----------------------------------------------------------------- 6: cooperative tiers
@pytest.mark.parametrize("n,nb", [(n, 1) for n in (1024, 1025, 2048, 2049, 3072, 3073, 4096)] + [(12289, 4)])
def test_coop_tiers_match_oracle(cuda, monkeypatch, n, nb):
    """1, 2, 3 and 4 elements per thread of the cooperative kernel on one workgroup, each
    at its last size and one past it, and 4 elements per thread across 4 workgroups."""
    X, y = hard_tail(n)
    X, y = X.to(cuda), y.to(cuda)
    K = X @ X.T
    ref = _oracle(X, y, K, 1.0, 60)
    _tail_support(ref[0], n)
    monkeypatch.setenv("HARP_SVM_COOP_NB", str(nb))
    assert coop_workgroups(n) == nb
    _same(_fit_device(X, y, K, 1.0, 60, nb, monkeypatch), ref, (n, nb))


# ------------------------------------------------------------------ 7: degenerate runs
@pytest.mark.parametrize("nb", [0, 16])
def test_one_class_only(cuda, monkeypatch, nb):
    X, _ = hard_tail(50)
    X, y = X.to(cuda), torch.ones(50, dtype=torch.float64, device=cuda)
    K = X @ X.T
    a, g, it = _fit_device(X, y, K, 1.0, 400, nb, monkeypatch)
    _same((a, g, it), _oracle(X, y, K, 1.0, 400), nb)
    assert it == 1 and bool((a == 0).all()) and bool((g == -1).all())


@pytest.mark.parametrize("nb", [0, 16])
def test_no_steps_allowed(cuda, monkeypatch, nb):
    X, y = hard_tail(50)
    X, y = X.to(cuda), y.to(cuda)
    K = X @ X.T
    a, g, it = _fit_device(X, y, K, 1.0, 0, nb, monkeypatch)
    _same((a, g, it), _oracle(X, y, K, 1.0, 0), nb)
    assert it == 1 and bool((a == 0).all()) and bool((g == -1).all())


def test_past_one_workgroup_limit_falls_back_to_loop(cuda, monkeypatch):
    """32769 rows with the cooperative kernel off: no device kernel takes the machine, ``fit``
    warns and runs the PyTorch loop."""
    n = 32769
    X, y = hard_tail(n)
    X, y = X.to(cuda), y.to(cuda)
    K = X @ X.T
    seen = _device_runs(monkeypatch)
    m, msgs = _run(lambda: BinarySVM(**_kw(1.0, 5)).fit(X, y, K), 0, monkeypatch)
    assert seen == [False] and any("falling back to the PyTorch SMO loop" in s for s in msgs), (seen, msgs)
    _same((m.alpha, m.grad, m.n_iterations), _oracle(X, y, K, 1.0, 5), n)
    assert m.n_iterations == 6
    del K
    torch.cuda.empty_cache()
