"""Device-resident SMO (csrc/svm.hip) vs the PyTorch SMO loop (same WSS-2 arithmetic)."""
import time

import pytest
import torch

from harp_amd.models.svm import BinarySVM, MultiClassSVM

pytestmark = pytest.mark.gpu


def _data(n, d, seed, classes=2, spread=1.5):
    g = torch.Generator().manual_seed(seed)
    centers = torch.randn(classes, d, generator=g) * spread
    y = torch.randint(0, classes, (n,), generator=g)
    X = centers[y] + torch.randn(n, d, generator=g)
    return X.double(), y


@pytest.mark.parametrize("n,kernel", [(700, "linear"), (3000, "rbf"), (9000, "rbf"), (20000, "rbf"),
                                      (26000, "rbf")])
def test_device_smo_matches_torch(cuda, n, kernel):
    X, y = _data(n, 16, n)
    Xg, yg = X.to(cuda), y.to(cuda)
    dev = BinarySVM(C=1.0, kernel=kernel, sigma=4.0).fit(Xg, yg)
    ref = BinarySVM(C=1.0, kernel=kernel, sigma=4.0, solver="torch").fit(Xg, yg)
    od, orf = dev.dual_objective(), ref.dual_objective()
    assert abs(od - orf) <= 1e-6 * abs(orf), (od, orf, dev.n_iterations, ref.n_iterations)
    assert abs(dev.bias - ref.bias) < 1e-4
    agree = (dev.predict(Xg) == ref.predict(Xg)).double().mean().item()
    assert agree > 0.999


@pytest.mark.parametrize("n", [5000, 20000, 40000])
def test_coop_smo_matches_one_cu_kernel(cuda, n, monkeypatch):
    """One machine split over 4 / 8 / 16 CUs of one XCD follows the one-CU kernel's exact
    trajectory (same steps, same alphas), and past the one-CU limit (40k rows) the torch
    oracle's objective."""
    from harp_amd.models import svm as S

    X, y = _data(n, 16, n + 1, spread=0.5)
    Xg, yg = X.to(cuda), y.to(cuda)
    K = S.kernel_matrix(Xg, Xg, "rbf", 4.0)
    runs = {}
    for nb in ([0] if n <= 32768 else []) + [4, 8, 16]:
        if nb and n > 4096 * nb:
            continue
        monkeypatch.setenv("HARP_SVM_COOP_NB", str(nb))
        m = BinarySVM(C=1.0, kernel="rbf", sigma=4.0).fit(Xg, yg, K)
        runs[nb] = (m.n_iterations, m.alpha.clone(), m.dual_objective())
    base = runs.get(0, next(iter(runs.values())))
    for nb, (it, al, ob) in runs.items():
        assert it == base[0], (nb, it, base[0])
        assert torch.equal(al, base[1]), nb
    if n > 32768:
        ref = BinarySVM(C=1.0, kernel="rbf", sigma=4.0, solver="torch", max_iterations=200000).fit(Xg, yg, K)
        assert abs(base[2] - ref.dual_objective()) <= 1e-6 * abs(ref.dual_objective())


@pytest.mark.parametrize("n,classes", [(20000, 3), (12000, 5)])
def test_coop_multiclass_matches_one_cu_kernel(cuda, n, classes, monkeypatch):
    """Multiclass machines on the cooperative kernel, one XCD each (3 machines), and two
    after one another on the first XCDs (10 machines), equal the one-CU kernel exactly."""
    X, y = _data(n, 8, 5 + classes, classes=classes, spread=1.0)
    Xg, yg = X.to(cuda), y.to(cuda)
    res = {}
    for nb in (0, 16):
        monkeypatch.setenv("HARP_SVM_COOP_NB", str(nb))
        m = MultiClassSVM(classes, C=1.0, kernel="rbf", sigma=3.0).fit(Xg, yg)
        res[nb] = {k: (v.n_iterations, v.alpha) for k, v in m.machines.items()}
    assert res[0].keys() == res[16].keys() and len(res[0]) == classes * (classes - 1) // 2
    for k in res[0]:
        assert res[0][k][0] == res[16][k][0], k
        assert torch.equal(res[0][k][1], res[16][k][1]), k


def test_device_multiclass_large_machines(cuda):
    """Three machines of ~20000 rows with column lists: by default (at most 16 machines of
    4096 rows or more) they run on the cooperative kernel, 16 CUs and two elements per
    thread each. The one-workgroup 1024 x 24 and 512-thread forms are reached in
    tests/test_svm_edges_gpu.py."""
    X, y = _data(30000, 8, 11, classes=3)
    Xg, yg = X.to(cuda), y.to(cuda)
    dev = MultiClassSVM(3, C=1.0, kernel="rbf", sigma=3.0).fit(Xg, yg)
    ref = MultiClassSVM(3, C=1.0, kernel="rbf", sigma=3.0, solver="torch").fit(Xg, yg)
    for k in dev.machines:
        a, b = dev.machines[k].dual_objective(), ref.machines[k].dual_objective()
        assert abs(a - b) <= 1e-6 * abs(b), (k, a, b)


def test_device_multiclass_one_launch(cuda):
    X, y = _data(2400, 8, 7, classes=5)
    Xg, yg = X.to(cuda), y.to(cuda)
    dev = MultiClassSVM(5, C=1.0, kernel="rbf", sigma=3.0).fit(Xg, yg)
    ref = MultiClassSVM(5, C=1.0, kernel="rbf", sigma=3.0, solver="torch").fit(Xg, yg)
    assert set(dev.machines) == set(ref.machines) and len(dev.machines) == 10
    for k in dev.machines:
        a, b = dev.machines[k].dual_objective(), ref.machines[k].dual_objective()
        assert abs(a - b) <= 1e-6 * abs(b), (k, a, b)
    assert (dev.predict(Xg) == ref.predict(Xg)).double().mean().item() > 0.999


def test_device_smo_20k_converges(cuda):
    """n = 20k RBF, overlapping classes (thousands of SMO steps): the device solver against
    the host-synchronised loop (timed on a step-capped run of the loop, scaled per step; the
    device time includes its setup and the bias / SV extraction). The machine runs on 16 CUs
    (8.2 us per step, 47.9x; the one-CU kernel: 21 us, 19-27x, profiles/r3_svm); the loop's
    per-step host overhead varies by box (300-640 us)."""
    X, y = _data(20000, 16, 3, spread=0.25)
    Xg, yg = X.to(cuda), y.to(cuda)
    from harp_amd.models.svm import kernel_matrix

    K = kernel_matrix(Xg, Xg, "rbf", 4.0)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    dev = BinarySVM(C=1.0, kernel="rbf", sigma=4.0).fit(Xg, yg, K)
    torch.cuda.synchronize()
    t_dev = time.perf_counter() - t0
    steps = dev.n_iterations
    cap = min(steps, 400)
    t0 = time.perf_counter()
    BinarySVM(C=1.0, kernel="rbf", sigma=4.0, solver="torch", max_iterations=cap).fit(Xg, yg, K)
    torch.cuda.synchronize()
    t_ref = (time.perf_counter() - t0) / cap * steps
    print(f"device {t_dev:.4f} s for {steps} steps; torch loop ~{t_ref:.3f} s -> {t_ref / t_dev:.1f}x")
    # correctness only (the speed ratio depends on the box: scripts/bench_speedups.py):
    # the device solution satisfies the WSS-2 stopping rule m(a) - M(a) < eps
    a, G, yv = dev.alpha, dev.grad, yg.double().reshape(-1)
    yv = torch.where(yv > 0, 1.0, -1.0).to(a)
    pos = yv > 0
    mg = -yv * G
    up = (pos & (a < 1.0)) | (~pos & (a > 0))
    low = (pos & (a > 0)) | (~pos & (a < 1.0))
    gap = float(mg[up].max() - mg[low].min())
    assert gap < 1e-3 + 1e-9, gap
    assert steps < 100000
