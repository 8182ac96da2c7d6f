"""ALS HIP kernels (csrc/als.hip) at their edges. The build kernels (LDS-DMA, plain fp32,
fp64) must reproduce A and rhs of the integer-valued cases of tests/mf_cases.py bit for bit
(every partial sum is a multiple of 1/4 below 2^24, so no summation order rounds): rows of
0, 1, 31 .. 33, 63 .. 65, 96, 97 and 130 ratings around the 32-row chunk and the DMA buffer
flip. The solvers (fused in-LDS Cholesky, one-wave register Cholesky in both broadcast
variants) are held to 8 times the normwise backward error of LAPACK's Cholesky in the same
precision (floor: 8 units of roundoff), and flag exactly the systems that are not SPD."""
import pytest
import torch

from harp_amd.ops import _lib
from harp_amd.ops import als as OA
from tests import mf_cases as MC

pytestmark = pytest.mark.gpu

F32, F64 = torch.float32, torch.float64
BUILD_PATHS = ([("dma", F32, f) for f in (4, 8, 36, 60, 64)] + [("plain", F32, f) for f in (1, 3, 50, 63)]
               + [("fp64", F64, f) for f in (1, 16, 63, 64)])
CANARY = -777.0
ROW0, SUB_M = 3, 5  # the sub-block: rows of 32, 33, 63, 64 and 65 ratings
COMBOS = [(s, g) for s in (False, True) for g in (False, True)]  # (scale_lam, G given)


def _dev(case, dt, cuda):
    d = lambda x, t=None: (x.to(cuda) if t is None else x.to(cuda, t)).contiguous()
    return d(case.crow), d(case.cols), d(case.vals, dt), d(case.F, dt), d(case.G, dt)


def _build(case, dev, dt, implicit, scale_lam, use_G, row0, m, cuda):
    crow, cols, vals, F, G = dev
    f = case.f
    A = torch.full((m + 1, f, f), CANARY, dtype=dt, device=cuda)
    rhs = torch.full((m + 1, f), CANARY, dtype=dt, device=cuda)
    OA.normal_equations(crow, cols, vals, F, G if use_G else None, implicit, MC.ALS_ALPHA, MC.ALS_LAM, scale_lam,
                        A[:m], rhs[:m], row0)
    torch.cuda.synchronize()
    A, rhs = A.cpu(), rhs.cpu()
    assert bool((A[m] == CANARY).all()) and bool((rhs[m] == CANARY).all()), "wrote past the block"
    return A[:m], rhs[:m]


def _assert_exact(case, dev, dt, implicit, cuda, what):
    n_rows = case.crow.numel() - 1
    for scale_lam, use_G in COMBOS:
        wantA, wantr, _ = MC.als_exact_reference(case, implicit, scale_lam, use_G)
        for row0, m in ((0, n_rows), (ROW0, SUB_M)):
            A, rhs = _build(case, dev, dt, implicit, scale_lam, use_G, row0, m, cuda)
            tag = (what, case.f, implicit, scale_lam, use_G, row0)
            bad = torch.nonzero((A.double() != wantA[row0:row0 + m]).flatten(1).any(1)).reshape(-1).tolist()
            assert not bad, (tag, "A differs in block rows", bad)
            assert torch.equal(rhs.double(), wantr[row0:row0 + m]), (tag, "rhs")
            assert A.dtype == dt and rhs.dtype == dt


@pytest.mark.parametrize("implicit", [False, True])
@pytest.mark.parametrize("path,dt,f", BUILD_PATHS, ids=[f"{p}-f{f}" for p, _, f in BUILD_PATHS])
def test_exact_build(cuda, path, dt, f, implicit):
    """A and rhs equal the fp64 outer-product reference bit for bit: whole matrix and a
    sub-block (row0 > 0, m < n_rows, canary behind it untouched), scale_lam on and off, G
    given and None."""
    case = MC.als_exact_case(f)
    assert (path == "dma") == (dt == F32 and f % 4 == 0)  # harp_als_normal_f32's default choice
    _assert_exact(case, _dev(case, dt, cuda), dt, implicit, cuda, path)


@pytest.mark.parametrize("f", [8, 64])
def test_dma_and_plain_build_agree(cuda, f):
    """With the host switch off the plain kernel builds the f % 4 == 0 systems: the same bits
    as the reference and therefore as the LDS-DMA kernel."""
    _lib.register({"harp_als_set_build_dma": [_lib.c_int]})
    lib = _lib.kernels()
    assert hasattr(lib, "harp_als_set_build_dma")
    case = MC.als_exact_case(f)
    dev = _dev(case, F32, cuda)
    n_rows = case.crow.numel() - 1
    got = {}
    try:
        for dma in (0, 1):
            assert lib.harp_als_set_build_dma(dma) == 0
            for implicit in (False, True):
                _assert_exact(case, dev, F32, implicit, cuda, f"dma={dma}")
                got[dma, implicit] = _build(case, dev, F32, implicit, True, True, 0, n_rows, cuda)
    finally:
        lib.harp_als_set_build_dma(1)
    for implicit in (False, True):
        assert torch.equal(got[0, implicit][0], got[1, implicit][0]) and torch.equal(got[0, implicit][1],
                                                                                     got[1, implicit][1])


def _definite(A):
    """Per system of the exact fp64 batch: +1 numerically SPD, -1 the zero matrix, 0 neither
    (singular: an explicit lam = 0 row with fewer independent ratings than factors; whether a
    Cholesky pivot of it rounds to zero or just above is not defined)."""
    ev = torch.linalg.eigvalsh(A)
    lo, hi = ev[:, 0], ev[:, -1].clamp_min(1e-300)
    out = torch.zeros(A.shape[0], dtype=torch.int64)
    out[lo > 1e-6 * hi] = 1
    out[A.flatten(1).abs().amax(1) == 0] = -1
    return out


def _assert_backward(tag, A, X, b, dt):
    """Batch backward error of X against LAPACK Cholesky in precision dt on the same systems."""
    eta = float(MC.backward_error(A, X, b).max())
    ref = float(MC.lapack_backward_error(A.to(dt), b.to(dt)).max())
    u = MC.roundoff(dt)
    print(f"MFRATIO als {tag} eta/u {eta / u:.2f} lapack/u {ref / u:.2f} ratio_to_bound {eta / max(8 * ref, 8 * u):.3f}")
    assert eta <= max(8 * ref, 8 * u), (tag, eta / u, ref / u)


@pytest.mark.parametrize("lam", [MC.ALS_LAM, 0.0])
@pytest.mark.parametrize("f", [1, 2, 33, 63, 64])
@pytest.mark.parametrize("dt", [F32, F64], ids=["fp32", "fp64"])
def test_fused_solve(cuda, dt, f, lam):
    """Build + in-LDS Cholesky on the exact cases (the systems are known exactly): info flags
    exactly the empty rows of lam = 0, every SPD system meets the backward-error bound."""
    case = MC.als_exact_case(f)
    crow, cols, vals, F, G = _dev(case, dt, cuda)
    n_rows = case.crow.numel() - 1
    empty = torch.tensor(MC.ALS_LENS) == 0
    n_spd = 0
    for implicit in (False, True):
        for scale_lam, use_G in COMBOS:
            A, b, _ = MC.als_exact_reference(case, implicit, scale_lam, use_G, lam)
            kind = _definite(A)
            if lam > 0 or use_G:
                assert bool((kind == 1).all())  # every system SPD, the empty rows' too
            else:
                assert bool((kind[empty] == -1).all())  # (implicit: so is a row whose only rating is 0)
            X = torch.full((n_rows, f), CANARY, dtype=dt, device=cuda)
            info = torch.full((n_rows,), 7, dtype=torch.int32, device=cuda)
            OA.normal_equations(crow, cols, vals, F, G if use_G else None, implicit, MC.ALS_ALPHA, lam, scale_lam,
                                None, None, 0, X=X, info=info)
            torch.cuda.synchronize()
            info, X = info.cpu(), X.cpu()
            tag = f"fused-{'fp32' if dt == F32 else 'fp64'}-f{f}-lam{lam}-imp{int(implicit)}-s{int(scale_lam)}-g{int(use_G)}"
            assert info[kind == -1].tolist() == [1] * int((kind == -1).sum()), (tag, info.tolist())
            assert int(info[kind == 1].sum()) == 0, (tag, info.tolist())
            assert set(info.tolist()) <= {0, 1}
            ok = kind == 1
            n_spd += int(ok.sum())
            if bool(ok.any()):
                _assert_backward(tag, A[ok], X[ok], b[ok], dt)
    assert n_spd >= (8 * n_rows if lam > 0 else 4 * n_rows + 2)  # lam = 0 without G: at least the longest rows


def _bad_systems(A, f):
    """Make systems 3, 10 and 20 of the batch not SPD: non-positive first pivot, non-positive
    last pivot (f - 1), all zero."""
    A = A.clone()
    A[3, 0, 0] = -1.0
    L = torch.linalg.cholesky(A[10].double())
    A[10, f - 1, f - 1] -= float(L[f - 1, f - 1] ** 2) + 1.0  # the last pivot becomes about -1
    A[20] = 0.0
    return A.contiguous(), [3, 10, 20]


@pytest.mark.parametrize("variant", [0, 1])
@pytest.mark.parametrize("m", [1, 4, 5, 37])
@pytest.mark.parametrize("f", [1, 2, 3, 4, 5, 31, 32, 33, 63, 64])
def test_chol_solve(cuda, f, m, variant):
    """One wave per system, LDS-broadcast (0) and v_readlane (1) variants: random SPD fp32
    systems against fp32 LAPACK; with m = 37 three systems are not SPD and exactly those are
    flagged (no padded lane's pivot leaks into info)."""
    A, b = MC.spd_batch(m, f, 100 * f + m)
    bad = []
    if m == 37:
        A, bad = _bad_systems(A, f)
    X = torch.full((m + 1, f), CANARY, device=cuda)
    info = torch.full((m + 1,), 7, dtype=torch.int32, device=cuda)
    OA.chol_solve(A.to(cuda), b.to(cuda), X[:m], info[:m], variant=variant)
    torch.cuda.synchronize()
    X, info = X.cpu(), info.cpu()
    assert bool((X[m] == CANARY).all()) and int(info[m]) == 7
    assert torch.nonzero(info[:m]).reshape(-1).tolist() == bad and int(info[:m].sum()) == len(bad)
    ok = torch.ones(m, dtype=torch.bool)
    ok[bad] = False
    _assert_backward(f"wave-v{variant}-f{f}-m{m}", A[ok], X[:m][ok], b[ok], F32)
