"""CPU self-check of tests/mf_cases.py: the CCD cases satisfy the mutant condition (a dropped
border nonzero or a skipped residual update sits at >= 4 tolerances, so the GPU tests cannot
hide one), the compare helper rejects mutant output, and the ALS exact cases are exact."""
import pytest
import torch

from harp_amd.ops import ccd as C
from tests import mf_cases as MC

CASE_KEYS = MC.all_ccd_case_keys()


def test_class_limits_and_borders():
    lim = MC.class_limits()
    if C.block_max() == 0:
        print("no GPU library: row classes use the documented block limits", MC.DOCUMENTED_BLOCK_MAX)
        assert lim == (C.LONG_ROW,) + MC.DOCUMENTED_BLOCK_MAX
    else:
        assert lim == (C.LONG_ROW, C.block_max(), C.block_max(True))
    assert lim[0] < lim[1] < lim[2] and MC.class_limits(False) == (C.LONG_ROW,) * 3
    assert MC.border_indices(0) == [] and MC.border_indices(1) == [0] and MC.border_indices(2) == [0, 1]
    assert MC.border_indices(65) == [0, 63, 64]
    b = MC.border_indices(4097)
    assert b[-3:] == [4032, 4095, 4096] and 1023 in b and 1024 in b and 64 in b
    # the boundary matrix has a row on both sides of every class limit and a one-element chunk
    lens = set(MC.BOUNDARY_LENS)
    for x in lim:
        assert {x, x + 1} <= lens
    assert any(n > lim[2] and n % C.CHUNK == 1 for n in lens)
    assert sum(n > lim[2] for n in lens) >= 2


@pytest.mark.parametrize("name", list(CASE_KEYS))
def test_ccd_mutant_condition(name):
    case, ref = MC.ccd_reference(*CASE_KEYS[name])
    shifts = MC.ccd_mutant_shifts(case, ref)
    assert set(shifts) == {c for c in ref.tolW if bool(((case.row_cls == MC.CLASSES.index(c)) & (case.lens > 1)).any())}
    print(f"\n{name}: class  fp32_err_W  tol_W  min_shift_a  ratio_a | fp32_err_res  tol_res  min_shift_b  ratio_b")
    for c, s in shifts.items():
        ra, rb = s["a"] / ref.tolW[c], s["b1" if name in MC.B_AT_LARGEST_STEP else "b"] / ref.tolR[c]
        print(f"MFTABLE {name} {c:5s} {ref.errW[c]:.2e} {ref.tolW[c]:.2e} {s['a']:.2e} {ra:.1f} | "
              f"{ref.errR[c]:.2e} {ref.tolR[c]:.2e} {rb * ref.tolR[c]:.2e} {rb:.1f}")
        assert s["self"] < 1e-9, (c, s["self"])  # the Gram formulation reproduces the reference
        assert ra >= MC.MUTANT_FACTOR, (name, c, "a", ra)
        assert rb >= MC.MUTANT_FACTOR, (name, c, "b", rb)
    # the reference itself passes its own comparison, and so does the fp32 yardstick's source
    MC.ccd_compare(case, ref, ref.W64, ref.res64)


def _pick_rows(case):
    """The longest row of every class present."""
    out = []
    for ci, c in enumerate(MC.CLASSES):
        m = (case.row_cls == ci) & (case.lens > 1)
        if bool(m.any()):
            out.append((c, int(torch.argmax(case.lens * m))))
    return out


@pytest.mark.parametrize("kind", ["a", "b"])
@pytest.mark.parametrize("name", ["boundary-k5-lam0.05", "boundary-k1-lam0.0", "lockstep-k3", "reuse-k3", "short-k4"])
def test_compare_rejects_mutants(name, kind):
    """Mutant output fed through the compare helper in place of a GPU result fails, at the
    first, a middle and the last border of the longest row of each class; the plain per-row
    mutant loop also agrees with the Gram evaluation used for the condition."""
    case, ref = MC.ccd_reference(*CASE_KEYS[name])
    shifts = MC.ccd_mutant_shifts(case, ref)
    for c, row in _pick_rows(case):
        n = int(case.lens[row])
        B = MC.border_indices(n)
        for j in {B[0], B[len(B) // 2], B[-1]}:
            for tb in ({0, case.k - 1} if kind == "b" else {0}):
                W, res = MC.ccd_mutant_row(case, ref, row, j, kind, tb)
                a = int(case.ptr[row])
                moved = float((W[row] - ref.W64[row]).abs().max()) if kind == "a" else float(
                    (res[a + j] - ref.res64[a + j]).abs())
                assert moved >= shifts[c][kind] * (1 - 1e-6), (c, row, j, moved, shifts[c][kind])
                with pytest.raises(AssertionError):
                    MC.ccd_compare(case, ref, W, res)


def test_residual_exact_case_is_exact():
    for k in (1, 37):
        rows, cols, val, Fr, Fc, want = MC.residual_exact_case(257, k)
        assert torch.equal(want, want.round()) and float(want.abs().max()) < 2 ** 24
        assert torch.equal(C.residual(rows, cols, val, Fr, Fc).double(), want)  # fp32 CPU path: same bits


@pytest.mark.parametrize("f", [1, 2, 3, 4, 8, 16, 33, 36, 50, 60, 63, 64])
def test_als_exact_cases_are_exact(f):
    case = MC.als_exact_case(f)
    lens = (case.crow[1:] - case.crow[:-1]).tolist()
    assert tuple(lens) == MC.ALS_LENS
    assert int(case.cols.min()) == 0 and int(case.cols.max()) == MC.ALS_N_COLS - 1
    assert bool((case.vals == 0).any()) and set(case.vals.tolist()) <= {0.0, 1.0, 2.0, 3.0}
    assert float(case.F.abs().max()) <= 2 and torch.equal(case.F, case.F.round())
    for r, n in enumerate(lens):  # a duplicate column inside every row of two or more
        if n >= 2:
            a = int(case.crow[r])
            assert case.cols[a:a + n].unique().numel() < n
    for implicit in (False, True):
        for scale_lam in (False, True):
            for use_G in (False, True):
                for lam in (MC.ALS_LAM, 0.0):
                    A, rhs, bound = MC.als_exact_reference(case, implicit, scale_lam, use_G, lam)
                    assert bound < 2 ** 24 and float(A.abs().max()) <= bound and float(rhs.abs().max()) <= bound
                    assert torch.equal(A * 4, (A * 4).round()) and torch.equal(rhs, rhs.round())  # multiples of 1/4
                    assert torch.equal(A.float().double(), A) and torch.equal(rhs.float().double(), rhs)
                    assert torch.equal(A, A.transpose(1, 2))


def test_backward_error_helpers():
    A, b = MC.spd_batch(5, 33, 0)
    for dt in (torch.float32, torch.float64):
        eta = MC.lapack_backward_error(A.to(dt), b.to(dt))
        assert float(eta.max()) < 64 * MC.roundoff(dt)
    x = torch.linalg.solve(A.double(), b.double())
    x[2, 3] *= 1.01  # one wrong component
    eta = MC.backward_error(A, x, b)
    assert float(eta[2]) > 1e3 * MC.roundoff(torch.float32) and float(eta[[0, 1, 3, 4]].max()) < 1e-12
    x[1, 0] = float("nan")
    assert float(MC.backward_error(A, x, b)[1]) == float("inf")
    z = torch.zeros(1, 4)
    assert float(MC.backward_error(torch.eye(4)[None], z, z)[0]) == 0.0
