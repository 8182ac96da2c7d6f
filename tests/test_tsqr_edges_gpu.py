"""Householder TSQR (csrc/tsqr.hip through ``house_tsqr``) at every register width, block
edge, tree shape and rank defect, against LAPACK's fp64 QR of the same matrix.

Reference: ``torch.linalg.qr`` in fp64 on the CPU, R's diagonal made non-negative.
Tolerances are relative to the reference's own errors, with u = 2^-53:
  * orthogonality |Q^T Q - I|_max <= max(8 |Q_ref^T Q_ref - I|_max, 16 d u),
  * residual |Q R - A|_max <= max(8 |Q_ref R_ref - A|_max, 16 d u |A|_max),
  * |R - R_ref|_max <= 64 d u cond_2(A) |A|_2 (full-rank cases with n >= d).
The factor 8 covers the different reduction order (a tree of 256-row blocks against a
blocked panel). Every case prints its three errors as fractions of these tolerances.

Worst fractions measured on the MI355X over all cases of this module: orthogonality 0.81
at (1281, 1) (a single column: the tolerance is its floor of 16 u, the error 6.5 u; the next
is 0.38 at (8193, 8)), residual 0.13 at (257, 1), R 0.017 at (255, 1); for d >= 7 every
fraction is below 0.15, for d >= 16 below 0.07. No case needed more than the factor 8.

Tree shapes (256 rows per block, W = register width, every level stacks W x W factors):
  d <= 8, n = 8192: 32 blocks -> 256 rows, one full block; n = 8193: 33 blocks -> 264 rows,
  the second block of level 2 holds a single 8 x 8 R;
  W = 64: n = 1025: 5 blocks -> 320 rows = a block of four R's and a block of one;
  n = 1281: 6 blocks -> 384 rows -> 2 blocks -> 128 rows (three levels).
"""
import pytest
import torch

from harp_amd.ops import _lib
from harp_amd.ops import linalg as LA

pytestmark = pytest.mark.gpu

U = 2.0**-53
_WORST = {"orth": 0.0, "resid": 0.0, "R": 0.0}


def _randn(n, d, seed=None):
    g = torch.Generator().manual_seed(n * 1009 + d if seed is None else seed)
    return torch.randn(n, d, generator=g, dtype=torch.float64)


def _eye_err(Q):
    return float((Q.t() @ Q - torch.eye(Q.shape[1], dtype=torch.float64)).abs().max()) if Q.numel() else 0.0


def _check(A, cuda, compare_r=True, what=""):
    """Factor A (a CPU fp64 matrix) natively and compare with LAPACK; returns (Q, R) on the CPU."""
    n, d = A.shape
    k = min(n, d)
    Q, R = LA.house_tsqr(A.to(cuda))
    Q, R = Q.cpu(), R.cpu()
    assert Q.shape == (n, d) and R.shape == (d, d)
    assert torch.equal(R, torch.triu(R)) and bool((torch.diagonal(R) >= 0).all())
    Qr, Rr = torch.linalg.qr(A)
    amax = float(A.abs().max())
    tol_o = max(8 * _eye_err(Qr), 16 * d * U)
    tol_r = max(8 * float((Qr @ Rr - A).abs().max()), 16 * d * U * amax)
    orth = _eye_err(Q[:, :k])
    resid = float((Q @ R - A).abs().max())
    frac = {"orth": orth / tol_o, "resid": resid / tol_r if tol_r > 0 else float(resid > 0)}
    if compare_r and n >= d:
        Rr = Rr * torch.sign(torch.diagonal(Rr))[:, None]
        tol_R = 64 * d * U * float(torch.linalg.cond(A)) * float(torch.linalg.matrix_norm(A, 2))
        frac["R"] = float((R - Rr).abs().max()) / tol_R
    for key, v in frac.items():
        _WORST[key] = max(_WORST[key], v)
    print(f"tsqr {what or tuple(A.shape)}: fractions of tolerance " +
          ", ".join(f"{key} {v:.3f}" for key, v in frac.items()) +
          " | worst so far " + ", ".join(f"{key} {v:.3f}" for key, v in _WORST.items()))
    assert all(v <= 1.0 for v in frac.values()), frac
    return Q, R


# ------------------------------------------------------------- every width, at its edges
WIDTH = {1: 8, 7: 8, 8: 8, 9: 16, 16: 16, 17: 32, 24: 32, 32: 32, 33: 64, 48: 64, 64: 64}


@pytest.mark.parametrize("n", [255, 256, 257, 1281])
@pytest.mark.parametrize("d", sorted(WIDTH))
def test_every_width_at_block_edges(cuda, d, n):
    """d at and around each register width (8, 16, 32, 64), n one short of a block, a full
    block, one row into the second block, and 1281 rows (6 blocks; three levels at W = 64)."""
    assert _lib.kernels().harp_tsqr_width(d) == WIDTH[d]
    _check(_randn(n, d), cuda)


@pytest.mark.parametrize("n,d", [(8192, 8), (8193, 8), (1025, 64)])
def test_second_level_block_of_one_r(cuda, n, d):
    """Level-2 blocks that are exactly full, and ones that hold a single R (see the module
    docstring for the row counts)."""
    W, TB = _lib.kernels().harp_tsqr_width(d), _lib.kernels().harp_tsqr_rows_per_block()
    rows2 = -(-n // TB) * W
    assert rows2 % TB == {8192: 0, 8193: 8, 1025: 64}[n] and TB == 256
    _check(_randn(n, d), cuda)


# ---------------------------------------------------------------------- n < d and n == d
@pytest.mark.parametrize("n,d", [(1, 8), (5, 16), (31, 32), (32, 32), (63, 64), (20, 33)])
def test_short_and_square(cuda, n, d):
    """Q R == A, Q[:, :n] orthonormal and R upper triangular when there are no more rows
    than columns (steps j >= n find an all-zero column tail: identity reflectors)."""
    _check(_randn(n, d), cuda)


# ------------------------------------------------------------------------ rank deficiency
def _zero_column():
    A = _randn(300, 24)
    A[:, 11] = 0
    return A


def _twin_columns():
    A = _randn(300, 32)
    A[:, 20] = A[:, 3]
    return A


def _zero_first_block():
    A = _randn(513, 9)
    A[:256] = 0
    return A


def _one_row(r):
    A = torch.zeros(300, 17, dtype=torch.float64)
    A[r] = _randn(1, 17, seed=r)[0]
    return A


@pytest.mark.parametrize("name,make", [
    ("zero-column-11-of-24", _zero_column),
    ("twin-columns-3-20-of-32", _twin_columns),
    ("zero-first-block-513x9", _zero_first_block),
    ("only-row-0-of-300x17", lambda: _one_row(0)),
    ("only-row-7-of-300x17", lambda: _one_row(7)),
    ("only-row-299-of-300x17", lambda: _one_row(299)),
])
def test_rank_deficient(cuda, name, make):
    """Q R == A and an orthonormal Q although R is singular; an exact 0 on R's diagonal takes
    the sgn == 0 -> 1 path. (R itself is not unique here, so it is not compared.)"""
    _check(make(), cuda, compare_r=False, what=name)


def test_all_zero_matrix(cuda):
    """Every reflector is the identity: R is exactly 0 and Q's columns are orthonormal."""
    A = torch.zeros(257, 16, dtype=torch.float64)
    Q, R = _check(A, cuda, compare_r=False, what="all-zero 257x16")
    assert torch.equal(R, torch.zeros(16, 16, dtype=torch.float64))
    assert torch.equal(Q.t() @ Q, torch.eye(16, dtype=torch.float64))


# ------------------------------------------------------------------------------ want_q
@pytest.mark.parametrize("n,d", [(513, 24), (1281, 64), (20, 33)])
def test_r_alone_is_the_same_r(cuda, n, d):
    A = _randn(n, d).to(cuda)
    assert torch.equal(LA.house_tsqr(A, want_q=False)[1], LA.house_tsqr(A)[1])
    assert LA.house_tsqr(A, want_q=False)[0] is None


# --------------------------------------------------------------------------------- scale
@pytest.mark.parametrize("k", [300, -300, 520, -520])
def test_power_of_two_scale_is_exact(cuda, k):
    """Every operation of the kernels commutes with a power-of-two scale while nothing
    leaves the fp64 range: Q is bit-identical and R scales exactly. At k = +-520 the squares
    of the unscaled column norm would leave the range (inf / 0); ``house_tsqr`` factors
    A / 2^e with |A|_max / 2^e in [1/2, 1), so these meet the same identity. (Unscaled, on
    the MI355X: k = +520 gave NaN in every element of Q and 299 of R; k = -520 a finite but
    wrong factorisation, |Q R - A| / |A|_max = 2.4e-12 with sig flushed to 0. k = +-300 was
    bit-exact before the prescale too, and ordinary inputs give the same bits with it.)"""
    A = _randn(513, 24).to(cuda)
    Q0, R0 = LA.house_tsqr(A)
    Qk, Rk = LA.house_tsqr(A * 2.0**k)
    assert bool(torch.isfinite(Qk).all()) and bool(torch.isfinite(Rk).all())
    assert torch.equal(Qk, Q0)
    assert torch.equal(Rk, R0 * 2.0**k)


@pytest.mark.parametrize("bad", [float("inf"), float("-inf"), float("nan")])
def test_non_finite_input_is_refused(cuda, bad):
    A = _randn(300, 9).to(cuda)
    A[123, 4] = bad
    with pytest.raises(ValueError, match="non-finite"):
        LA.house_tsqr(A)
