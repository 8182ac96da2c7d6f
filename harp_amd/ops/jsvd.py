"""One-sided (Hestenes) Jacobi SVD of a small fp64 matrix (``csrc/jsvd.hip``): the d x d step
of the native SVD.

For a tall block ``X = Q R`` only the factor is left to decompose, and :func:`svd_small`
returns ``M = Z diag(s) W^T`` for a square ``M``:

* the pair (p, q), p < q, gives ``alpha = |m_p|^2``, ``beta = |m_q|^2``, ``gamma = m_p . m_q``,
  formed fresh at every visit; it is skipped when ``|gamma| <= tol sqrt(alpha beta)`` with
  ``tol = sqrt(d) 2^-53`` (LAPACK ``dgesvj``), so a zero column never rotates;
* otherwise ``zeta = (beta - alpha) / (2 gamma)``, ``t = sign(zeta) / (|zeta| + sqrt(1 + zeta^2))``
  (1 for ``zeta = 0``), ``c = 1 / sqrt(1 + t^2)``, ``sn = c t``, ``m_p' = c m_p - sn m_q``,
  ``m_q' = sn m_p + c m_q``, and the same rotation on the columns of ``W`` (which starts as I);
* the pairs come in round-robin tournament order over ``Wp`` = d rounded up to even slots: at
  step s slot i < Wp-1 meets ``(2 s - i) mod (Wp-1)``, slot s meets slot Wp-1;
* a sweep without a rotation ends the iteration (``sweeps`` = sweeps run, -1 after
  ``MAX_SWEEPS``);
* ``s`` = the column norms in descending order (ties by column index), ``Z`` the normalised
  columns, ``W`` the rotations' columns in the same order. A column of exactly zero norm gives
  ``s = 0`` and a zero column of ``Z``: ``Z`` is not completed to a basis. Tiny non-zero
  columns come out orthonormal, because the stopping rule is relative.

Singular values of a column-scaled matrix ``B D`` come out to high relative accuracy
(about ``d eps cond(B)``), which a bidiagonalisation does not give.

HIP tensors run the kernel (mandatory: a missing library raises). CPU tensors run the fp64
torch mirror of the same rules; it is the gloo path and the sparring partner of the GPU
tests. The kernel is bitwise repeatable, so every rank of a distributed run gets the same bits
from the same all-gathered factor.

Limit: ``d <= MAX_D`` (one wave up to 64 columns, one workgroup up to 128). Reference: DAAL
``svd`` step 2 (ml/daal daal_svd, SVDDaalCollectiveMapper).
"""
from __future__ import annotations

import math
from typing import Optional, Tuple

import torch

from . import _lib

_lib.register({
    "harp_jsvd_max_d": [],
    # M, ld, d, want_w, Z, s, W, sweeps, stream
    "harp_jsvd_small": [_lib.c_void_p, _lib.c_long, _lib.c_int, _lib.c_int, _lib.c_void_p, _lib.c_void_p,
                        _lib.c_void_p, _lib.c_void_p, _lib.c_void_p],
})

MAX_D = 128  # mirrored from csrc/jsvd.hip (JSVD_MAX_D; checked against harp_jsvd_max_d on first use)
MAX_SWEEPS = 60  # JSVD_MAX_SWEEPS
_checked = False


def _kernels():
    global _checked
    k = _lib.kernels()
    if not _checked:
        if k.harp_jsvd_max_d() != MAX_D:
            raise RuntimeError(f"ops/jsvd.py mirrors MAX_D = {MAX_D}, csrc/jsvd.hip was built with {k.harp_jsvd_max_d()}")
        _checked = True
    return k


def check_width(d: int) -> None:
    if not 1 <= d <= MAX_D:
        raise ValueError(f"the native SVD handles 1 to {MAX_D} columns (got {d}): use engine=\"torch\"")


def _mirror(M: torch.Tensor, want_w: bool):
    """The kernel's rules in fp64 torch on the CPU (sums in torch's order, not the kernel's)."""
    d = M.shape[0]
    Wp = (d + 1) & ~1
    n = Wp - 1
    a = torch.zeros((d, Wp), dtype=torch.float64)
    a[:, :d] = M
    w = torch.eye(d, Wp, dtype=torch.float64) if want_w else None
    tol = math.sqrt(d) * 2.0 ** -53
    slots = torch.arange(n)
    sweeps = -1
    for sweep in range(1, MAX_SWEEPS + 1):
        rotated = False
        for s in range(n):
            pr = (2 * s - slots) % n
            pr[s] = n
            lo, hi = slots[slots < pr], pr[slots < pr]  # each pair once, from its lower slot
            ap, aq = a[:, lo], a[:, hi]
            alpha, beta, gamma = (ap * ap).sum(0), (aq * aq).sum(0), (ap * aq).sum(0)
            rot = gamma.abs() > tol * (alpha * beta).sqrt()
            if not bool(rot.any()):
                continue
            rotated = True
            lo, hi, ap, aq = lo[rot], hi[rot], ap[:, rot], aq[:, rot]
            zeta = (beta[rot] - alpha[rot]) / (2.0 * gamma[rot])
            sg = torch.where(zeta < 0, -torch.ones_like(zeta), torch.ones_like(zeta))
            t = torch.where(zeta == 0, torch.ones_like(zeta), sg / (zeta.abs() + (1.0 + zeta * zeta).sqrt()))
            c = 1.0 / (1.0 + t * t).sqrt()
            sn = c * t
            a[:, lo], a[:, hi] = c * ap - sn * aq, sn * ap + c * aq
            if want_w:
                wp, wq = w[:, lo], w[:, hi]
                w[:, lo], w[:, hi] = c * wp - sn * wq, sn * wp + c * wq
        if not rotated:
            sweeps = sweep
            break
    a = a[:, :d]
    sig = (a * a).sum(0).sqrt()
    order = torch.sort(sig, descending=True, stable=True).indices  # ties: the lower column first
    sig, a = sig[order], a[:, order]
    Z = torch.where(sig > 0, a / torch.where(sig > 0, sig, torch.ones_like(sig)), torch.zeros_like(a))
    return Z, sig, (w[:, :d][:, order].contiguous() if want_w else None), torch.tensor(sweeps, dtype=torch.int32)


def svd_small(M: torch.Tensor, want_w: bool = True) -> Tuple[torch.Tensor, torch.Tensor, Optional[torch.Tensor],
                                                              torch.Tensor]:
    """``(Z, s, W, sweeps)`` with ``M = Z diag(s) W^T`` for a square fp64 ``M`` [d, d], d <= MAX_D,
    on M's device: ``s`` descending, ``W`` orthogonal (None without ``want_w``), ``sweeps`` an
    int32 scalar tensor (-1: no convergence within MAX_SWEEPS)."""
    if M.dim() != 2 or M.shape[0] != M.shape[1] or M.dtype != torch.float64:
        raise ValueError(f"expected a square fp64 matrix (got {M.dtype} {tuple(M.shape)})")
    d = M.shape[0]
    check_width(d)
    # the squared column norms are formed unscaled, so the matrix is scaled by a power of two
    # into [1/2, 1) exactly as qrcp_small does, and s scaled back: no bit of the result changes
    # for input that was in range before
    amax = float(M.abs().max())
    if not math.isfinite(amax):
        raise ValueError("svd_small: the matrix holds a non-finite entry")
    e = math.frexp(amax)[1] if amax > 0.0 else 0
    A = (M if e == 0 else (M * 2.0 ** (-(e // 2))) * 2.0 ** (-(e - e // 2))).contiguous()
    if _lib.use_native(M):
        k = _kernels()
        Z = torch.empty((d, d), dtype=torch.float64, device=M.device)
        s = torch.empty(d, dtype=torch.float64, device=M.device)
        W = torch.empty((d, d), dtype=torch.float64, device=M.device) if want_w else None
        sweeps = torch.empty((), dtype=torch.int32, device=M.device)
        _lib.check(k.harp_jsvd_small(A.data_ptr(), d, d, int(want_w), Z.data_ptr(), s.data_ptr(), _lib.ptr(W),
                                     sweeps.data_ptr(), _lib.stream_ptr(M.device)), "jsvd_small")
    else:
        Z, s, W, sweeps = _mirror(A, want_w)
    if e != 0:
        s = (s * 2.0 ** (e // 2)) * 2.0 ** (e - e // 2)
    return Z, s, W, sweeps
