"""Column-pivoted QR of a small fp64 matrix (``csrc/pqr.hip``): the d x d step of the native
rank-revealing QR.

For a tall block ``X = Q1 R1`` every pivot decision depends on ``R1`` alone, so
``X P = Q1 (R1 P) = (Q1 Q2) R2`` and :func:`qrcp_small` factors ``R1 [:, perm] = Q2 R2``:

* pivot at step k = the free column with the largest squared norm over rows k.., formed fresh
  at every step (no downdating), ties to the lowest current slot, slots swapped as LAPACK
  swaps columns;
* reflectors in LAPACK's ``dlarfg`` form, a zero residual gives ``tau = 0``;
* ``R2`` upper triangular with exact zeros below and a non-negative diagonal (the convention
  of ``ops.linalg.house_tsqr``), ``Q2`` explicit.

HIP tensors run the kernel (mandatory: a missing library raises). CPU tensors run the fp64
torch mirror of the same rules; it is the gloo path and the oracle of the GPU tests. The
kernel is bitwise repeatable, so every rank of a distributed run takes the same pivots from
the same ``R1``.

Limit: ``d <= MAX_D`` (one wave up to 64 columns, one workgroup with the matrix in LDS up to
128). Reference: DAAL ``pivoted_qr`` (ml/daal daal_pivoted_qr, PQRDaalCollectiveMapper).
"""
from __future__ import annotations

import math
from typing import Tuple

import torch

from . import _lib

_lib.register({
    "harp_pqr_max_d": [],
    # A, ld, d, Q2, R2, perm, stream
    "harp_pqr_small": [_lib.c_void_p, _lib.c_long, _lib.c_int, _lib.c_void_p, _lib.c_void_p, _lib.c_void_p,
                       _lib.c_void_p],
})

MAX_D = 128  # mirrored from csrc/pqr.hip (PQR_MAX_D; checked against harp_pqr_max_d on first use)
_checked = False


def _kernels():
    global _checked
    k = _lib.kernels()
    if not _checked:
        if k.harp_pqr_max_d() != MAX_D:
            raise RuntimeError(f"ops/pqr.py mirrors MAX_D = {MAX_D}, csrc/pqr.hip was built with {k.harp_pqr_max_d()}")
        _checked = True
    return k


def check_width(d: int) -> None:
    if not 1 <= d <= MAX_D:
        raise ValueError(f"the native pivoted QR handles 1 to {MAX_D} columns (got {d}): use engine=\"host\"")


def _mirror(A: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """The kernel's rules in fp64 torch on the CPU (sums in torch's order, not the kernel's)."""
    d = A.shape[0]
    a = A.clone()
    slot = torch.arange(d)
    steps = []
    for k in range(d):
        alpha, sig = a[k], (a[k + 1:] * a[k + 1:]).sum(0)
        nrm = torch.where(slot >= k, alpha * alpha + sig, torch.full((d,), -math.inf, dtype=torch.float64))
        tied = (nrm == nrm.max()).nonzero()[:, 0]
        p = int(tied[slot[tied].argmin()])
        al, sg = float(alpha[p]), float(sig[p])
        beta, tau, sc = al, 0.0, 0.0
        if sg > 0.0:
            beta = -math.copysign(math.sqrt(al * al + sg), al)
            tau, sc = (beta - al) / beta, 1.0 / (al - beta)
        slot[slot == k] = slot[p]
        slot[p] = k
        v = torch.zeros(d, dtype=torch.float64)
        v[k] = 1.0
        v[k + 1:] = a[k + 1:, p] * sc
        upd = slot > k
        a[:, upd] -= torch.outer(v, tau * (v @ a[:, upd]))
        a[k, p] = beta
        a[k + 1:, p] = 0.0
        steps.append((v, tau, -1.0 if beta < 0.0 else 1.0))
    perm = torch.empty(d, dtype=torch.int32)
    perm[slot] = torch.arange(d, dtype=torch.int32)
    sgn = torch.tensor([s for _, _, s in steps], dtype=torch.float64)
    R2 = torch.triu(a[:, perm.long()]) * sgn[:, None]
    Q2 = torch.eye(d, dtype=torch.float64)
    for v, tau, _ in reversed(steps):
        Q2 -= torch.outer(v, tau * (v @ Q2))
    return Q2 * sgn[None, :], R2, perm


def qrcp_small(R: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """``(Q2, R2, perm)`` with ``R[:, perm] = Q2 R2`` for a square fp64 ``R`` [d, d], d <= MAX_D,
    on R's device; ``perm`` is int32."""
    if R.dim() != 2 or R.shape[0] != R.shape[1] or R.dtype != torch.float64:
        raise ValueError(f"expected a square fp64 matrix (got {R.dtype} {tuple(R.shape)})")
    d = R.shape[0]
    check_width(d)
    # reflector norms are formed unscaled, so the matrix is scaled by a power of two into
    # [1/2, 1) exactly as house_tsqr does, and R2 scaled back: no bit of the result changes
    # for input that was in range before
    amax = float(R.abs().max())
    if not math.isfinite(amax):
        raise ValueError("qrcp_small: the matrix holds a non-finite entry")
    e = math.frexp(amax)[1] if amax > 0.0 else 0
    A = (R if e == 0 else (R * 2.0 ** (-(e // 2))) * 2.0 ** (-(e - e // 2))).contiguous()
    if _lib.use_native(R):
        k = _kernels()
        Q2 = torch.empty((d, d), dtype=torch.float64, device=R.device)
        R2 = torch.empty((d, d), dtype=torch.float64, device=R.device)
        perm = torch.empty(d, dtype=torch.int32, device=R.device)
        _lib.check(k.harp_pqr_small(A.data_ptr(), d, d, Q2.data_ptr(), R2.data_ptr(), perm.data_ptr(),
                                    _lib.stream_ptr(R.device)), "pqr_small")
    else:
        Q2, R2, perm = _mirror(A)
    if e != 0:
        R2 = (R2 * 2.0 ** (e // 2)) * 2.0 ** (e - e // 2)
    return Q2, R2, perm
