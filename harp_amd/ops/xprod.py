"""Dense cross-products in fp64 (``csrc/xprod.hip``): the step-1 partial result of the DAAL
covariance / low-order moments / correlation PCA / linear and ridge regression family from one
pass over the rows. The rows (bf16, fp32 or fp64, unit column stride, any row stride) are read in
place and widened in registers; no fp64 copy, no shifted copy and no joined ``[X | Y]`` copy is
built.

* :func:`cross_products`: for the joined row ``z = [x | y]`` (``d + m <= MAX_D``) and a shift
  ``c``: ``S = sum (z - c)(z - c)^T`` on the fp64 matrix cores, ``s = sum (z - c)``, and the
  column minimum and maximum of the raw values, then the shift undone in fp64 on the device:
  ``xtx = S + c s^T + s c^T + n c c^T``, ``sum = s + n c``.
* :func:`col_moments`: the any-d form without the Gram: ``s``, ``sum (x - c)^2``, min, max.

Every sum has one fixed order (the rows of a workgroup's chunks, then the workgroups in order), so
the result is bitwise repeatable; integer-valued data is exact. A NaN propagates into min and max
as ``torch.min`` / ``torch.max`` do. ``n == 0`` launches nothing: zero sums, and min / max are
+inf / -inf (the identities of the workers' MIN / MAX all-reduce).

HIP tensors run the kernels (mandatory: a missing library raises). CPU tensors run the plain fp64
torch mirror of the same formulas; that is the gloo path.
"""
from __future__ import annotations

from typing import Dict, Optional

import torch

from . import _lib

_lib.register({
    "harp_xprod_max_d": [],
    "harp_xprod_grid": [_lib.c_long, _lib.c_int],
    "harp_xprod_record": [_lib.c_int],
    # X, dtx, ldx, d, Y, dty, ldy, m, n, c, partial, stream
    "harp_xprod_pass": [_lib.c_void_p, _lib.c_int, _lib.c_long, _lib.c_int, _lib.c_void_p, _lib.c_int, _lib.c_long,
                        _lib.c_int, _lib.c_long, _lib.c_void_p, _lib.c_void_p, _lib.c_void_p],
    # partial, records, w, out, stream
    "harp_xprod_reduce": [_lib.c_void_p, _lib.c_int, _lib.c_int, _lib.c_void_p, _lib.c_void_p],
    "harp_xprod_splits": [_lib.c_long, _lib.c_int],
    # X, dtype, ldx, d, n, c, partial, stream
    "harp_xprod_moments": [_lib.c_void_p, _lib.c_int, _lib.c_long, _lib.c_int, _lib.c_long, _lib.c_void_p,
                           _lib.c_void_p, _lib.c_void_p],
    # partial, splits, d, out, stream
    "harp_xprod_moments_reduce": [_lib.c_void_p, _lib.c_int, _lib.c_int, _lib.c_void_p, _lib.c_void_p],
})

MAX_D = 256   # mirrored from csrc/xprod.hip (XP_MAX_D; checked on first use)
_GRID = 512   # XP_GRID: the most workgroups (= records) of a pass
_DTYPES = {torch.bfloat16: 0, torch.float32: 1, torch.float64: 2}
_checked = False


def _record(w: int) -> int:
    """Doubles of a workgroup record at joined width w: the 16 x 16 upper blocks, then s, min, max."""
    nt = (w + 15) // 16
    return nt * (nt + 1) // 2 * 256 + 3 * 16 * nt


def _kernels():
    global _checked
    k = _lib.kernels()
    if not _checked:
        if k.harp_xprod_max_d() != MAX_D:
            raise RuntimeError(f"ops/xprod.py mirrors MAX_D = {MAX_D}, csrc/xprod.hip was built with "
                               f"{k.harp_xprod_max_d()}")
        for w in (1, 16, 17, MAX_D):
            if k.harp_xprod_record(w) != _record(w) or not 0 < k.harp_xprod_grid(1 << 40, w) <= _GRID:
                raise RuntimeError(f"ops/xprod.py and csrc/xprod.hip disagree on the records at width {w}")
        _checked = True
    return k


def check_width(w: int) -> None:
    if not 1 <= w <= MAX_D:
        raise ValueError(f"the native cross-products handle 1 to {MAX_D} columns (got {w}): use engine=\"torch\"")


def _check_rows(X: torch.Tensor) -> None:
    if X.layout != torch.strided or X.dim() != 2:
        raise ValueError(f"the native cross-products read dense rows [n, d] (got {X.layout}): use engine=\"torch\"")
    if X.shape[0] > 0 and X.shape[1] < 1:
        raise ValueError("the native cross-products need at least one column")
    if X.shape[0] > 1 and X.stride(0) < X.shape[1] or X.shape[0] > 0 and X.shape[1] > 1 and X.stride(1) != 1:
        raise ValueError("the native cross-products read rows of unit column stride: use engine=\"torch\"")
    if X.device.type == "cuda" and X.dtype not in _DTYPES:
        raise ValueError(f"the native cross-products read bf16, fp32 or fp64 rows (got {X.dtype}): "
                         "use engine=\"torch\"")


def _ld(X: torch.Tensor) -> int:
    return X.stride(0) if X.shape[0] > 1 else X.shape[1]


def _shift(shift: Optional[torch.Tensor], blocks, w: int, dev) -> torch.Tensor:
    if shift is not None:
        c = shift.reshape(-1).to(dev, torch.float64).contiguous()
        if c.numel() != w:
            raise ValueError(f"expected a shift of {w} values (got {c.numel()})")
        return c
    if blocks[0].shape[0] == 0:
        return torch.zeros(w, dtype=torch.float64, device=dev)
    return torch.cat([B[0].double() for B in blocks])


def _unshift(n: int, c: torch.Tensor, s: torch.Tensor, S: torch.Tensor):
    cs = torch.outer(c, s)
    return s + n * c, S + cs + cs.t() + n * torch.outer(c, c)


def cross_products(X: torch.Tensor, Y: Optional[torch.Tensor] = None,
                   shift: Optional[torch.Tensor] = None) -> Dict[str, torch.Tensor]:
    """``n`` [1], ``sum`` [w], ``xtx`` [w, w], ``min``, ``max`` [w] of the joined rows ``[X | Y]``
    (w = d + m) in fp64 on X's device, and the shifted pieces they were formed from: ``shift`` (c;
    default: the first row), ``shifted_sum`` (s) and ``shifted_xtx`` (S)."""
    _check_rows(X)
    blocks = [X]
    if Y is not None:
        _check_rows(Y)
        if Y.shape[0] != X.shape[0] or Y.device != X.device:
            raise ValueError(f"the two blocks need the same rows on one device (got {tuple(X.shape)} on {X.device} "
                             f"and {tuple(Y.shape)} on {Y.device})")
        if Y.shape[1] > 0:
            blocks.append(Y)
    n, d = X.shape
    m = blocks[1].shape[1] if len(blocks) > 1 else 0
    w = d + m
    check_width(w)
    dev = X.device
    c = _shift(shift, blocks, w, dev)
    if n == 0:
        s = torch.zeros(w, dtype=torch.float64, device=dev)
        S = torch.zeros((w, w), dtype=torch.float64, device=dev)
        mn, mx = torch.full_like(s, float("inf")), torch.full_like(s, -float("inf"))
    elif not _lib.use_native(X):
        Z = torch.cat([B.double() for B in blocks], 1)
        Zc = Z - c
        S, s = Zc.t() @ Zc, Zc.sum(0)
        mn, mx = Z.min(0).values, Z.max(0).values
    else:
        k = _kernels()
        Yb = blocks[1] if m else X
        records = k.harp_xprod_grid(n, w)
        partial = torch.empty(records * _record(w), dtype=torch.float64, device=dev)
        out = torch.empty(w * w + 3 * w, dtype=torch.float64, device=dev)
        stream = _lib.stream_ptr(dev)
        _lib.check(k.harp_xprod_pass(X.data_ptr(), _DTYPES[X.dtype], _ld(X), d, Yb.data_ptr(), _DTYPES[Yb.dtype],
                                     _ld(Yb), m, n, c.data_ptr(), partial.data_ptr(), stream), "xprod_pass")
        _lib.check(k.harp_xprod_reduce(partial.data_ptr(), records, w, out.data_ptr(), stream), "xprod_reduce")
        S = out[:w * w].view(w, w)
        s, mn, mx = out[w * w:].view(3, w)
    total, xtx = _unshift(n, c, s, S)
    return {"n": torch.tensor([float(n)], dtype=torch.float64, device=dev), "sum": total, "xtx": xtx, "min": mn,
            "max": mx, "shift": c, "shifted_sum": s, "shifted_xtx": S}


def col_moments(X: torch.Tensor, shift: Optional[torch.Tensor] = None) -> Dict[str, torch.Tensor]:
    """``n`` [1], ``sum``, ``sumsq``, ``min``, ``max`` [d] of the columns of X (any d) in fp64 on X's
    device, with ``shift`` (c; default: the first row), ``shifted_sum = sum (x - c)`` and
    ``shifted_sumsq = sum (x - c)^2``."""
    _check_rows(X)
    n, d = X.shape
    dev = X.device
    c = _shift(shift, [X], d, dev)
    if n == 0:
        s = torch.zeros(d, dtype=torch.float64, device=dev)
        q = torch.zeros_like(s)
        mn, mx = torch.full_like(s, float("inf")), torch.full_like(s, -float("inf"))
    elif not _lib.use_native(X):
        Xd = X.double()
        Xc = Xd - c
        s, q = Xc.sum(0), (Xc * Xc).sum(0)
        mn, mx = Xd.min(0).values, Xd.max(0).values
    else:
        k = _kernels()
        splits = k.harp_xprod_splits(n, d)
        partial = torch.empty(splits * 4 * d, dtype=torch.float64, device=dev)
        out = torch.empty((4, d), dtype=torch.float64, device=dev)
        stream = _lib.stream_ptr(dev)
        _lib.check(k.harp_xprod_moments(X.data_ptr(), _DTYPES[X.dtype], _ld(X), d, n, c.data_ptr(),
                                        partial.data_ptr(), stream), "xprod_moments")
        _lib.check(k.harp_xprod_moments_reduce(partial.data_ptr(), splits, d, out.data_ptr(), stream),
                   "xprod_moments_reduce")
        s, q, mn, mx = out
    return {"n": torch.tensor([float(n)], dtype=torch.float64, device=dev), "sum": s + n * c,
            "sumsq": q + 2 * c * s + n * c * c, "min": mn, "max": mx, "shift": c, "shifted_sum": s,
            "shifted_sumsq": q}
