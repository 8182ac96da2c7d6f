"""Dense multinomial naive Bayes in fp64 (``csrc/nb.hip``): per-class feature sums and counts
from one pass over the rows, and prediction on the fp64 matrix cores with the argmax fused. The
rows (bf16, fp32 or fp64, unit column stride, any row stride) are read in place and widened in
registers; no fp64 copy of X, no one-hot matrix and no ``[n, C]`` score tensor is built.

* :func:`class_sums`: ``sums[y[r]] += x_r``, ``counts[y[r]] += 1``, both fp64. Every sum has one
  fixed order (row pairs inside a row split, then the splits in order), so the result is bitwise
  repeatable; integer-valued data is exact. A label outside ``[0, C)`` raises ``ValueError``.
* :func:`predict`: ``argmax_c (x . log_theta[c] + log_prior[c])`` in fp64. Ties go to the lowest
  class. A NaN score never wins, and a row whose scores are all NaN gets label 0 (``torch.argmax``
  would return the position of the first NaN instead).

HIP tensors run the kernels (mandatory: a missing library raises). CPU tensors run the plain
fp64 torch mirror (``index_add_``; matmul, then the argmax with the rules above); that is the
gloo path.

Limits: ``C <= MAX_C``. Reference: DAAL multinomial_naive_bayes on a dense table (ml/daal
daal_naive/densedistri).
"""
from __future__ import annotations

import ctypes
from typing import Tuple

import torch

from . import _lib

_lib.register({
    "harp_nb_max_c": [],
    "harp_nb_splits": [_lib.c_long, _lib.c_int],
    # X, dtype, n, ldx, d, y, C, partial, err, stream
    "harp_nb_class_sums": [_lib.c_void_p, _lib.c_int, _lib.c_long, _lib.c_long, _lib.c_int, _lib.c_void_p, _lib.c_int,
                           _lib.c_void_p, _lib.c_void_p, _lib.c_void_p],
    # partial, splits, C, d, sums, counts, stream
    "harp_nb_reduce": [_lib.c_void_p, _lib.c_int, _lib.c_int, _lib.c_int, _lib.c_void_p, _lib.c_void_p,
                       _lib.c_void_p],
    "harp_nb_operand_doubles": [_lib.c_int, _lib.c_int],  # returns long
    # LT, ldt, C, d, W, stream
    "harp_nb_prepare": [_lib.c_void_p, _lib.c_long, _lib.c_int, _lib.c_int, _lib.c_void_p, _lib.c_void_p],
    # X, dtype, n, ldx, d, W, prior, C, labels, stream
    "harp_nb_predict": [_lib.c_void_p, _lib.c_int, _lib.c_long, _lib.c_long, _lib.c_int, _lib.c_void_p, _lib.c_void_p,
                        _lib.c_int, _lib.c_void_p, _lib.c_void_p],
})

MAX_C = 64    # mirrored from csrc/nb.hip (NB_MAX_C; checked on first use)
_TILE = 256   # NB_TILE: columns of a class-sums workgroup
_GRID = 512   # NB_GRID: its workgroups
_DTYPES = {torch.bfloat16: 0, torch.float32: 1, torch.float64: 2}
_checked = False


def _kernels():
    global _checked
    k = _lib.kernels()
    if not _checked:
        if k.harp_nb_max_c() != MAX_C:
            raise RuntimeError(f"ops/nb.py mirrors MAX_C = {MAX_C}, csrc/nb.hip was built with {k.harp_nb_max_c()}")
        for d in (1, _TILE, _TILE + 1, 3 * _TILE):
            if k.harp_nb_splits(1 << 40, d) * (d + 1) * 8 != partial_bytes(d, 1):
                raise RuntimeError(f"ops/nb.py and csrc/nb.hip disagree on the row splits at width {d}")
        k.harp_nb_operand_doubles.restype = ctypes.c_long
        _checked = True
    return k


def check_classes(C: int) -> None:
    if not 1 <= C <= MAX_C:
        raise ValueError(f"the native naive Bayes handles 1 to {MAX_C} classes (got {C}): use engine=\"torch\"")


def partial_bytes(d: int, C: int) -> int:
    """Upper bound, over n, of the bytes of the row-split partials of :func:`class_sums`."""
    tiles = (d + _TILE - 1) // _TILE
    return max(1, _GRID // tiles) * C * (d + 1) * 8


def _check_rows(X: torch.Tensor) -> None:
    if X.layout != torch.strided or X.dim() != 2:
        raise ValueError(f"the native naive Bayes reads dense rows [n, d] (got {X.layout}): use engine=\"torch\"")
    if X.shape[0] > 0 and X.shape[1] < 1:
        raise ValueError("the native naive Bayes needs at least one column")
    if X.shape[0] > 1 and X.stride(0) < X.shape[1] or X.shape[0] > 0 and X.shape[1] > 1 and X.stride(1) != 1:
        raise ValueError("the native naive Bayes reads rows of unit column stride: use engine=\"torch\"")
    if X.device.type == "cuda" and X.dtype not in _DTYPES:
        raise ValueError(f"the native naive Bayes reads bf16, fp32 or fp64 rows (got {X.dtype}): "
                         "use engine=\"torch\"")


def class_sums(X: torch.Tensor, y: torch.Tensor, num_classes: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """(sums [C, d], counts [C]) in fp64 on X's device, for labels y [n] in [0, C)."""
    check_classes(num_classes)
    _check_rows(X)
    n, d = X.shape
    C = num_classes
    dev = X.device
    assert y.numel() == n
    sums = torch.zeros((C, d), dtype=torch.float64, device=dev)
    counts = torch.zeros(C, dtype=torch.float64, device=dev)
    if n == 0:
        return sums, counts
    if not _lib.use_native(X):
        yl = y.reshape(-1).long().to(dev)
        if int(yl.min()) < 0 or int(yl.max()) >= C:
            raise ValueError(f"label outside [0, {C})")
        sums.index_add_(0, yl, X.double())
        return sums, torch.bincount(yl, minlength=C).double()
    k = _kernels()
    y32 = y.reshape(-1).to(dev, torch.int32).contiguous()
    splits = k.harp_nb_splits(n, d)
    partial = torch.empty(splits * C * (d + 1), dtype=torch.float64, device=dev)
    err = torch.zeros(1, dtype=torch.int32, device=dev)
    stream = _lib.stream_ptr(dev)
    ldx = X.stride(0) if n > 1 else d
    _lib.check(k.harp_nb_class_sums(X.data_ptr(), _DTYPES[X.dtype], n, ldx, d, y32.data_ptr(), C, partial.data_ptr(),
                                    err.data_ptr(), stream), "nb_class_sums")
    _lib.check(k.harp_nb_reduce(partial.data_ptr(), splits, C, d, sums.data_ptr(), counts.data_ptr(), stream),
               "nb_reduce")
    if int(err) != 0:
        raise ValueError(f"label outside [0, {C})")
    return sums, counts


def _argmax_rule(S: torch.Tensor) -> torch.Tensor:
    """Row argmax: ties to the lowest column, a NaN never wins, a row of NaNs gives 0."""
    C = S.shape[1]
    ok = ~torch.isnan(S)
    S = torch.where(ok, S, torch.full_like(S, -float("inf")))
    idx = torch.arange(C, device=S.device).expand_as(S)
    win = torch.where(ok & (S == S.max(1, keepdim=True).values), idx, torch.full_like(idx, C)).min(1).values
    return torch.where(win == C, torch.zeros_like(win), win)


def predict(X: torch.Tensor, log_theta: torch.Tensor, log_prior: torch.Tensor) -> torch.Tensor:
    """int64 labels [n] of the rows of X [n, d] under log_theta [C, d] and log_prior [C]."""
    C = log_theta.shape[0]
    check_classes(C)
    _check_rows(X)
    n, d = X.shape
    dev = X.device
    if log_theta.dim() != 2 or log_theta.shape[1] != d or log_prior.numel() != C:
        raise ValueError(f"expected log_theta [C, {d}] and log_prior [C] (got {tuple(log_theta.shape)} and "
                         f"{tuple(log_prior.shape)})")
    if n == 0:
        return torch.empty(0, dtype=torch.int64, device=dev)
    lt = log_theta.to(dev, torch.float64)
    lp = log_prior.reshape(-1).to(dev, torch.float64)
    if not _lib.use_native(X):
        return _argmax_rule(X.double() @ lt.t() + lp)
    k = _kernels()
    lt, lp = lt.contiguous(), lp.contiguous()
    W = torch.empty(k.harp_nb_operand_doubles(C, d), dtype=torch.float64, device=dev)
    labels = torch.empty(n, dtype=torch.int32, device=dev)
    stream = _lib.stream_ptr(dev)
    _lib.check(k.harp_nb_prepare(lt.data_ptr(), d, C, d, W.data_ptr(), stream), "nb_prepare")
    ldx = X.stride(0) if n > 1 else d
    _lib.check(k.harp_nb_predict(X.data_ptr(), _DTYPES[X.dtype], n, ldx, d, W.data_ptr(), lp.data_ptr(), C,
                                 labels.data_ptr(), stream), "nb_predict")
    return labels.long()
