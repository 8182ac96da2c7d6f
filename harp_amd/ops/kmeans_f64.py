"""Dense K-means step in fp64 (``csrc/kmeans_f64.hip``): exact nearest-centroid labels on the
fp64 matrix cores, then sums, counts and the within-cluster sum of squares from one pass over
the label-sorted rows. No tensor proportional to n * K is built, and the points (bf16, fp32 or
fp64, unit column stride, any row stride) are read in place and widened in registers.

* :func:`assign`: ``labels[i] = argmin_k (|c_k|^2 - 2 x_i . c_k)`` in fp64, ties to the lowest
  index; a row whose distances are all NaN gets label 0. Bitwise repeatable.
* :func:`assign_accumulate`: the labels, then ``sums[k] = sum of the rows of cluster k``,
  ``counts[k]`` and ``wss[k] = sum |x - c_k|^2`` formed directly from ``x - c_k`` (no
  ``|x|^2 + |c|^2 - 2 x.c`` cancellation). The rows are bucketed by ``ops.segment.bucket_labels``;
  ``counts`` are the bucket sizes (exact). Partial sums meet in memory by fp64 atomic adds, so
  ``sums`` and ``wss`` are exact up to the order of those adds and not bitwise repeatable.

HIP tensors run the kernels (mandatory: a missing library raises). CPU tensors run the torch
formula of ``models/kmeans_csr.py`` (argmin of the expanded distance, ``index_add_`` sums) with
``wss`` in the direct form; that is the gloo path.

Limits: ``1 <= d <= MAX_D``, ``K <= MAX_K`` (the counting sort's). Reference: DAAL kmeans
DistributedStep1Local on a dense table (ml/daal daal_kmeans/regroupallgather).
"""
from __future__ import annotations

import ctypes
from typing import Tuple

import torch

from . import _lib
from . import segment as SG

_lib.register({
    "harp_kmeans_f64_max_d": [],
    "harp_kmeans_f64_param": [_lib.c_int, _lib.c_int],
    "harp_kmeans_f64_operand_doubles": [_lib.c_int, _lib.c_int],  # returns long
    # C, ldc, K, d, W, stream
    "harp_kmeans_f64_prepare": [_lib.c_void_p, _lib.c_long, _lib.c_int, _lib.c_int, _lib.c_void_p, _lib.c_void_p],
    # X, dtype, n, ldx, d, W, K, labels, stream
    "harp_kmeans_f64_assign": [_lib.c_void_p, _lib.c_int, _lib.c_long, _lib.c_long, _lib.c_int, _lib.c_void_p,
                               _lib.c_int, _lib.c_void_p, _lib.c_void_p],
    # X, dtype, n, ldx, d, C, perm, start, K, sums, wss, stream
    "harp_kmeans_f64_sums": [_lib.c_void_p, _lib.c_int, _lib.c_long, _lib.c_long, _lib.c_int, _lib.c_void_p,
                             _lib.c_void_p, _lib.c_void_p, _lib.c_int, _lib.c_void_p, _lib.c_void_p, _lib.c_void_p],
})

MAX_D = 256    # mirrored from csrc/kmeans_f64.hip (KMF_MAX_D; checked on first use)
MAX_K = 16384  # KMF_MAX_K
_STEPS = (1, 2, 4, 8, 16, 24, 28, 32, 48, 64)  # kmf_steps: MFMA steps per row, the padded width is 4 S
_DTYPES = {torch.bfloat16: 0, torch.float32: 1, torch.float64: 2}
_checked = False


def _steps(d: int) -> int:
    return next(s for s in _STEPS if 4 * s >= d)


def padded_width(d: int) -> int:
    return 4 * _steps(d)


def stage_centroids(d: int) -> int:
    """Centroids of one LDS stage of the assign kernel at width d."""
    return 16 * (min(16, max(2, 64 // _steps(d))) & ~1)


def points_per_workgroup(d: int) -> int:
    return 128 if _steps(d) <= 32 else 64


def _kernels():
    global _checked
    k = _lib.kernels()
    if not _checked:
        if k.harp_kmeans_f64_max_d() != MAX_D:
            raise RuntimeError(f"ops/kmeans_f64.py mirrors MAX_D = {MAX_D}, csrc/kmeans_f64.hip was built with "
                               f"{k.harp_kmeans_f64_max_d()}")
        for d in range(1, MAX_D + 1):
            mine = (padded_width(d), stage_centroids(d), points_per_workgroup(d))
            built = tuple(k.harp_kmeans_f64_param(w, d) for w in range(3))
            if mine != built:
                raise RuntimeError(f"ops/kmeans_f64.py mirrors {mine} at width {d}, csrc/kmeans_f64.hip has {built}")
        k.harp_kmeans_f64_operand_doubles.restype = ctypes.c_long
        _checked = True
    return k


def check_width(d: int) -> None:
    if not 1 <= d <= MAX_D:
        raise ValueError(f"the native fp64 K-means handles 1 to {MAX_D} columns (got {d}): use engine=\"torch\"")


def _check(X: torch.Tensor, C: torch.Tensor) -> None:
    if X.dim() != 2 or C.dim() != 2 or X.shape[1] != C.shape[1] or X.layout != torch.strided:
        raise ValueError(f"expected dense X [n, d] and C [K, d] (got {tuple(X.shape)} and {tuple(C.shape)})")
    check_width(X.shape[1])
    if not 1 <= C.shape[0] <= MAX_K:
        raise ValueError(f"the native fp64 K-means handles 1 to {MAX_K} centroids (got {C.shape[0]}): "
                         "use engine=\"torch\"")
    if C.dtype != torch.float64 or C.device != X.device:
        raise ValueError("the centroids are fp64 on the device of X")


def _native_rows(X: torch.Tensor) -> None:
    if X.dtype not in _DTYPES:
        raise ValueError(f"the native fp64 K-means reads bf16, fp32 or fp64 rows (got {X.dtype}): use engine=\"torch\"")
    if X.shape[0] > 1 and (X.stride(1) != 1 or X.stride(0) < X.shape[1]) or X.shape[0] >= 2 ** 31:
        raise ValueError("the native fp64 K-means reads rows of unit column stride, fewer than 2^31 of them")


def _sq_dist(X: torch.Tensor, C: torch.Tensor) -> torch.Tensor:
    Xd = X.double()
    return ((Xd ** 2).sum(1)[:, None] + (C * C).sum(1)[None, :] - 2 * (Xd @ C.t())).clamp_min(0)


def _assign_native(X: torch.Tensor, C: torch.Tensor) -> torch.Tensor:
    k = _kernels()
    n, d = X.shape
    K = C.shape[0]
    labels = torch.empty(n, dtype=torch.int32, device=X.device)
    if n == 0:
        return labels
    Cc = C.contiguous()
    W = torch.empty(k.harp_kmeans_f64_operand_doubles(K, d), dtype=torch.float64, device=X.device)
    stream = _lib.stream_ptr(X.device)
    _lib.check(k.harp_kmeans_f64_prepare(Cc.data_ptr(), d, K, d, W.data_ptr(), stream), "kmeans_f64_prepare")
    ldx = X.stride(0) if n > 1 else d
    _lib.check(k.harp_kmeans_f64_assign(X.data_ptr(), _DTYPES[X.dtype], n, ldx, d, W.data_ptr(), K,
                                        labels.data_ptr(), stream), "kmeans_f64_assign")
    return labels


def assign(X: torch.Tensor, C: torch.Tensor) -> torch.Tensor:
    """int32 labels [n] of the rows of X [n, d] among the fp64 centroids C [K, d]."""
    _check(X, C)
    if _lib.use_native(X):
        _native_rows(X)
        return _assign_native(X, C)
    if X.shape[0] == 0:
        return torch.empty(0, dtype=torch.int32)
    return _sq_dist(X, C).min(1)[1].to(torch.int32)


def assign_accumulate(X: torch.Tensor, C: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor,
                                                                   torch.Tensor]:
    """(labels int32 [n], sums [K, d], counts [K], wss [K]), the last three fp64, on X's device."""
    labels = assign(X, C)
    n, d = X.shape
    K = C.shape[0]
    sums = torch.zeros((K, d), dtype=torch.float64, device=X.device)
    wss = torch.zeros(K, dtype=torch.float64, device=X.device)
    if n == 0:
        return labels, sums, torch.zeros_like(wss), wss
    if not _lib.use_native(X):
        Xd, lab = X.double(), labels.long()
        sums.index_add_(0, lab, Xd)
        wss.index_add_(0, lab, ((Xd - C[lab]) ** 2).sum(1))
        return labels, sums, torch.bincount(lab, minlength=K).double(), wss
    perm, start = SG.bucket_labels(labels, K)
    Cc = C.contiguous()
    ldx = X.stride(0) if n > 1 else d
    _lib.check(_kernels().harp_kmeans_f64_sums(X.data_ptr(), _DTYPES[X.dtype], n, ldx, d, Cc.data_ptr(),
                                               perm.data_ptr(), start.data_ptr(), K, sums.data_ptr(),
                                               wss.data_ptr(), _lib.stream_ptr(X.device)), "kmeans_f64_sums")
    return labels, sums, (start[1:] - start[:-1]).double(), wss
