"""Exact k-nearest-neighbour search in fp64 (``csrc/knn_f64.hip``): squared Euclidean distances
on the fp64 matrix cores with the top-k fused into the sweep. No tensor proportional to M * N is
built; training rows and queries (bf16, fp32 or fp64, unit column stride, any row stride) are read
in place and widened in registers.

* :func:`prepare`: the sweep operand of the training rows. It depends on them alone, so a
  classifier prepares it once and every search reuses it.
* :func:`knn_search`: ``(distances [M, min(k, N)] fp64 ascending, indices int64)``, ties to the
  lower training index, bitwise repeatable. A slot that no non-NaN distance fills is ``(inf, -1)``.
  The training rows are swept in ``splits`` contiguous ranges by separate workgroups (the
  launcher's choice fills the chip when there are few queries) and the ranges' lists merged.

HIP tensors run the kernels (mandatory: a missing library raises). CPU tensors run the torch
formula in fp64, ``(qn + tn - 2 Q T^T).clamp_min(0)`` over query tiles with a stable sort on
(distance, index); that is the gloo path and the mirror. There ``prepare`` returns the squared
norms of the training rows.

Limits: ``1 <= d <= MAX_D``, ``1 <= k <= MAX_K``, fewer than 2^31 training rows. Reference: DAAL
kdtree_knn_classification prediction (ml/daal daal_knn).
"""
from __future__ import annotations

import ctypes
from typing import Optional, Tuple

import torch

from . import _lib

_lib.register({
    "harp_knn_f64_max_d": [],
    "harp_knn_f64_max_k": [],
    "harp_knn_f64_param": [_lib.c_int, _lib.c_int, _lib.c_int],
    "harp_knn_f64_operand_doubles": [_lib.c_long, _lib.c_int],  # returns long
    # T, dtype, N, ldt, d, W, stream
    "harp_knn_f64_prepare": [_lib.c_void_p, _lib.c_int, _lib.c_long, _lib.c_long, _lib.c_int, _lib.c_void_p,
                             _lib.c_void_p],
    "harp_knn_f64_splits": [_lib.c_long, _lib.c_long, _lib.c_int, _lib.c_int],
    # Q, dtype, M, ldq, d, W, N, k, splits, outD, outI, stream
    "harp_knn_f64_search": [_lib.c_void_p, _lib.c_int, _lib.c_long, _lib.c_long, _lib.c_int, _lib.c_void_p,
                            _lib.c_long, _lib.c_int, _lib.c_int, _lib.c_void_p, _lib.c_void_p, _lib.c_void_p],
    # pd, pi, splits, M, k, outD, outI, stream
    "harp_knn_f64_merge": [_lib.c_void_p, _lib.c_void_p, _lib.c_int, _lib.c_long, _lib.c_int, _lib.c_void_p,
                           _lib.c_void_p, _lib.c_void_p],
})

MAX_D = 256       # mirrored from csrc/knn_f64.hip (KNF_MAX_D; checked on first use)
MAX_K = 32        # KNF_MAX_K
MAX_SPLITS = 1024  # KNF_MAX_SPLITS
_STEPS = (1, 2, 4, 8, 16, 32, 48, 64)  # knf_steps: MFMA steps per row, the padded width is 4 S
_DTYPES = {torch.bfloat16: 0, torch.float32: 1, torch.float64: 2}
_checked = False


def _steps(d: int) -> int:
    return next(s for s in _STEPS if 4 * s >= d)


def padded_width(d: int) -> int:
    return 4 * _steps(d)


def stage_rows(d: int) -> int:
    """Training rows of one LDS stage of the search kernel at width d."""
    return 16 * (min(16, max(2, 64 // _steps(d))) & ~1)


def list_length(k: int) -> int:
    return next(kk for kk in (4, 8, 16, 32) if kk >= k)


def queries_per_workgroup(d: int, k: int) -> int:
    return 128 if _steps(d) <= 16 and list_length(k) <= 16 else 64


def _kernels():
    global _checked
    lib = _lib.kernels()
    if not _checked:
        if (lib.harp_knn_f64_max_d(), lib.harp_knn_f64_max_k()) != (MAX_D, MAX_K):
            raise RuntimeError(f"ops/knn_f64.py mirrors MAX_D = {MAX_D} and MAX_K = {MAX_K}, csrc/knn_f64.hip was "
                               f"built with {lib.harp_knn_f64_max_d()} and {lib.harp_knn_f64_max_k()}")
        for d in range(1, MAX_D + 1):
            for k in (4, 8, 16, 32):
                mine = (padded_width(d), stage_rows(d), queries_per_workgroup(d, k))
                built = tuple(lib.harp_knn_f64_param(w, d, k) for w in range(3))
                if mine != built:
                    raise RuntimeError(f"ops/knn_f64.py mirrors {mine} at width {d}, k = {k}; csrc/knn_f64.hip "
                                       f"has {built}")
        lib.harp_knn_f64_operand_doubles.restype = ctypes.c_long
        _checked = True
    return lib


def check_width(d: int) -> None:
    if not 1 <= d <= MAX_D:
        raise ValueError(f"the native fp64 kNN handles 1 to {MAX_D} columns (got {d}): use engine=\"torch\"")


def check_k(k: int) -> None:
    if not 1 <= k <= MAX_K:
        raise ValueError(f"the native fp64 kNN handles 1 <= k <= {MAX_K} (got {k}): use engine=\"torch\"")


def _check_rows(X: torch.Tensor, what: str) -> None:
    if X.dim() != 2 or X.layout != torch.strided:
        raise ValueError(f"the native fp64 kNN reads dense {what} rows [n, d] (got {X.layout}, {tuple(X.shape)}): "
                         "use engine=\"torch\"")
    check_width(X.shape[1])
    if X.dtype not in _DTYPES:
        raise ValueError(f"the native fp64 kNN reads bf16, fp32 or fp64 rows (got {X.dtype}): use engine=\"torch\"")
    if X.shape[0] > 1 and (X.stride(1) != 1 or X.stride(0) < X.shape[1]) or X.shape[0] >= 2 ** 31:
        raise ValueError("the native fp64 kNN reads rows of unit column stride, fewer than 2^31 of them")


def _ld(X: torch.Tensor) -> int:
    return X.stride(0) if X.shape[0] > 1 else X.shape[1]


def prepare(train: torch.Tensor) -> torch.Tensor:
    """The reusable operand of the training rows [N, d]: the kernel's sweep operand on a HIP
    device, the fp64 squared norms on the CPU."""
    _check_rows(train, "training")
    N, d = train.shape
    if N < 1:
        raise ValueError("kNN needs at least one training row")
    if not _lib.use_native(train):
        return (train.double() ** 2).sum(1)
    lib = _kernels()
    W = torch.empty(lib.harp_knn_f64_operand_doubles(N, d), dtype=torch.float64, device=train.device)
    _lib.check(lib.harp_knn_f64_prepare(train.data_ptr(), _DTYPES[train.dtype], N, _ld(train), d, W.data_ptr(),
                                        _lib.stream_ptr(train.device)), "knn_f64_prepare")
    return W


def _torch_search(train, queries, k, tn):
    """The mirror: a stable sort of the clamped expansion orders ties by training index."""
    T = train.double()
    tile = max(1, min(8192, (1 << 24) // max(1, T.shape[0])))
    ds, ix = [], []
    for a in range(0, queries.shape[0], tile):
        Q = queries[a:a + tile].double()
        D = ((Q * Q).sum(1)[:, None] + tn[None, :] - 2 * (Q @ T.t())).clamp_min(0)
        empty = D.isnan() | D.isinf()  # what never enters a list of the kernel
        dv, iv = D.masked_fill(empty, float("inf")).sort(dim=1, stable=True)
        dv, iv = dv[:, :k], iv[:, :k]
        ds.append(dv), ix.append(iv.masked_fill(torch.gather(empty, 1, iv), -1))
    return torch.cat(ds), torch.cat(ix)


def knn_search(train: torch.Tensor, queries: torch.Tensor, k: int, operand: Optional[torch.Tensor] = None,
               splits: Optional[int] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """(fp64 squared distances [M, min(k, N)] ascending, int64 training indices) of the nearest
    training rows of every query. ``operand``: what :func:`prepare` returned for ``train``.
    ``splits``: None for the launcher's choice, or the number of ranges the training rows are
    swept in."""
    _check_rows(train, "training")
    _check_rows(queries, "query")
    N, d = train.shape
    M = queries.shape[0]
    if queries.shape[1] != d or queries.device != train.device:
        raise ValueError(f"queries [M, {d}] on the device of the training rows expected (got {tuple(queries.shape)} "
                         f"on {queries.device})")
    if N < 1:
        raise ValueError("kNN needs at least one training row")
    check_k(k)
    if splits is not None and not 1 <= splits <= MAX_SPLITS:
        raise ValueError(f"splits is 1 to {MAX_SPLITS} (got {splits})")
    k = min(k, N)
    if operand is None:
        operand = prepare(train)
    native = _lib.use_native(train)
    want = _kernels().harp_knn_f64_operand_doubles(N, d) if native else N
    if operand.dtype != torch.float64 or operand.numel() != want or operand.device != train.device \
            or not operand.is_contiguous():
        raise ValueError(f"operand is not what prepare() returns for these training rows ({operand.numel()} "
                         f"doubles, expected {want})")
    if M == 0 or not native:
        if M == 0:
            return (torch.empty((0, k), dtype=torch.float64, device=train.device),
                    torch.empty((0, k), dtype=torch.int64, device=train.device))
        return _torch_search(train, queries, k, operand)
    lib = _kernels()
    stream = _lib.stream_ptr(train.device)
    if splits is None:
        splits = lib.harp_knn_f64_splits(M, N, d, k)
    outD = torch.empty((M, k), dtype=torch.float64, device=train.device)
    outI = torch.empty((M, k), dtype=torch.int32, device=train.device)
    pd, pi = outD, outI
    if splits > 1:
        pd = torch.empty((splits, M, k), dtype=torch.float64, device=train.device)
        pi = torch.empty((splits, M, k), dtype=torch.int32, device=train.device)
    _lib.check(lib.harp_knn_f64_search(queries.data_ptr(), _DTYPES[queries.dtype], M, _ld(queries), d,
                                       operand.data_ptr(), N, k, splits, pd.data_ptr(), pi.data_ptr(), stream),
               "knn_f64_search")
    if splits > 1:
        _lib.check(lib.harp_knn_f64_merge(pd.data_ptr(), pi.data_ptr(), splits, M, k, outD.data_ptr(),
                                          outI.data_ptr(), stream), "knn_f64_merge")
    return outD, outI.long()
