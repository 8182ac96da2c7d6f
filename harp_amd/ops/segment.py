"""Label bucketing (counting sort) and per-bucket row sums on the GPU.

``bucket_labels(labels, K)`` -> (perm, start): indices grouped by label, bucket offsets.
``bucket_rowsum(X, perm, start, out)``: out[k] = sum of bf16 rows X[perm[start[k]:start[k+1]]].
``bucket_labels_spans(labels, K, span)``: the same sort span by span (buckets ``span * K + label``).
See csrc/segsum.hip for why this beats float atomics on gfx950.
"""
from __future__ import annotations

import ctypes
import os
from typing import Dict, Tuple

import torch

from . import _lib

_lib.register({
    "harp_bucket_chunk": [_lib.c_long],
    "harp_bucket_workspace_ints": [_lib.c_long, _lib.c_int],
    "harp_bucket_labels": [_lib.c_void_p, _lib.c_long, _lib.c_int, _lib.c_void_p, _lib.c_void_p, _lib.c_void_p,
                           _lib.c_void_p],
    "harp_bucket_rowsum_bf16": [_lib.c_void_p, _lib.c_int, _lib.c_long, _lib.c_void_p, _lib.c_void_p, _lib.c_int,
                                _lib.c_long, _lib.c_void_p, _lib.c_int, _lib.c_void_p],
    # X, ldx, Cm2, dp, perm, start, NG, nspans, n, rowof, sums, ld, stream
    "harp_kmeans_resolve_rowsum": [_lib.c_void_p, _lib.c_long, _lib.c_void_p, _lib.c_int, _lib.c_void_p,
                                   _lib.c_void_p, _lib.c_int, _lib.c_int, _lib.c_long, _lib.c_void_p, _lib.c_void_p,
                                   _lib.c_int, _lib.c_void_p],
})
_WS: Dict[Tuple, torch.Tensor] = {}
_WS_SPANS: Dict[Tuple, torch.Tensor] = {}  # (device, stream) -> the span-ordered sort's workspace


def _lib_ret_long(fn):
    fn.restype = ctypes.c_long
    return fn


def bucket_labels(labels: torch.Tensor, K: int) -> Tuple[torch.Tensor, torch.Tensor]:
    n = labels.numel()
    if not _lib.use_native(labels):
        order = torch.argsort(labels.long(), stable=True)
        counts = torch.bincount(labels.long(), minlength=K)
        start = torch.zeros(K + 1, dtype=torch.int64)
        start[1:] = torch.cumsum(counts, 0)
        return order.to(torch.int32), start.to(torch.int32)
    lib = _lib.kernels()
    _lib_ret_long(lib.harp_bucket_workspace_ints)
    need = lib.harp_bucket_workspace_ints(n, K)
    stream = torch.cuda.current_stream(labels.device).cuda_stream
    key = (labels.device, n, K, stream)
    ws = _WS.get(key)
    if ws is None:
        # a larger workspace already alive on this stream serves a smaller call
        ws = next((w for k, w in _WS.items() if k[0] == labels.device and k[3] == stream and w.numel() >= need),
                  None)
    if ws is None:
        for k in [k for k in _WS if k[3] == stream]:
            del _WS[k]  # one workspace alive per stream (allocated and reused on that stream)
        ws = torch.empty(need, dtype=torch.int32, device=labels.device)
        _WS[key] = ws
    so, po = ctypes.c_long(0), ctypes.c_long(0)
    st = lib.harp_bucket_labels(labels.data_ptr(), n, K, ws.data_ptr(), ctypes.byref(so), ctypes.byref(po),
                                _lib.stream_ptr(labels.device))
    _lib.check(st, "bucket_labels")
    return ws[po.value:po.value + n], ws[so.value:so.value + K + 1]


def bucket_labels_spans(labels: torch.Tensor, K: int, span: int, want_rank: bool = False):
    """Counting sort of ``labels`` (values in [0, K)) span by span: ``span`` (a power of two >=
    1024) consecutive points form a span, and bucket ``s * K + g`` holds the points of span ``s``
    with label ``g``. Returns (perm, start): ``perm`` [n] the point indices in bucket order,
    ``start`` [nspans * K + 1] the bucket offsets (monotone, ``start[-1] == n``). With
    ``want_rank`` also (rank, rowof): ``rank`` [n] int32 with ``rank[perm[j]] == j`` and an
    uninitialised uint8 [n] for the resolve pass, both inside the same cached workspace. One
    launch of each of the five bucketing kernels whatever the number of spans."""
    n = labels.numel()
    nspans = (n + span - 1) // span
    if not _lib.use_native(labels):
        key = torch.arange(n, dtype=torch.int64) // span * K + labels.long()
        order = torch.argsort(key, stable=True)
        start = torch.zeros(nspans * K + 1, dtype=torch.int64)
        start[1:] = torch.cumsum(torch.bincount(key, minlength=nspans * K), 0)
        out = (order.to(torch.int32), start.to(torch.int32))
        if want_rank:
            rank = torch.empty(n, dtype=torch.int32)
            rank[order] = torch.arange(n, dtype=torch.int32)
            out += (rank, torch.empty(n, dtype=torch.uint8))
        return out
    assert labels.dtype == torch.int32 and labels.is_contiguous()
    lib = _lib.kernels()
    need = _lib_ret_long(lib.harp_bucket_spans_workspace_ints)(n, K, span)
    if need <= 0:
        raise ValueError(f"bucket_labels_spans: n = {n}, K = {K}, span = {span} (a power of two >= 1024, n < 2^31)")
    base = (need + 3) // 4 * 4  # rank and rowof behind the sort's own arrays, 16-byte aligned
    total = base + (n + (n + 3) // 4 if want_rank else 0)
    stream = torch.cuda.current_stream(labels.device).cuda_stream
    key = (labels.device, stream)
    ws = _WS_SPANS.get(key)
    if ws is None or ws.numel() < total:
        ws = _WS_SPANS[key] = torch.empty(total, dtype=torch.int32, device=labels.device)
    rank = ws[base:base + n] if want_rank else None
    so, po = ctypes.c_long(0), ctypes.c_long(0)
    st = lib.harp_bucket_labels_spans(labels.data_ptr(), n, K, span, ws.data_ptr(), ctypes.byref(so), ctypes.byref(po),
                                      _lib.ptr(rank), _lib.stream_ptr(labels.device))
    _lib.check(st, "bucket_labels_spans")
    out = (ws[po.value:po.value + n], ws[so.value:so.value + nspans * K + 1])
    if want_rank:
        out += (rank, ws[base + n:total].view(torch.uint8)[:n])
    return out


# 256: the per-slice form before round 4. The kernel takes multiples of 8 in [8, 1024]
SUM_SLICE = min(1024, max(8, int(os.environ.get("HARP_ROWSUM_SLICE", "1024")) // 8 * 8))


def bucket_rowsum(X: torch.Tensor, perm: torch.Tensor, start: torch.Tensor, out: torch.Tensor) -> torch.Tensor:
    """out[k] += sum of the bucket's rows (zero ``out`` first for a plain sum)."""
    K = start.numel() - 1
    if not _lib.use_native(X):
        idx = torch.repeat_interleave(torch.arange(K), (start[1:] - start[:-1]).long())
        out[:K, : X.shape[1]].index_add_(0, idx, X[perm.long()].float())
        return out
    assert X.dtype == torch.bfloat16 and X.stride(1) == 1 and out.dtype == torch.float32 and out.is_contiguous()
    # the kernel sums rows of up to SUM_SLICE columns in one pass (one wave per slot past 256
    # columns); wider rows go as slices
    for c0 in range(0, X.shape[1], SUM_SLICE):
        w = min(SUM_SLICE, X.shape[1] - c0)
        st = _lib.kernels().harp_bucket_rowsum_bf16(X[:, c0:].data_ptr(), w, X.stride(0), perm.data_ptr(),
                                                    start.data_ptr(), K, perm.numel(), out[:, c0:].data_ptr(),
                                                    out.stride(0), _lib.stream_ptr(X.device))
        _lib.check(st, "bucket_rowsum")
    return out


def resolve_rowsum(X: torch.Tensor, Cm2: torch.Tensor, perm: torch.Tensor, start: torch.Tensor,
                   rowof: torch.Tensor, out: torch.Tensor, NG: int | None = None) -> torch.Tensor:
    """Second half of the keyless K-means assign (csrc/kmeans_resolve.hip): ``perm`` / ``start``
    bucket the points by (span, winning 32-row centroid group), ``NG`` groups per span (default:
    one span, ``start.numel() - 1`` groups); one launch over the sorted rows writes the argmin row
    inside the group of point ``perm[j]`` to ``rowof[j]`` (uint8, sorted order) and adds every row
    into ``out[32 * group + row]`` (zero ``out`` first for a plain sum). :func:`finish_labels`
    then completes the labels. GPU only, rows of at most 128 columns."""
    NG = start.numel() - 1 if NG is None else NG
    nspans = (start.numel() - 1) // NG
    dp = X.shape[1]
    assert X.dtype == torch.bfloat16 and X.stride(1) == 1 and out.dtype == torch.float32 and out.is_contiguous()
    assert Cm2.dtype == torch.bfloat16 and Cm2.is_contiguous() and Cm2.shape[1] == dp and Cm2.shape[0] >= 32 * NG
    assert out.shape[0] >= 32 * NG and rowof.dtype == torch.uint8 and rowof.is_contiguous()
    assert rowof.numel() == perm.numel() == X.shape[0] and start.numel() == nspans * NG + 1
    st = _lib.kernels().harp_kmeans_resolve_rowsum(X.data_ptr(), X.stride(0), Cm2.data_ptr(), dp, perm.data_ptr(),
                                                   start.data_ptr(), NG, nspans, perm.numel(), rowof.data_ptr(),
                                                   out.data_ptr(), out.stride(0), _lib.stream_ptr(X.device))
    _lib.check(st, "kmeans_resolve_rowsum")
    return out


def finish_labels(labels: torch.Tensor, rank: torch.Tensor, rowof: torch.Tensor) -> torch.Tensor:
    """``labels[p] = 32 * labels[p] + rowof[rank[p]]`` in place: the keyless sweep's group ids become
    final labels (``rank`` from :func:`bucket_labels_spans`, ``rowof`` from :func:`resolve_rowsum`)."""
    assert labels.dtype == rank.dtype == torch.int32 and rowof.dtype == torch.uint8
    assert labels.is_contiguous() and rank.is_contiguous() and rowof.is_contiguous()
    assert labels.numel() == rank.numel() == rowof.numel()
    st = _lib.kernels().harp_kmeans_finish_labels(labels.data_ptr(), rank.data_ptr(), rowof.data_ptr(),
                                                  labels.numel(), _lib.stream_ptr(labels.device))
    _lib.check(st, "kmeans_finish_labels")
    return labels
