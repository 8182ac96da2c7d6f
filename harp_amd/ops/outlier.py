"""Outlier detection passes (``csrc/outlier.hip``): one fused Mahalanobis pass over a row block
and the elementwise univariate rule.

:func:`mahalanobis_pass` reads the block once, in its own dtype (bf16 / fp32 / fp64) and through
its row stride, and returns everything one BACON iteration needs: per row ``dist2 = ||P (x -
c)||^2`` and ``member = dist2 < t2`` (or ``<=``); over the members their count, ``sum (x - s)`` and
``sum (x - s)(x - s)^T``; over all rows the number of mask bytes that flipped. ``P = L^-1`` is the
packed lower triangle of the whitening matrix (:func:`whiten`), or None for the identity.
:func:`model_from_stats` turns a record into the next mean and covariance.

HIP tensors run the kernels (mandatory: a missing library raises). CPU tensors run the torch
mirror of the same arithmetic in fp64, over row slices; it is the gloo path and the oracle of
the GPU tests. Nothing of size [n, d] is allocated on the device: the extra memory of a pass is
the mask (n bytes, the caller's), the optional distances (8 n bytes) and the block partials.

Distributed form: every worker passes over its own rows and the records are summed
(:func:`reduce_record`: one ``all_reduce`` per pass).

Limit: ``d <= MAX_D`` (the row lives in registers).

Reference hot loops: DAAL ``univariate_outlier_detection``, ``multivariate_outlier_detection``
and ``bacon_outlier_detection`` (ml/daal daal_outlier).
"""
from __future__ import annotations

from typing import Dict, Optional, Tuple

import torch

from . import _lib

_P, _I, _L, _D = _lib.c_void_p, _lib.c_int, _lib.c_long, _lib.c_double

_lib.register({
    # which
    "harp_outlier_param": [_I],
    # X, dtype, n, ldx, d, cs, P, identity, t2, strict, mask, dist2, stats, partial, flags, stream
    "harp_outlier_pass": [_P, _I, _L, _L, _I, _P, _P, _I, _D, _I, _P, _P, _I, _P, _I, _P],
    # partial, nb, d, record, stream
    "harp_outlier_reduce": [_P, _I, _I, _P, _P],
    # X, dtype, n, ldx, d, loc, sc, thr, W, stream
    "harp_outlier_univariate": [_P, _I, _L, _L, _I, _P, _P, _D, _P, _P],
})

# mirrored from csrc/outlier.hip (OUTLIER_*; checked against harp_outlier_param on first use)
CHUNK = 256  # rows of a chunk
GRID = 512  # workgroups of the pass
MAX_D = 64  # widest row
P_PAD = 16  # doubles of padding after the packed P
VECTOR_STATS = 1  # mahalanobis_pass flag: Gram matrix on the vector FMAs (slower as measured: profiles/outlier)
REF_ROWS = 1 << 16  # rows of one slice of the torch mirror

_DTYPE_ID = {torch.bfloat16: 0, torch.float32: 1, torch.float64: 2}
_checked = False


def _kernels():
    global _checked
    k = _lib.kernels()
    if not _checked:
        got = [k.harp_outlier_param(i) for i in range(4)]
        want = [CHUNK, GRID, MAX_D, P_PAD]
        if got != want:
            raise RuntimeError(f"ops/outlier.py mirrors {want}, csrc/outlier.hip was built with {got}")
        _checked = True
    return k


def check_width(d: int) -> None:
    if not 1 <= d <= MAX_D:
        raise ValueError(f"the native outlier engine handles 1 to {MAX_D} features (got {d})")


def _check_block(X: torch.Tensor) -> torch.Tensor:
    """X itself when its rows are contiguous (any row stride >= d), else a contiguous copy."""
    if X.dim() != 2:
        raise ValueError(f"expected a [n, d] block (got {tuple(X.shape)})")
    if X.dtype not in _DTYPE_ID:
        raise ValueError(f"the outlier passes support bf16, fp32 and fp64 (got {X.dtype})")
    n, d = X.shape
    check_width(d)
    if (d > 1 and X.stride(1) != 1) or (n > 1 and (X.stride(0) < d or X.stride(0) >= 1 << 24)):
        return X.contiguous()
    return X


def record_len(d: int) -> int:
    return 2 + d + d * (d + 1) // 2


def unpack_lower(P: torch.Tensor, d: int) -> torch.Tensor:
    """The [d, d] lower-triangular matrix of a packed triangle (row i = [P_i0 .. P_ii])."""
    M = torch.zeros((d, d), dtype=torch.float64, device=P.device)
    i = torch.tril_indices(d, d, device=P.device)
    M[i[0], i[1]] = P.double()
    return M


def whiten(cov: torch.Tensor) -> torch.Tensor:
    """Packed lower triangle of ``P = L^-1`` with ``L L^T = cov + 1e-12 I`` (the jitter of
    ``stats.mahalanobis_sq``), fp64, on cov's device: ``||P (x - c)||^2`` is the squared
    Mahalanobis distance."""
    d = cov.shape[0]
    eye = torch.eye(d, dtype=torch.float64, device=cov.device)
    L = torch.linalg.cholesky(cov.double() + 1e-12 * eye)
    Pm = torch.linalg.solve_triangular(L, eye, upper=False)
    i = torch.tril_indices(d, d, device=cov.device)
    return Pm[i[0], i[1]].contiguous()


def split_record(record: torch.Tensor, d: int) -> Dict[str, torch.Tensor]:
    """Views of a record: ``count`` and ``changed`` (int64 scalars), ``sum`` [d] and ``gram`` (the
    packed upper triangle, row by row)."""
    ints = record[:2].view(torch.int64)
    return {"count": ints[0], "changed": ints[1], "sum": record[2:2 + d], "gram": record[2 + d:]}


def reduce_record(record: torch.Tensor, comm) -> torch.Tensor:
    """Sum of the workers' records, one ``all_reduce``: the two counters travel as fp64 numbers
    (exact below 2**53) beside the fp64 sums and come back as int64."""
    if comm is None or comm.world_size == 1:
        return record
    buf = record.clone()
    buf[:2] = record[:2].view(torch.int64).double()
    comm.all_reduce(buf)
    out = buf.clone()
    out[:2] = buf[:2].round().long().view(torch.float64)
    return out


def model_from_stats(record: torch.Tensor, shift: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """(mean [d], unbiased covariance [d, d]) of the members of a record whose sums were taken
    about ``shift``: what ``torch.cov`` gives for those rows, up to rounding. On the record's
    device, no host read."""
    d = shift.numel()
    r = split_record(record, d)
    m = r["count"].double()
    s1 = r["sum"]
    iu = torch.triu_indices(d, d, device=record.device)
    S = torch.zeros((d, d), dtype=torch.float64, device=record.device)
    S[iu[0], iu[1]] = r["gram"]
    S = S + S.triu(1).t()
    mean = shift.double().to(record.device) + s1 / m
    cov = (S - torch.outer(s1, s1) / m) / (m - 1).clamp_min(1)
    return mean, cov


# ---------------------------------------------------------------- torch mirror
def reference_pass(X: torch.Tensor, center: torch.Tensor, P: Optional[torch.Tensor], t2: float, shift: torch.Tensor,
                   mask: Optional[torch.Tensor] = None, want_dist: bool = False, strict: bool = True,
                   want_stats: bool = True, bounds: bool = False) -> Dict[str, torch.Tensor]:
    """The pass in fp64 torch, over slices of ``REF_ROWS`` rows, on X's device. ``bounds``: also
    ``abs_sum`` / ``abs_gram`` (the same sums over absolute values) and ``dist2_scale`` [n] =
    ``(|P| |x - c|)^2`` summed over the rows of P, the scales of the rounding-error bounds."""
    n, d = X.shape
    dev = X.device
    c = center.double().to(dev)
    s = shift.double().to(dev)
    Pm = None if P is None else unpack_lower(P.to(dev), d)
    iu = torch.triu_indices(d, d, device=dev)
    count = changed = 0
    ssum = torch.zeros(d, dtype=torch.float64, device=dev)
    gram = torch.zeros((d, d), dtype=torch.float64, device=dev)
    asum, agram = torch.zeros_like(ssum), torch.zeros_like(gram)
    dist = torch.empty(n, dtype=torch.float64, device=dev) if want_dist else None
    scale = torch.empty(n, dtype=torch.float64, device=dev) if bounds else None
    for a in range(0, n, REF_ROWS):
        Xc = X[a:a + REF_ROWS].double()
        Y = Xc - c
        Z = Y if Pm is None else Y @ Pm.t()
        d2 = (Z * Z).sum(1)
        member = d2 < t2 if strict else d2 <= t2
        count += int(member.sum())
        if dist is not None:
            dist[a:a + REF_ROWS] = d2
        if scale is not None:
            Za = Y.abs() if Pm is None else Y.abs() @ Pm.abs().t()
            scale[a:a + REF_ROWS] = (Za * Za).sum(1)
        if mask is not None:
            old = mask[a:a + REF_ROWS]
            changed += int(((old != 0) != member).sum())
            old.copy_(member)
        if want_stats:
            U = torch.where(member[:, None], Xc - s, torch.zeros((), dtype=torch.float64, device=dev))
            ssum += U.sum(0)
            gram += U.t() @ U
            if bounds:
                asum += U.abs().sum(0)
                agram += U.abs().t() @ U.abs()
    record = torch.cat([torch.tensor([count, changed], dtype=torch.int64, device=dev).view(torch.float64), ssum,
                        gram[iu[0], iu[1]]])
    out = dict(split_record(record, d), record=record, dist2=dist)
    if bounds:
        out.update(abs_sum=asum, abs_gram=agram[iu[0], iu[1]], dist2_scale=scale)
    return out


# ---------------------------------------------------------------- the pass
def mahalanobis_pass(X: torch.Tensor, center: torch.Tensor, P: Optional[torch.Tensor], t2: float,
                     shift: torch.Tensor, mask: Optional[torch.Tensor] = None, want_dist: bool = False,
                     strict: bool = True, want_stats: bool = True, flags: int = 0) -> Dict[str, torch.Tensor]:
    """One pass over the local block ``X`` [n, d] (n may be 0).

    ``center`` [d] and ``P`` (packed lower triangle of ``L^-1``, :func:`whiten`; None = identity,
    the Euclidean distance) define ``dist2``; a row is a member when ``dist2 < t2`` (``strict``)
    or ``dist2 <= t2``. ``shift`` [d] is subtracted before the members' sums are taken (pass the
    current centre: the sums then carry no cancellation). ``mask`` (uint8 [n], optional) holds the
    previous membership and is overwritten with the new one; ``changed`` counts the bytes that
    flipped (0 without a mask). ``want_stats=False`` skips the sums (they come back as zeros).

    Returns ``count`` and ``changed`` (int64 scalars on X's device), ``sum`` [d], ``gram`` (packed
    upper triangle of the [d, d] scatter about ``shift``, row by row), ``record`` (the four in one
    fp64 tensor, counters as int64 bit patterns: the unit of :func:`reduce_record` and
    :func:`model_from_stats`) and ``dist2`` (fp64 [n], or None). The result is bitwise repeatable
    for a given shape and dtype."""
    X = _check_block(X)
    n, d = X.shape
    if mask is not None and (mask.dtype != torch.uint8 or mask.shape != (n,) or not mask.is_contiguous()
                             or mask.device != X.device):
        raise ValueError("mask must be a contiguous uint8 [n] tensor on X's device")
    if P is not None and P.numel() != d * (d + 1) // 2:
        raise ValueError(f"P must be the packed lower triangle, {d * (d + 1) // 2} values (got {P.numel()})")
    if not _lib.use_native(X):
        return reference_pass(X, center, P, t2, shift, mask, want_dist, strict, want_stats)
    k = _kernels()
    dev = X.device
    rl = record_len(d)
    dist = torch.empty(n, dtype=torch.float64, device=dev) if want_dist else None
    record = torch.zeros(rl, dtype=torch.float64, device=dev)
    if n > 0:
        cs = torch.zeros(2 * MAX_D, dtype=torch.float64, device=dev)
        cs[:d] = center.to(dev)
        cs[MAX_D:MAX_D + d] = shift.to(dev)
        Pp = None
        if P is not None:
            Pp = torch.zeros(MAX_D * (MAX_D + 1) // 2 + P_PAD, dtype=torch.float64, device=dev)
            Pp[:P.numel()] = P.to(dev)
        nb = min(GRID, -(-n // CHUNK))
        partial = torch.empty((nb, rl), dtype=torch.float64, device=dev)
        ldx = X.stride(0) if n > 1 else d
        stream = _lib.stream_ptr(dev)
        st = k.harp_outlier_pass(X.data_ptr(), _DTYPE_ID[X.dtype], n, ldx, d, cs.data_ptr(), _lib.ptr(Pp),
                                 int(P is None), float(t2), int(strict), _lib.ptr(mask), _lib.ptr(dist),
                                 int(want_stats), partial.data_ptr(), flags, stream)
        _lib.check(st, "outlier_pass")
        st = k.harp_outlier_reduce(partial.data_ptr(), nb, d, record.data_ptr(), stream)
        _lib.check(st, "outlier_reduce")
    return dict(split_record(record, d), record=record, dist2=dist)


def univariate(X: torch.Tensor, loc: torch.Tensor, scatter: torch.Tensor, threshold: float) -> torch.Tensor:
    """Weights [n, d] in X's dtype: ``|(double)x - loc_j| / max(scatter_j, 1e-300) <= threshold``
    (1 = inlier). One pass, no fp64 copy of X; equal to the torch expression on every element."""
    if X.dim() != 2 or X.dtype not in _DTYPE_ID:
        raise ValueError(f"expected a bf16 / fp32 / fp64 [n, d] block (got {X.dtype} {tuple(X.shape)})")
    n, d = X.shape
    if not _lib.use_native(X):
        out = torch.empty((n, d), dtype=X.dtype)
        sc = scatter.double().clamp_min(1e-300)
        for a in range(0, n, REF_ROWS):
            out[a:a + REF_ROWS] = (((X[a:a + REF_ROWS].double() - loc.double()) / sc).abs() <= threshold).to(X.dtype)
        return out
    if d < 1:
        raise ValueError("expected at least one column")
    if (d > 1 and X.stride(1) != 1) or (n > 1 and X.stride(0) < d):
        X = X.contiguous()
    out = torch.empty((n, d), dtype=X.dtype, device=X.device)
    loc = loc.double().to(X.device).contiguous()
    sc = scatter.double().to(X.device).contiguous()
    st = _kernels().harp_outlier_univariate(X.data_ptr(), _DTYPE_ID[X.dtype], n, X.stride(0) if n > 1 else d, d,
                                            loc.data_ptr(), sc.data_ptr(), float(threshold), out.data_ptr(),
                                            _lib.stream_ptr(X.device))
    _lib.check(st, "outlier_univariate")
    return out
