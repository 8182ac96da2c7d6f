"""Exact order statistics by radix select (``csrc/quantile.hip``): no sort, no copy of the
block, no row gather. A value maps to an order-preserving unsigned key; every wanted order
statistic of every column is found digit by digit, ``RADIX_BITS`` bits at a time from the top.
A digit costs one histogram pass over the block (:func:`digit_histogram`) and one small
:func:`pick`; the pass count is fixed by the dtype (bf16 2, fp32 4, fp64 8), so :func:`select`
never reads the device to decide what to do next.

HIP tensors run the kernels (mandatory: a missing library raises). CPU tensors run the torch
mirror of the same pass in this module (key by integer views, mask by prefix, ``bincount``);
it gives the same integer histograms, so it is both the gloo path and the oracle of the GPU
tests.

Distributed form: each worker histograms its own rows, one ``all_reduce(SUM)`` of the int64
histogram per pass (pass 0 also carries the row count and the NaN counts), and every worker
picks the same digit. Integer sums are exact: the result is bit-identical for any sharding.

Limits: dtypes bf16 / fp32 / fp64; at most ``MAX_TARGETS`` order statistics per sweep (the LDS
budget of the histogram kernel), more run as further sweeps of the same passes. Many-target
use (the 255 thresholds of tree binning) is out of scope. Peak extra memory is the histograms:
``2 * d * T * 256 * 8`` bytes (a pass's histogram and the all-reduce buffer) plus the [d, T]
prefixes and ranks and the [T, d] output; the block is read in place, through its row stride.

Reference hot loop: DAAL ``quantiles`` batch (ml/daal daal_quantile, QTEDaalCollectiveMapper),
which sorts every column.
"""
from __future__ import annotations

from typing import Callable, List, Optional, Sequence, Tuple, Union

import torch

from . import _lib

_P, _I, _L = _lib.c_void_p, _lib.c_int, _lib.c_long

_lib.register({
    # which
    "harp_quantile_param": [_I],
    # X, dtype, n, ldx, d, p, prefix, T, hist, nan_count, flags, stream
    "harp_quantile_hist": [_P, _I, _L, _L, _I, _I, _P, _I, _P, _P, _I, _P],
    # hist, ht, prefix, remaining, d, T, last, dtype, nan_count, out, stream
    "harp_quantile_pick": [_P, _I, _P, _P, _I, _I, _I, _I, _P, _P, _P],
})

# mirrored from csrc/quantile.hip (QUANTILE_*; checked against harp_quantile_param on first use)
RADIX_BITS = 8
BINS = 1 << RADIX_BITS
CHUNK = 4096  # rows of one histogram workgroup
MAX_TARGETS = 8  # order statistics of one sweep
COLUMN_GROUP = {torch.bfloat16: 32, torch.float32: 16, torch.float64: 16}  # columns of one workgroup

_DTYPE_ID = {torch.bfloat16: 0, torch.float32: 1, torch.float64: 2}
_INT = {torch.bfloat16: torch.int16, torch.float32: torch.int32, torch.float64: torch.int64}
_WIDTH = {torch.bfloat16: 16, torch.float32: 32, torch.float64: 64}
SHARED_DIGIT = 1  # digit_histogram flag: one add per column when a wave's matching lanes share a digit (slower as measured: profiles/quantile)

_checked = False


def passes(dtype: torch.dtype) -> int:
    """Radix passes (= all-reduces per sweep) of a dtype."""
    _check_dtype(dtype)
    return _WIDTH[dtype] // RADIX_BITS


def _check_dtype(dtype: torch.dtype) -> None:
    if dtype not in _DTYPE_ID:
        raise ValueError(f"radix select supports bf16, fp32 and fp64 (got {dtype})")


def _kernels():
    global _checked
    k = _lib.kernels()
    if not _checked:
        got = [k.harp_quantile_param(i) for i in range(6)]
        want = [RADIX_BITS, CHUNK, MAX_TARGETS] + [COLUMN_GROUP[t] for t in (torch.bfloat16, torch.float32,
                                                                             torch.float64)]
        if got != want:
            raise RuntimeError(f"ops/quantile.py mirrors {want}, csrc/quantile.hip was built with {got}")
        _checked = True
    return k


def _row_major(X: torch.Tensor) -> torch.Tensor:
    """X itself when its rows are contiguous (any row stride >= d: a column slice of a wider
    matrix is read in place), else a contiguous copy."""
    if X.dim() != 2:
        raise ValueError(f"expected a [n, d] block (got {tuple(X.shape)})")
    n, d = X.shape
    if d < 1:
        raise ValueError("expected at least one column")
    if (d > 1 and X.stride(1) != 1) or (n > 1 and X.stride(0) < d):
        return X.contiguous()
    return X


# ---------------------------------------------------------------- torch mirror
def _signed_key(X: torch.Tensor) -> torch.Tensor:
    """Signed integers of X's width in X's order: the unsigned key with its top bit flipped.
    -0.0 maps to +0.0's key."""
    bits = X.view(_INT[X.dtype])
    lim = torch.iinfo(bits.dtype)
    bits = torch.where(bits == lim.min, torch.zeros_like(bits), bits)
    return torch.where(bits < 0, bits ^ lim.max, bits)


def _ref_histogram(X: torch.Tensor, prefix: torch.Tensor, p: int) -> Tuple[torch.Tensor, Optional[torch.Tensor]]:
    n, d = X.shape
    T = prefix.shape[1]
    W = _WIDTH[X.dtype]
    sk = _signed_key(X)
    valid = ~torch.isnan(X)
    lo = W - RADIX_BITS * (p + 1)
    digit = ((sk >> lo) & (BINS - 1)).long()
    col = torch.arange(d, dtype=torch.int64) * BINS
    if p == 0:
        digit = digit ^ (BINS >> 1)  # the unsigned key's top bit
        hist = torch.bincount((digit + col)[valid], minlength=d * BINS).view(d, 1, BINS)
        return hist, (~valid).sum(0)
    hi = W - RADIX_BITS * p
    # the unsigned key's top 8p bits, as the non-negative integers the prefixes are
    top = ((sk >> hi).long() & ((1 << (RADIX_BITS * p)) - 1)) ^ (1 << (RADIX_BITS * p - 1))
    idx = digit + col
    hist = torch.empty((d, T, BINS), dtype=torch.int64)
    for t in range(T):
        m = valid & (top == prefix[:, t])
        hist[:, t] = torch.bincount(idx[m], minlength=d * BINS).view(d, BINS)
    return hist, None


def _ref_value(key: torch.Tensor, dtype: torch.dtype) -> torch.Tensor:
    """Inverse key map: unsigned keys (int64 bit patterns) -> values."""
    W = _WIDTH[dtype]
    if W == 64:
        lim = torch.iinfo(torch.int64)
        bits = torch.where(key < 0, key ^ lim.min, ~key)
    else:
        sign = 1 << (W - 1)
        bits = torch.where((key & sign) != 0, key ^ sign, ~key & (2 * sign - 1))
        bits = torch.where(bits >= sign, bits - 2 * sign, bits)  # as a signed integer of width W
    return bits.to(_INT[dtype]).view(dtype)


# ---------------------------------------------------------------- one pass
def digit_histogram(X: torch.Tensor, prefix: torch.Tensor, p: int,
                    flags: int = 0) -> Tuple[torch.Tensor, Optional[torch.Tensor]]:
    """Pass ``p`` over the local block ``X`` [n, d] (n may be 0): the int64 histogram of the next
    ``RADIX_BITS``-bit key digit of the rows whose key's top ``RADIX_BITS * p`` bits equal
    ``prefix`` [d, T] (int64), [d, T, 256]. Pass 0 has no prefix: it returns one histogram per
    column, [d, 1, 256], and the per-column NaN counts [d] (None for the later passes)."""
    _check_dtype(X.dtype)
    if not 0 <= p < passes(X.dtype):
        raise ValueError(f"pass {p} of a {X.dtype} key")
    X = _row_major(X)
    n, d = X.shape
    T = prefix.shape[1]
    if prefix.shape[0] != d or prefix.dtype != torch.int64 or not 1 <= T <= MAX_TARGETS:
        raise ValueError(f"prefix must be int64 [d, T <= {MAX_TARGETS}] (got {prefix.dtype} {tuple(prefix.shape)})")
    if not _lib.use_native(X):
        return _ref_histogram(X, prefix, p)
    k = _kernels()
    prefix = prefix.contiguous()
    hist = torch.zeros((d, 1 if p == 0 else T, BINS), dtype=torch.int64, device=X.device)
    nan = torch.zeros(d, dtype=torch.int64, device=X.device) if p == 0 else None
    ldx = X.stride(0) if n > 1 else d
    st = k.harp_quantile_hist(X.data_ptr(), _DTYPE_ID[X.dtype], n, ldx, d, p, prefix.data_ptr(), T, hist.data_ptr(),
                              _lib.ptr(nan), flags, _lib.stream_ptr(X.device))
    _lib.check(st, "quantile_hist")
    return hist, nan


def pick(hist: torch.Tensor, prefix: torch.Tensor, remaining: torch.Tensor, p: int,
         dtype: Optional[torch.dtype] = None, nan_count: Optional[torch.Tensor] = None) -> Optional[torch.Tensor]:
    """One digit of every (column, target) from the summed ``hist`` ([d, 1 or T, 256]): the first
    bin whose running count exceeds ``remaining`` [d, T], the 0-based rank inside the current
    bucket. In place: the digit is appended to ``prefix``, the counts below it leave
    ``remaining``. With ``dtype`` given, its last pass returns the values [T, d] (NaN in the
    columns with ``nan_count`` > 0); every other call returns None."""
    d, T = prefix.shape
    last = dtype is not None and p == passes(dtype) - 1
    if not 0 <= p < (passes(dtype) if dtype is not None else 8):
        raise ValueError(f"pass {p}")
    if hist.shape[0] != d or hist.shape[1] not in (1, T) or hist.shape[2] != BINS:
        raise ValueError(f"hist must be [d, 1 or T, {BINS}] (got {tuple(hist.shape)})")
    if not (prefix.is_contiguous() and remaining.is_contiguous() and remaining.shape == prefix.shape):
        raise ValueError("prefix and remaining are updated in place: contiguous [d, T] tensors")
    if not _lib.use_native(prefix):
        cum = hist.cumsum(-1)[..., :BINS - 1].expand(d, T, BINS - 1)
        digit = (cum <= remaining[..., None]).sum(-1)
        below = torch.where(digit > 0, cum.gather(2, (digit - 1).clamp_min(0)[..., None])[..., 0],
                            torch.zeros_like(remaining))
        prefix.copy_((prefix << RADIX_BITS) | digit)
        remaining.sub_(below)
        if not last:
            return None
        out = _ref_value(prefix, dtype).t().contiguous()
        if nan_count is not None:
            out[:, nan_count > 0] = float("nan")
        return out
    out = torch.empty((T, d), dtype=dtype, device=prefix.device) if last else None
    hist = hist.contiguous()
    st = _kernels().harp_quantile_pick(hist.data_ptr(), hist.shape[1], prefix.data_ptr(), remaining.data_ptr(), d, T,
                                       int(last), _DTYPE_ID[dtype] if last else 0, _lib.ptr(nan_count), _lib.ptr(out),
                                       _lib.stream_ptr(prefix.device))
    _lib.check(st, "quantile_pick")
    return out


# ---------------------------------------------------------------- select
Ranks = Union[Sequence[int], torch.Tensor, Callable[[int], Sequence[int]]]


def select(X: torch.Tensor, ranks: Ranks, comm=None) -> torch.Tensor:
    """Order statistics [len(ranks), d] of the columns of the rows of all workers, in X's dtype:
    row i is the element at global 0-based rank ``ranks[i]`` of every sorted column (an element
    of the data, never an interpolation). ``ranks`` may be a function of the global row count
    (known after pass 0's all-reduce). ``comm``: every worker passes its own rows [n_local, d]
    (an empty shard is legal) and gets the same result. A column with a NaN is NaN in every row.
    Raises ``ValueError`` when there are no rows at all."""
    _check_dtype(X.dtype)
    X = _row_major(X)
    n_local, d = X.shape
    dev = X.device
    npass = passes(X.dtype)
    dist = comm is not None and comm.world_size > 1
    n_global: Optional[int] = None if dist else n_local
    if not dist and n_local == 0:
        raise ValueError("order statistics of no rows")
    wanted: Optional[List[int]] = None
    if n_global is not None:
        wanted = _rank_list(ranks, n_global)
        if not wanted:
            return torch.empty((0, d), dtype=X.dtype, device=dev)
    rows: List[torch.Tensor] = []
    start = 0
    while wanted is None or start < len(wanted):
        T = MAX_TARGETS if wanted is None else min(MAX_TARGETS, len(wanted) - start)
        prefix = torch.zeros((d, T), dtype=torch.int64, device=dev)
        remaining = None
        nan = None
        for p in range(npass):
            hist, nan_local = digit_histogram(X, prefix, p)
            if p == 0:
                nan = nan_local
            if dist:
                if p == 0:
                    buf = torch.cat([hist.reshape(-1), nan_local,
                                     torch.tensor([n_local], dtype=torch.int64, device=dev)])
                    comm.all_reduce(buf)
                    hist, nan = buf[:d * BINS].view(d, 1, BINS), buf[d * BINS:d * BINS + d]
                    if wanted is None:  # the first sweep learns the global row count
                        n_global = int(buf[-1])
                        if n_global == 0:
                            raise ValueError("order statistics of no rows")
                        wanted = _rank_list(ranks, n_global)
                        if not wanted:
                            return torch.empty((0, d), dtype=X.dtype, device=dev)
                        T = min(MAX_TARGETS, len(wanted))
                        prefix = prefix[:, :T].contiguous()
                else:
                    comm.all_reduce(hist)
            if p == 0:
                remaining = torch.tensor(wanted[start:start + T], dtype=torch.int64, device=dev).repeat(d, 1)
            out = pick(hist, prefix, remaining, p, X.dtype, nan)
        rows.append(out)
        start += T
    return rows[0] if len(rows) == 1 else torch.cat(rows)


def _rank_list(ranks: Ranks, n: int) -> List[int]:
    if callable(ranks):
        ranks = ranks(n)
    out = [int(r) for r in (ranks.tolist() if isinstance(ranks, torch.Tensor) else ranks)]
    for r in out:
        if not 0 <= r < n:
            raise ValueError(f"rank {r} outside 0..{n - 1}")
    return out
