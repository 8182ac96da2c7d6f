"""CSR statistics (``csrc/csr_stats.hip``), fp64: sparse Gram, per-column moments, per-class
feature sums and a sparse-dense product with a fused argmax.

The step-1 partials of the reference's csr applications (ml/daal/.../daal_cov/csrdistri,
daal_mom/csrdistri, daal_pca/corcsrdistr, daal_naive/csrdistri) computed from the CSR arrays:
no function here forms a dense n x d block. On a HIP device every function launches the
native kernels; on CPU tensors it runs the fp64 torch reference (``*_ref``, ``index_add_``
over the stored entries), which is also the oracle of the GPU tests.

Sums are accumulated with fp64 atomics on the GPU, so the last bits of a result depend on
the arrival order (as in the sparse K-means step); integer-valued data is exact.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Dict, Optional

import torch

from . import _lib

_lib.register({
    "harp_csr_gram_tile": [],
    "harp_csr_mom_lds_max_d": [],
    "harp_csr_block_offsets": [_lib.c_void_p, _lib.c_void_p, _lib.c_long, _lib.c_int, _lib.c_void_p, _lib.c_void_p],
    "harp_csr_gram": [_lib.c_void_p, _lib.c_void_p, _lib.c_void_p, _lib.c_long, _lib.c_int, _lib.c_void_p, _lib.c_int,
                      _lib.c_long, _lib.c_int, _lib.c_void_p, _lib.c_void_p],
    "harp_csr_col_moments": [_lib.c_void_p, _lib.c_void_p, _lib.c_long, _lib.c_int, _lib.c_void_p, _lib.c_void_p,
                             _lib.c_void_p],
    "harp_csr_class_sums": [_lib.c_void_p, _lib.c_void_p, _lib.c_void_p, _lib.c_long, _lib.c_int, _lib.c_void_p,
                            _lib.c_int, _lib.c_void_p, _lib.c_void_p, _lib.c_void_p, _lib.c_void_p],
    "harp_csr_spmm": [_lib.c_void_p, _lib.c_void_p, _lib.c_void_p, _lib.c_long, _lib.c_void_p, _lib.c_int, _lib.c_int,
                      _lib.c_void_p, _lib.c_void_p, _lib.c_void_p, _lib.c_void_p],
})

GRAM_TILE = 96         # T of the tiled Gram path (CSR_GRAM_TILE in csrc/csr_stats.hip)
MOM_LDS_MAX_D = 1024   # widest d whose moment accumulators are privatised in LDS
# Gram path choice: direct when the estimated number of products, nnz^2 / n, times this
# constant is below the tiled path's n * npairs row visits. Measured at n = 1e6, d = 1000
# (profiles/csr_stats/README.md): the two paths tie at density 0.3 %, where visits / products = 7.3
GRAM_DIRECT_COST = 7.0
GRAM_TARGET_WORKGROUPS = 4096  # tile pairs x row splits of the tiled path (measured: profiles/csr_stats)
_REF_CHUNK = 1 << 22   # products / gathered entries per slice of the torch references


@dataclass
class CSROperand:
    rowptr: torch.Tensor  # int64 [n + 1]
    col: torch.Tensor     # int32 [nnz], strictly increasing within a row
    val: torch.Tensor     # fp64 [nnz]
    n: int
    d: int
    blk: Optional[torch.Tensor] = None  # int32 [nb + 1, n] feature-block offsets (tiled Gram), built on demand

    @property
    def nnz(self) -> int:
        return self.val.numel()

    @property
    def device(self) -> torch.device:
        return self.val.device

    def rows(self) -> torch.Tensor:
        """Row index of every stored entry (int64 [nnz])."""
        counts = self.rowptr[1:] - self.rowptr[:-1]
        return torch.repeat_interleave(torch.arange(self.n, device=self.device), counts)


def _is_sparse(X) -> bool:
    return isinstance(X, torch.Tensor) and (X.is_sparse or X.layout in (torch.sparse_csr, torch.sparse_csc))


def _sorted_rows(rowptr: torch.Tensor, col: torch.Tensor) -> bool:
    if col.numel() < 2:
        return True
    inc = col[1:] > col[:-1]
    starts = rowptr[1:-1]  # positions where a new row begins
    starts = starts[(starts > 0) & (starts < col.numel())]
    inc[starts - 1] = True
    return bool(inc.all())


def to_csr_operand(X) -> CSROperand:
    """Kernel operands of a sparse (COO or CSR) matrix, built once and cached on the tensor.
    Columns must be sorted within a row for the block offsets: CSR input that is not is
    coalesced first (which also sums duplicates)."""
    if isinstance(X, CSROperand):
        return X
    cached = getattr(X, "_harp_csr_operand", None)
    if cached is not None:
        return cached
    if X.layout == torch.sparse_csr:
        Xc = X
        if not _sorted_rows(Xc.crow_indices(), Xc.col_indices()):
            Xc = torch.sparse_coo_tensor(_coo_indices(Xc), Xc.values(), Xc.shape).coalesce().to_sparse_csr()
    else:
        Xc = X.to_sparse_coo().coalesce().to_sparse_csr()
    n, d = X.shape
    col = Xc.col_indices()
    if col.numel() and (int(col.min()) < 0 or int(col.max()) >= d):
        raise ValueError(f"column index outside [0, {d})")
    A = CSROperand(Xc.crow_indices().long().contiguous(), col.to(torch.int32).contiguous(),
                   Xc.values().double().contiguous(), n, d)
    try:
        X._harp_csr_operand = A
    except AttributeError:
        pass
    return A


def _coo_indices(Xc: torch.Tensor) -> torch.Tensor:
    rp = Xc.crow_indices()
    rows = torch.repeat_interleave(torch.arange(Xc.shape[0], device=rp.device), rp[1:] - rp[:-1])
    return torch.stack([rows, Xc.col_indices().long()])


def _native(A: CSROperand) -> bool:
    return _lib.use_native(A.val)


def block_offsets(A: CSROperand) -> torch.Tensor:
    """``blk [nb + 1, n]`` (int32): per row, the offset from its first stored entry to its first
    entry with column >= b * GRAM_TILE. Feature-block-major, so 64 lanes holding 64
    consecutive rows read one block's offsets as one contiguous load. Cached on ``A``."""
    if A.blk is None:
        nb = (A.d + GRAM_TILE - 1) // GRAM_TILE
        blk = torch.empty((nb + 1, A.n), dtype=torch.int32, device=A.device)
        lib = _lib.kernels()
        assert lib.harp_csr_gram_tile() == GRAM_TILE and lib.harp_csr_mom_lds_max_d() == MOM_LDS_MAX_D
        _lib.check(lib.harp_csr_block_offsets(A.rowptr.data_ptr(), A.col.data_ptr(), A.n, A.d, blk.data_ptr(),
                                              _lib.stream_ptr(A.device)), "csr_block_offsets")
        A.blk = blk
    return A.blk


# ------------------------------------------------------------------ Gram
def gram_path(n: int, d: int, nnz: int) -> str:
    """"tiled" or "direct" from the shape alone: the tiled path visits every row once per
    tile pair, the direct path pays a scattered global atomic per product."""
    nb = (d + GRAM_TILE - 1) // GRAM_TILE
    visits = n * (nb * (nb + 1) // 2)
    products = nnz * nnz / max(n, 1)
    return "direct" if products * GRAM_DIRECT_COST < visits else "tiled"


def gram_ref(A: CSROperand, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Upper triangle of X^T X in fp64 by expanding every row's products (col_i <= col_j) and
    one ``index_add_`` per slice of rows."""
    G = torch.zeros((A.d, A.d), dtype=torch.float64, device=A.device) if out is None else out
    if A.nnz == 0:
        return G
    flat = G.view(-1)
    counts = (A.rowptr[1:] - A.rowptr[:-1])
    cum = torch.cumsum(counts * counts, 0)
    r0 = 0
    while r0 < A.n:
        base = int(cum[r0 - 1]) if r0 else 0
        r1 = int(torch.searchsorted(cum, torch.tensor(base + _REF_CHUNK, device=cum.device), right=True))
        r1 = max(r1, r0 + 1)
        a, b = int(A.rowptr[r0]), int(A.rowptr[r1])
        if b > a:
            m = counts[r0:r1]
            per = torch.repeat_interleave(m, m)                      # row length, per stored entry
            start = torch.repeat_interleave(A.rowptr[r0:r1] - a, m)  # row start, per stored entry
            p = torch.repeat_interleave(torch.arange(b - a, device=A.device), per)
            first = torch.cumsum(per, 0) - per
            q = torch.arange(p.numel(), device=A.device) - torch.repeat_interleave(first, per) + start[p]
            cp, cq = A.col[a:b][p].long(), A.col[a:b][q].long()
            keep = cp <= cq
            flat.index_add_(0, (cp * A.d + cq)[keep], (A.val[a:b][p] * A.val[a:b][q])[keep])
        r0 = r1
    return G


def gram(A, out: Optional[torch.Tensor] = None, path: Optional[str] = None,
         rows_per_split: Optional[int] = None) -> torch.Tensor:
    """ADDS the upper triangle of X^T X (fp64) into ``out [d, d]`` (zeros when None); mirror it
    with ``ops.linalg.symmetrize_upper``. ``path``: "tiled", "direct" or None (chosen by
    :func:`gram_path`). ``rows_per_split``: rows per workgroup of the tiled path (rounded up to
    a multiple of 64; default: about ``GRAM_TARGET_WORKGROUPS`` workgroups)."""
    A = to_csr_operand(A)
    if path not in (None, "tiled", "direct"):
        raise ValueError(f"path={path!r}: expected 'tiled', 'direct' or None")
    if out is None:
        out = torch.zeros((A.d, A.d), dtype=torch.float64, device=A.device)
    assert out.shape == (A.d, A.d) and out.dtype == torch.float64 and out.is_contiguous() and out.device == A.device
    if A.n == 0 or A.nnz == 0:
        return out
    if not _native(A):
        return gram_ref(A, out)
    path = path or gram_path(A.n, A.d, A.nnz)
    lib = _lib.kernels()
    if path == "direct":
        lanes = 8 if A.nnz < 8 * A.n else 64
        st = lib.harp_csr_gram(A.rowptr.data_ptr(), A.col.data_ptr(), A.val.data_ptr(), A.n, A.d, None, 1, 0, lanes,
                               out.data_ptr(), _lib.stream_ptr(A.device))
    else:
        blk = block_offsets(A)
        nb = (A.d + GRAM_TILE - 1) // GRAM_TILE
        if rows_per_split is None:
            nsplit = max(1, GRAM_TARGET_WORKGROUPS // (nb * (nb + 1) // 2))
            rows_per_split = max(1024, -(-A.n // nsplit))  # at least one 64-row batch per wave
        rows_per_split = max(64, (int(rows_per_split) + 63) // 64 * 64)
        rows_per_split = max(rows_per_split, (-(-A.n // 65535) + 63) // 64 * 64)  # grid.y limit
        st = lib.harp_csr_gram(A.rowptr.data_ptr(), A.col.data_ptr(), A.val.data_ptr(), A.n, A.d, blk.data_ptr(), 0,
                               rows_per_split, 0, out.data_ptr(), _lib.stream_ptr(A.device))
    _lib.check(st, "csr_gram")
    return out


# ------------------------------------------------------------------ column moments
def col_moments_ref(A: CSROperand, center: Optional[torch.Tensor] = None) -> Dict[str, torch.Tensor]:
    d, dev = A.d, A.device
    c = torch.zeros(d, dtype=torch.float64, device=dev) if center is None else center.double().to(dev)
    j = A.col.long()
    v = A.val - c[j]
    z = lambda: torch.zeros(d, dtype=torch.float64, device=dev)  # noqa: E731
    inf = torch.full((d,), float("inf"), dtype=torch.float64, device=dev)
    return {"count": z().index_add_(0, j, torch.ones_like(A.val)), "sum": z().index_add_(0, j, v),
            "sumsq": z().index_add_(0, j, v * v),
            "min": inf.clone().scatter_reduce_(0, j, A.val, "amin"),
            "max": (-inf).scatter_reduce_(0, j, A.val, "amax")}


def col_moments(A, center: Optional[torch.Tensor] = None) -> Dict[str, torch.Tensor]:
    """One pass over the STORED entries, per column: ``count``, ``sum`` of (v - center),
    ``sumsq`` of (v - center)^2, ``min`` and ``max`` of v (+inf / -inf for an empty column).
    The implicit zeros are the caller's to add (:func:`with_implicit_zeros`)."""
    A = to_csr_operand(A)
    if not _native(A):
        return col_moments_ref(A, center)
    d, dev = A.d, A.device
    c = torch.zeros(d, dtype=torch.float64, device=dev) if center is None else center.double().to(dev).contiguous()
    assert c.numel() == d
    out = torch.zeros((5, d), dtype=torch.float64, device=dev)
    out[3] = float("inf")
    out[4] = -float("inf")
    _lib.check(_lib.kernels().harp_csr_col_moments(A.col.data_ptr(), A.val.data_ptr(), A.nnz, d, c.data_ptr(),
                                                   out.data_ptr(), _lib.stream_ptr(dev)), "csr_col_moments")
    return {"count": out[0], "sum": out[1], "sumsq": out[2], "min": out[3], "max": out[4]}


def with_implicit_zeros(m: Dict[str, torch.Tensor], n: int, center: Optional[torch.Tensor] = None):
    """Moments of the full columns from those of the stored entries: the n - count zeros of a
    column add (0 - c) to the sum and c^2 to the sum of squares, and 0 enters the minimum and
    maximum only where a column has an implicit zero."""
    nz = n - m["count"]
    s, ss = m["sum"], m["sumsq"]
    if center is not None:
        c = center.double().to(s.device)
        s, ss = s - nz * c, ss + nz * c * c
    zero = torch.zeros_like(s)
    has0 = nz > 0
    return {"count": m["count"], "sum": s, "sumsq": ss,
            "min": torch.where(has0, torch.minimum(m["min"], zero), m["min"]),
            "max": torch.where(has0, torch.maximum(m["max"], zero), m["max"])}


# ------------------------------------------------------------------ class sums
def class_sums_ref(A: CSROperand, y: torch.Tensor, num_classes: int):
    yl = y.reshape(-1).long().to(A.device)
    if yl.numel() and (int(yl.min()) < 0 or int(yl.max()) >= num_classes):
        raise ValueError(f"label outside [0, {num_classes})")
    sums = torch.zeros((num_classes, A.d), dtype=torch.float64, device=A.device)
    sums.view(-1).index_add_(0, yl[A.rows()] * A.d + A.col.long(), A.val)
    return sums, torch.bincount(yl, minlength=num_classes).double()


def class_sums(A, y: torch.Tensor, num_classes: int):
    """(sums [C, d], counts [C]) in fp64: ``sums[y[r]] += row r``, ``counts[y[r]] += 1``.
    A label outside [0, C) raises ``ValueError``."""
    A = to_csr_operand(A)
    assert y.numel() == A.n
    if not _native(A):
        return class_sums_ref(A, y, num_classes)
    dev = A.device
    y32 = y.reshape(-1).to(dev, torch.int32).contiguous()
    sums = torch.zeros((num_classes, A.d), dtype=torch.float64, device=dev)
    counts = torch.zeros(num_classes, dtype=torch.float64, device=dev)
    err = torch.zeros(1, dtype=torch.int32, device=dev)
    _lib.check(_lib.kernels().harp_csr_class_sums(A.rowptr.data_ptr(), A.col.data_ptr(), A.val.data_ptr(), A.n, A.d,
                                                  y32.data_ptr(), num_classes, sums.data_ptr(), counts.data_ptr(),
                                                  err.data_ptr(), _lib.stream_ptr(dev)), "csr_class_sums")
    if int(err) != 0:
        raise ValueError(f"label outside [0, {num_classes})")
    return sums, counts


# ------------------------------------------------------------------ sparse x dense
def _argmax_low(S: torch.Tensor) -> torch.Tensor:
    """Row argmax with exact ties going to the lowest column."""
    m = S.shape[1]
    idx = torch.arange(m, device=S.device).expand_as(S)
    return torch.where(S == S.max(1, keepdim=True).values, idx, torch.full_like(idx, m)).min(1).values


def spmm_ref(A: CSROperand, B: torch.Tensor, bias: Optional[torch.Tensor] = None, argmax: bool = False):
    B = B.double().to(A.device)
    m = B.shape[1]
    out = torch.zeros((A.n, m), dtype=torch.float64, device=A.device)
    rows = A.rows()
    step = max(1, _REF_CHUNK // max(m, 1))
    for a in range(0, A.nnz, step):
        sl = slice(a, a + step)
        out.index_add_(0, rows[sl], A.val[sl, None] * B[A.col[sl].long()])
    if bias is not None:
        out += bias.double().to(A.device)
    return _argmax_low(out) if argmax else out


def spmm(A, B: torch.Tensor, bias: Optional[torch.Tensor] = None, argmax: bool = False) -> torch.Tensor:
    """``X @ B + bias`` in fp64 for dense ``B [d, m]``: the scores ``[n, m]``, or with
    ``argmax=True`` only the per-row argmax (int64 [n], ties to the lowest column) -- the
    [n, m] tensor is then never written."""
    A = to_csr_operand(A)
    assert B.shape[0] == A.d
    if not _native(A):
        return spmm_ref(A, B, bias, argmax)
    dev = A.device
    m = B.shape[1]
    mp = (m + 63) // 64 * 64
    BP = torch.zeros((A.d, mp), dtype=torch.float64, device=dev)
    BP[:, :m] = B
    b = None if bias is None else bias.double().to(dev).contiguous()
    out = None if argmax else torch.empty((A.n, m), dtype=torch.float64, device=dev)
    am = torch.empty(A.n, dtype=torch.int32, device=dev) if argmax else None
    _lib.check(_lib.kernels().harp_csr_spmm(A.rowptr.data_ptr(), A.col.data_ptr(), A.val.data_ptr(), A.n,
                                            BP.data_ptr(), m, mp, _lib.ptr(b), _lib.ptr(out), _lib.ptr(am),
                                            _lib.stream_ptr(dev)), "csr_spmm")
    return am.long() if argmax else out
