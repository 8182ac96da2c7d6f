"""Sparse kernel matrices (``csrc/csr_kernel.hip``), fp64: ``K = f(X Y^T)`` for two CSR
operands with a dense output.

The kernel functions of the reference's csr applications (ml/daal/.../daal_kernel_func/
{LinCSRBatch, RbfCSRBatch} in matrixMatrix mode) and the Gram matrix that
daal_svm/MultiClassCSRBatch trains on, computed from the CSR arrays: no function here forms
a dense n x d block. On a HIP device every function launches the native kernels; on CPU
tensors it runs the fp64 torch reference (``*_ref``), which is also the oracle of the GPU
tests.

Every output element is owned by one lane and adds its products in ascending column order,
so the same inputs give the same bits on every run, both paths agree bitwise, and
``kernel_block(X, X)`` is bitwise symmetric.
"""
from __future__ import annotations

from typing import Optional, Tuple

import torch

from . import _lib
from .csr_stats import _REF_CHUNK, CSROperand, to_csr_operand

_lib.register({
    "harp_csr_kernel_tile": [],
    "harp_csr_kernel_slab": [],
    # rowptr, col, val, n, out, stream
    "harp_csr_row_sqnorm": [_lib.c_void_p, _lib.c_void_p, _lib.c_void_p, _lib.c_long, _lib.c_void_p, _lib.c_void_p],
    # xrp, xcol, xval, n, i0, i1, yrp, ycol, yval, m, d, mode, p0, p1, nx, ny, path, out, ld, stream
    "harp_csr_kernel_block": [_lib.c_void_p, _lib.c_void_p, _lib.c_void_p, _lib.c_long, _lib.c_long, _lib.c_long,
                              _lib.c_void_p, _lib.c_void_p, _lib.c_void_p, _lib.c_long, _lib.c_int, _lib.c_int,
                              _lib.c_double, _lib.c_double, _lib.c_void_p, _lib.c_void_p, _lib.c_int, _lib.c_void_p,
                              _lib.c_long, _lib.c_void_p],
})

KERNEL_TILE = 64   # T: output tile edge (CSR_KERNEL_TILE in csrc/csr_kernel.hip)
KERNEL_SLAB = 32   # S: columns per slab of the slab path (CSR_KERNEL_SLAB)
KINDS = {"gram": 0, "linear": 1, "rbf": 2, "sqdist": 3}
PATHS = {"slab": 0, "merge": 1}
# Path choice: the slab path pays one barrier per (tile, slab) whatever the slab holds, the
# merge path one cursor step per (output element, stored entry of the X row) and is fast
# while the Y rows of a tile fit its LDS stage. Slab when a T-row x S-column cell of the
# sparser operand holds at least this many entries on average. Measured at n = m = 20,000,
# d = 10,000 (profiles/csr_kernel/README.md): merge wins at 10.2 entries per cell (0.5 %),
# slab at 20.5 (1 %); the constant is their geometric mean.
SLAB_MIN_CELL_ENTRIES = 14.0


def tile() -> int:
    t = int(_lib.kernels().harp_csr_kernel_tile())
    assert t == KERNEL_TILE
    return t


def slab() -> int:
    s = int(_lib.kernels().harp_csr_kernel_slab())
    assert s == KERNEL_SLAB
    return s


def kernel_path(n: int, m: int, d: int, nnz_x: int, nnz_y: int) -> str:
    """"slab" or "merge" from the shape alone: the average number of stored entries in a
    T-row x S-column cell of the sparser operand against ``SLAB_MIN_CELL_ENTRIES``."""
    if d <= 0 or n <= 0 or m <= 0:
        return "merge"
    cell = KERNEL_TILE * KERNEL_SLAB / d
    per_cell = min(nnz_x / n, nnz_y / m) * cell
    return "slab" if per_cell >= SLAB_MIN_CELL_ENTRIES else "merge"


# ------------------------------------------------------------------ row norms
def row_sqnorm_ref(A: CSROperand) -> torch.Tensor:
    out = torch.zeros(A.n, dtype=torch.float64, device=A.device)
    return out.index_add_(0, A.rows(), A.val * A.val)


def row_sqnorm(A) -> torch.Tensor:
    """``|x_i|^2`` per row (fp64 [n])."""
    A = to_csr_operand(A)
    if not _lib.use_native(A.val):
        return row_sqnorm_ref(A)
    out = torch.empty(A.n, dtype=torch.float64, device=A.device)
    _lib.check(_lib.kernels().harp_csr_row_sqnorm(A.rowptr.data_ptr(), A.col.data_ptr(), A.val.data_ptr(), A.n,
                                                  out.data_ptr(), _lib.stream_ptr(A.device)), "csr_row_sqnorm")
    return out


# ------------------------------------------------------------------ row gather
def take_rows(A, idx: torch.Tensor) -> torch.Tensor:
    """Rows ``idx`` of a sparse matrix as a CSR tensor, gathered with torch ops on ``rowptr``,
    ``col`` and ``val`` (no dense intermediate). The result carries its kernel operand."""
    A = to_csr_operand(A)
    idx = idx.reshape(-1).long().to(A.device)
    counts = A.rowptr[idx + 1] - A.rowptr[idx]
    rowptr = torch.zeros(idx.numel() + 1, dtype=torch.int64, device=A.device)
    torch.cumsum(counts, 0, out=rowptr[1:])
    total = int(rowptr[-1]) if idx.numel() else 0
    pos = (torch.repeat_interleave(A.rowptr[idx] - rowptr[:-1], counts)
           + torch.arange(total, device=A.device))
    col, val = A.col[pos], A.val[pos]
    out = torch.sparse_csr_tensor(rowptr, col.long(), val, size=(idx.numel(), A.d))
    out._harp_csr_operand = CSROperand(rowptr, col.contiguous(), val.contiguous(), idx.numel(), A.d)
    return out


# ------------------------------------------------------------------ kernel block
def _finish_ref(G, kind, k, b, sigma, nx, ny):
    """The dense-input expressions of models/kernels.py, applied to the Gram block."""
    if kind == "gram":
        return G
    if kind == "linear":
        return k * G + b
    D = (nx[:, None] + ny[None, :] - 2 * G).clamp_min(0)
    return torch.exp(-D / (2 * sigma * sigma)) if kind == "rbf" else D


def gram_block_ref(X: CSROperand, Y: CSROperand, i0: int, i1: int) -> torch.Tensor:
    """``X[i0:i1] Y^T`` in fp64: the products of a slice of X's stored entries against a
    column-sorted view of Y, one ``index_add_`` per slice (entries in row-major order, so an
    output element adds its products in ascending column order)."""
    m, dev = Y.n, X.device
    G = torch.zeros((i1 - i0, m), dtype=torch.float64, device=dev)
    a, b = int(X.rowptr[i0]), int(X.rowptr[i1])
    if b == a or Y.nnz == 0:
        return G
    order = torch.argsort(Y.col.long(), stable=True)  # Y's entries by column
    yrow, yval = Y.rows()[order], Y.val[order]
    colptr = torch.zeros(X.d + 1, dtype=torch.int64, device=dev)
    torch.cumsum(torch.bincount(Y.col.long(), minlength=X.d), 0, out=colptr[1:])
    xrow = X.rows()[a:b] - i0
    xc = X.col[a:b].long()
    cnt = colptr[xc + 1] - colptr[xc]  # products per X entry
    cum = torch.cumsum(cnt, 0)
    flat = G.view(-1)
    e0, ne = 0, b - a
    while e0 < ne:
        base = int(cum[e0 - 1]) if e0 else 0
        e1 = int(torch.searchsorted(cum, torch.tensor(base + _REF_CHUNK, device=dev), right=True))
        e1 = min(max(e1, e0 + 1), ne)
        c = cnt[e0:e1]
        tot = int(c.sum())
        if tot:
            e = torch.repeat_interleave(torch.arange(e0, e1, device=dev), c)
            first = torch.cumsum(c, 0) - c
            q = torch.arange(tot, device=dev) - torch.repeat_interleave(first, c) + colptr[xc[e]]
            flat.index_add_(0, xrow[e] * m + yrow[q], X.val[a:b][e] * yval[q])
        e0 = e1
    return G


def kernel_block_ref(X, Y, kind: str = "gram", k: float = 1.0, b: float = 0.0, sigma: float = 1.0,
                     rows: Optional[Tuple[int, int]] = None) -> torch.Tensor:
    X, Y = to_csr_operand(X), to_csr_operand(Y)
    i0, i1 = (0, X.n) if rows is None else rows
    G = gram_block_ref(X, Y, i0, i1)
    if kind in ("rbf", "sqdist"):
        return _finish_ref(G, kind, k, b, sigma, row_sqnorm_ref(X)[i0:i1], row_sqnorm_ref(Y))
    return _finish_ref(G, kind, k, b, sigma, None, None)


def _norms(A: CSROperand) -> torch.Tensor:
    nrm = getattr(A, "_sqnorm", None)
    if nrm is None:
        nrm = row_sqnorm(A)
        A._sqnorm = nrm  # cached on the operand, like CSROperand.blk
    return nrm


def kernel_block(X, Y, kind: str = "gram", k: float = 1.0, b: float = 0.0, sigma: float = 1.0,
                 rows: Optional[Tuple[int, int]] = None, out: Optional[torch.Tensor] = None,
                 path: Optional[str] = None) -> torch.Tensor:
    """The dense fp64 block ``out[i - i0, j] = f(<x_i, y_j>)`` for rows ``[i0, i1)`` of sparse
    ``X [n, d]`` against all rows of sparse ``Y [m, d]``. ``kind``: "gram" (g), "linear"
    (k g + b), "rbf" (exp(-|x - y|^2 / (2 sigma^2))) or "sqdist" (the clamped squared
    distance). ``out``: a ``[i1 - i0, m]`` fp64 view with unit column stride (rows may be
    strided); ``path``: "slab", "merge" or None (chosen by :func:`kernel_path`)."""
    X, Y = to_csr_operand(X), to_csr_operand(Y)
    if kind not in KINDS:
        raise ValueError(f"kind={kind!r}: expected one of {sorted(KINDS)}")
    if path not in (None, "slab", "merge"):
        raise ValueError(f"path={path!r}: expected 'slab', 'merge' or None")
    if X.d != Y.d:
        raise ValueError(f"operands differ in width: {X.d} and {Y.d}")
    if kind == "rbf" and not sigma > 0:
        raise ValueError("sigma must be positive")
    i0, i1 = (0, X.n) if rows is None else (int(rows[0]), int(rows[1]))
    if not 0 <= i0 <= i1 <= X.n:
        raise ValueError(f"rows={rows!r} outside [0, {X.n}]")
    m, dev = Y.n, X.device
    if Y.device != dev:
        raise ValueError("operands on different devices")
    if out is None:
        out = torch.empty((i1 - i0, m), dtype=torch.float64, device=dev)
    if (out.shape != (i1 - i0, m) or out.dtype != torch.float64 or out.device != dev
            or (m > 1 and out.stride(1) != 1) or (i1 - i0 > 1 and out.stride(0) < m)):
        raise ValueError("out must be a [i1 - i0, m] fp64 view on the operands' device with unit column stride")
    if i1 == i0 or m == 0:
        return out
    if not _lib.use_native(X.val):
        out.copy_(kernel_block_ref(X, Y, kind, k, b, sigma, (i0, i1)))
        return out
    path = path or kernel_path(i1 - i0, m, X.d, int(X.nnz * (i1 - i0) / max(X.n, 1)), Y.nnz)
    need = kind in ("rbf", "sqdist")
    nx = _norms(X) if need else None
    ny = _norms(Y) if need else None
    p0, p1 = (float(k), float(b)) if kind == "linear" else (1.0 / (2 * sigma * sigma), 0.0)
    ld = out.stride(0) if i1 - i0 > 1 else max(out.stride(0), m)
    st = _lib.kernels().harp_csr_kernel_block(
        X.rowptr.data_ptr(), X.col.data_ptr(), X.val.data_ptr(), X.n, i0, i1, Y.rowptr.data_ptr(), Y.col.data_ptr(),
        Y.val.data_ptr(), m, X.d, KINDS[kind], p0, p1, _lib.ptr(nx), _lib.ptr(ny), PATHS[path], out.data_ptr(), ld,
        _lib.stream_ptr(dev))
    _lib.check(st, "csr_kernel_block")
    return out
