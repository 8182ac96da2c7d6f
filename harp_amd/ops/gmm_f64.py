"""EM for Gaussian mixtures in fp64 (``csrc/gmm_f64.hip``): the E-step and the sufficient statistics
on the fp64 matrix cores without a responsibility matrix. Rows (bf16, fp32 or fp64, unit column
stride, any row stride) are read in place; the only per-row buffers are ``lse [n]`` and, for
prediction, the labels. Results are bitwise repeatable.

* :func:`prepare`: the components (weights, means, covariances) as the kernels' operand:
  ``P_k = L_k^-1`` from the K Cholesky factors (torch, on the device), ``c_k = P_k mu_k`` and
  ``b_k = log w_k - 0.5 (log|Sigma_k| + d log 2 pi)``.
* :func:`estep_stats`: one EM iteration's ``(N_k [K], S1 [K, d], S2, sum of the rows' log-
  likelihood)``; S2 is ``[K, d, d]`` for full and ``[K, d]`` for diagonal covariances. The rows
  are swept in ``splits`` interleaved ranges by separate workgroups (the launcher's choice fills
  the chip when there are few components) and the ranges' records added in split order.
* :func:`predict`: the arg-max component of every row, ties to the lowest, a NaN never wins.

Diagonal covariances go through the same kernels with a diagonal P, and their second moments are
the diagonal of the Gram: correct, not tuned (the off-diagonal products are computed and dropped).

HIP tensors run the kernels (mandatory: a missing library raises). CPU tensors run the torch
mirror ``log p = b - 0.5 |x P^T - c|^2`` over row tiles; that is the gloo path.

Limits: ``1 <= d <= MAX_D``, ``1 <= K <= MAX_K``, fewer than 2^31 rows. Reference: DAAL em_gmm
(ml/daal daal_em/BatchDense).
"""
from __future__ import annotations

import math
from typing import Optional, Tuple

import torch

from . import _lib

_lib.register({
    "harp_gmm_f64_max_d": [],
    "harp_gmm_f64_max_k": [],
    "harp_gmm_f64_param": [_lib.c_int, _lib.c_int],
    # P, c, b, K, d, op, stream
    "harp_gmm_f64_prepare": [_lib.c_void_p, _lib.c_void_p, _lib.c_void_p, _lib.c_int, _lib.c_int, _lib.c_void_p,
                             _lib.c_void_p],
    "harp_gmm_f64_lse_grid": [_lib.c_long],
    # X, dtype, n, ldx, d, op, K, lse, llpart, label, stream
    "harp_gmm_f64_lse": [_lib.c_void_p, _lib.c_int, _lib.c_long, _lib.c_long, _lib.c_int, _lib.c_void_p, _lib.c_int,
                         _lib.c_void_p, _lib.c_void_p, _lib.c_void_p, _lib.c_void_p],
    "harp_gmm_f64_splits": [_lib.c_long, _lib.c_int, _lib.c_int],
    # X, dtype, n, ldx, d, op, K, lse, splits, rec, stream
    "harp_gmm_f64_stats": [_lib.c_void_p, _lib.c_int, _lib.c_long, _lib.c_long, _lib.c_int, _lib.c_void_p, _lib.c_int,
                           _lib.c_void_p, _lib.c_int, _lib.c_void_p, _lib.c_void_p],
    # rec, splits, K, d, llpart, nll, N, S1, S2, ll, stream
    "harp_gmm_f64_reduce": [_lib.c_void_p, _lib.c_int, _lib.c_int, _lib.c_int, _lib.c_void_p, _lib.c_int,
                            _lib.c_void_p, _lib.c_void_p, _lib.c_void_p, _lib.c_void_p, _lib.c_void_p],
})

MAX_D = 64         # mirrored from csrc/gmm_f64.hip (GF_MAX_D; checked on first use)
MAX_K = 1024       # GF_MAX_K
MAX_SPLITS = 1024  # GF_MAX_SPLITS
CHUNK = 64         # GF_CH: rows of a staged chunk
_DTYPES = {torch.bfloat16: 0, torch.float32: 1, torch.float64: 2}
_checked = False


def group(d: int) -> int:
    """Components of one statistics workgroup at width d."""
    return 4 if d > 48 else 8


def _kernels():
    global _checked
    lib = _lib.kernels()
    if not _checked:
        if (lib.harp_gmm_f64_max_d(), lib.harp_gmm_f64_max_k()) != (MAX_D, MAX_K):
            raise RuntimeError(f"ops/gmm_f64.py mirrors MAX_D = {MAX_D} and MAX_K = {MAX_K}, csrc/gmm_f64.hip was "
                               f"built with {lib.harp_gmm_f64_max_d()} and {lib.harp_gmm_f64_max_k()}")
        for d in range(1, MAX_D + 1):
            if (lib.harp_gmm_f64_param(2, d), lib.harp_gmm_f64_param(3, d)) != (CHUNK, group(d)):
                raise RuntimeError(f"ops/gmm_f64.py and csrc/gmm_f64.hip disagree on the chunk or the component "
                                   f"group at width {d}")
        _checked = True
    return lib


def check_shape(d: int, K: int, n: int = 0) -> None:
    if not 1 <= d <= MAX_D:
        raise ValueError(f"the native fp64 EM handles 1 to {MAX_D} columns (got {d}): use engine=\"auto\"")
    if not 1 <= K <= MAX_K:
        raise ValueError(f"the native fp64 EM handles 1 to {MAX_K} components (got {K}): use engine=\"auto\"")
    if n >= 2 ** 31:
        raise ValueError(f"the native fp64 EM handles fewer than 2^31 rows (got {n}): use engine=\"auto\"")


def rows(X: torch.Tensor) -> torch.Tensor:
    """X as the kernels read it: dense bf16 / fp32 / fp64 rows of unit column stride and a row
    stride >= d. Another layout is copied once (in its own dtype); another dtype is an error."""
    if X.dim() != 2 or X.layout != torch.strided:
        raise ValueError(f"the native fp64 EM reads dense rows [n, d] (got {X.layout}, {tuple(X.shape)}): "
                         "use engine=\"auto\"")
    if X.dtype not in _DTYPES:
        raise ValueError(f"the native fp64 EM reads bf16, fp32 or fp64 rows (got {X.dtype}): use engine=\"auto\"")
    if X.stride(1) != 1 or (X.shape[0] > 1 and X.stride(0) < X.shape[1]):
        return X.contiguous()
    return X


def _ld(X: torch.Tensor) -> int:
    return X.stride(0) if X.shape[0] > 1 else X.shape[1]


def whiten(w: torch.Tensor, mu: torch.Tensor, cov: torch.Tensor, covariance: str):
    """(P [K, d, d] lower triangular, c [K, d], b [K]) of the components, fp64 on mu's device."""
    K, d = mu.shape
    if covariance == "full":
        L = torch.linalg.cholesky(cov)
        eye = torch.eye(d, dtype=torch.float64, device=mu.device).expand(K, d, d)
        P = torch.linalg.solve_triangular(L, eye, upper=False)
        logdet = 2 * torch.log(torch.diagonal(L, dim1=1, dim2=2)).sum(1)
    else:
        P = torch.diag_embed(cov.rsqrt())
        logdet = torch.log(cov).sum(1)
    c = torch.einsum("kij,kj->ki", P, mu)
    b = torch.log(w) - 0.5 * (logdet + d * math.log(2 * math.pi))
    return P.contiguous(), c.contiguous(), b.contiguous()


def prepare(w: torch.Tensor, mu: torch.Tensor, cov: torch.Tensor, covariance: str = "full"):
    """The components as the kernels read them: the MFMA operand [K, operand doubles] on a HIP
    device, the tuple (P, c, b) on the CPU."""
    K, d = mu.shape
    check_shape(d, K)
    P, c, b = whiten(w.double(), mu.double(), cov.double(), covariance)
    if not _lib.use_native(mu):
        return P, c, b
    lib = _kernels()
    op = torch.empty((K, lib.harp_gmm_f64_param(0, d)), dtype=torch.float64, device=mu.device)
    _lib.check(lib.harp_gmm_f64_prepare(P.data_ptr(), c.data_ptr(), b.data_ptr(), K, d, op.data_ptr(),
                                        _lib.stream_ptr(mu.device)), "gmm_f64_prepare")
    return op


def _logp_tiles(X: torch.Tensor, P, c, b, tile: int = 16384):
    """The mirror: log p [rows of a tile, K] for one row tile after the other."""
    for a in range(0, X.shape[0], tile):
        Xt = X[a:a + tile].double()
        z = torch.einsum("kij,nj->nki", P, Xt) - c[None]
        yield Xt, b[None, :] - 0.5 * (z * z).sum(2)


def _lse(X, op, K, want_labels: bool):
    lib = _kernels()
    n, d = X.shape
    dev = X.device
    lse = torch.empty(n, dtype=torch.float64, device=dev)
    llpart = torch.empty(lib.harp_gmm_f64_lse_grid(n), dtype=torch.float64, device=dev)
    label = torch.empty(n, dtype=torch.int32, device=dev) if want_labels else None
    _lib.check(lib.harp_gmm_f64_lse(X.data_ptr(), _DTYPES[X.dtype], n, _ld(X), d, op.data_ptr(), K, lse.data_ptr(),
                                    llpart.data_ptr(), _lib.ptr(label), _lib.stream_ptr(dev)), "gmm_f64_lse")
    return lse, llpart, label


def estep_stats(X: torch.Tensor, w: torch.Tensor, mu: torch.Tensor, cov: torch.Tensor, covariance: str = "full",
                splits: Optional[int] = None) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    """(N_k [K], S1 = sum r x [K, d], S2 = sum r x x^T [K, d, d] (full) or sum r x^2 [K, d] (diag),
    sum_n log sum_k w_k N(x_n | k)) of the rows X [n, d] (as :func:`rows` returns them).
    ``splits``: None for the launcher's choice, or the number of row ranges of the statistics."""
    n, d = X.shape
    K = mu.shape[0]
    check_shape(d, K, n)
    if splits is not None and not 1 <= splits <= MAX_SPLITS:
        raise ValueError(f"splits is 1 to {MAX_SPLITS} (got {splits})")
    dev = X.device
    N = torch.zeros(K, dtype=torch.float64, device=dev)
    S1 = torch.zeros((K, d), dtype=torch.float64, device=dev)
    S2 = torch.zeros((K, d, d), dtype=torch.float64, device=dev)
    ll = torch.zeros(1, dtype=torch.float64, device=dev)
    if n > 0 and not _lib.use_native(X):
        P, c, b = prepare(w, mu, cov, covariance)
        for Xt, logp in _logp_tiles(X, P, c, b):
            lse = torch.logsumexp(logp, 1)
            R = torch.exp(logp - lse[:, None])
            ll += lse.sum()
            N += R.sum(0)
            S1 += R.t() @ Xt
            S2 += torch.einsum("nk,ni,nj->kij", R, Xt, Xt)
    elif n > 0:
        lib = _kernels()
        op = prepare(w, mu, cov, covariance)
        stream = _lib.stream_ptr(dev)
        lse, llpart, _ = _lse(X, op, K, False)
        if splits is None:
            splits = lib.harp_gmm_f64_splits(n, d, K)
        rec = torch.empty((splits, K, lib.harp_gmm_f64_param(1, d)), dtype=torch.float64, device=dev)
        _lib.check(lib.harp_gmm_f64_stats(X.data_ptr(), _DTYPES[X.dtype], n, _ld(X), d, op.data_ptr(), K,
                                          lse.data_ptr(), splits, rec.data_ptr(), stream), "gmm_f64_stats")
        _lib.check(lib.harp_gmm_f64_reduce(rec.data_ptr(), splits, K, d, llpart.data_ptr(), llpart.numel(),
                                           N.data_ptr(), S1.data_ptr(), S2.data_ptr(), ll.data_ptr(), stream),
                   "gmm_f64_reduce")
    if covariance != "full":
        S2 = torch.diagonal(S2, dim1=1, dim2=2).contiguous()
    return N, S1, S2, ll[0]


def predict(X: torch.Tensor, w: torch.Tensor, mu: torch.Tensor, cov: torch.Tensor,
            covariance: str = "full") -> torch.Tensor:
    """int64 labels [n]: the component of the largest log p(x, k), ties to the lowest."""
    n, d = X.shape
    K = mu.shape[0]
    check_shape(d, K, n)
    if n == 0:
        return torch.empty(0, dtype=torch.int64, device=X.device)
    if not _lib.use_native(X):
        P, c, b = prepare(w, mu, cov, covariance)
        # a NaN never wins: it is ranked below every number (all NaN: component 0)
        return torch.cat([torch.nan_to_num(logp, nan=-math.inf).argmax(1) for _, logp in _logp_tiles(X, P, c, b)])
    return _lse(X, prepare(w, mu, cov, covariance), K, True)[2].long()


def column_moments(X: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """(sum x, sum x^2) per column in fp64 without an fp64 copy of the rows (``ops.xprod``'s
    moments pass with a zero shift)."""
    from . import xprod as XP

    m = XP.col_moments(X, shift=torch.zeros(X.shape[1], dtype=torch.float64, device=X.device))
    return m["sum"], m["sumsq"]
