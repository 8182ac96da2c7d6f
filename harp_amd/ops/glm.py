"""Sum-of-functions objectives and their solvers (``csrc/glm.hip``): the fused value + gradient pass
and the one-launch SGD / AdaGrad run.

:func:`value_grad` makes one pass over a row block ``X`` [n, d] (bf16 / fp32 / fp64, any row stride,
read in place) or over the rows an index list names (int indices, repeats and any order allowed, no
``X[idx]`` copy) and returns the unnormalised local sums ``models.optim.Objective._local`` returns:
the value, the gradient (intercept first) and the row count. :func:`run` executes every iteration of
``sgd`` or ``adagrad`` on ``MSE`` / ``LogisticLoss`` in one launch of one workgroup, with no host read.

HIP tensors run the kernels (mandatory: a missing library raises). CPU tensors run the torch
formulas of ``models/optim.py``, which are the gloo path and the oracle of the GPU tests. Nothing of
size [n, .] is allocated on the device: the extra memory of a pass is the block partials.

Limits: ``d <= MAX_D`` for the one-output objectives, ``K <= CE_MAX_K`` and ``d <= CE_MAX_D`` for
cross-entropy, a batch of at most ``SOLVER_MAX_BATCH`` rows and ``dim <= SOLVER_MAX_DIM`` for the
one-launch run.

Reference hot loops: DAAL ``optimization_solver`` mse / logistic_loss / cross_entropy_loss, sgd,
adagrad (ml/daal daal_optimization_solvers).
"""
from __future__ import annotations

from typing import Optional, Tuple

import torch

from . import _lib

_P, _I, _L, _D = _lib.c_void_p, _lib.c_int, _lib.c_long, _lib.c_double

_lib.register({
    # which
    "harp_glm_param": [_I],
    # X, dtype, n, ldx, d, y, w, icpt, kind, K, idx, m, partial, stream
    "harp_glm_pass": [_P, _I, _L, _L, _I, _P, _P, _I, _I, _I, _P, _L, _P, _P],
    # partial, nb, len, record, stream
    "harp_glm_reduce": [_P, _I, _I, _P, _P],
    # X, dtype, n, ldx, d, y, icpt, kind, method, table, iterations, batch, lr, gamma, inner, momentum, l2,
    # threshold, eps, x, niter, stream
    "harp_solver_run": [_P, _I, _L, _L, _I, _P, _I, _I, _I, _P, _I, _I, _P, _P, _I, _D, _D, _D, _D, _P, _P, _P],
})

# mirrored from csrc/glm.hip (GLM_*; checked against harp_glm_param on first use)
CHUNK = 256  # rows of a chunk of the one-output pass
GRID = 512  # its workgroups
MAX_D = 256  # widest row of the one-output objectives
CE_ROWS = 32  # rows of a cross-entropy chunk
CE_GRID = 512  # its workgroups
CE_MAX_K = 64  # most classes
CE_MAX_D = 128  # widest row of cross-entropy
SOLVER_MAX_BATCH = 64  # rows of one step of the one-launch run
SOLVER_MAX_DIM = 257  # its longest argument

KINDS = {"mse": 0, "logistic": 1, "cross_entropy": 2}
METHODS = {"sgd": 0, "adagrad": 1}
_DTYPE_ID = {torch.bfloat16: 0, torch.float32: 1, torch.float64: 2}
_checked = False


def _kernels():
    global _checked
    k = _lib.kernels()
    if not _checked:
        got = [k.harp_glm_param(i) for i in range(9)]
        want = [CHUNK, GRID, MAX_D, CE_ROWS, CE_GRID, CE_MAX_K, CE_MAX_D, SOLVER_MAX_BATCH, SOLVER_MAX_DIM]
        if got != want:
            raise RuntimeError(f"ops/glm.py mirrors {want}, csrc/glm.hip was built with {got}")
        _checked = True
    return k


def check_width(kind: str, d: int, num_classes: int = 0) -> None:
    if kind not in KINDS:
        raise ValueError(f"kind={kind!r}: expected one of {sorted(KINDS)}")
    if kind == "cross_entropy":
        if not 1 <= num_classes <= CE_MAX_K:
            raise ValueError(f"the native cross-entropy pass handles 1 to {CE_MAX_K} classes (got {num_classes})")
        if not 1 <= d <= CE_MAX_D:
            raise ValueError(f"the native cross-entropy pass handles 1 to {CE_MAX_D} features (got {d})")
    elif not 1 <= d <= MAX_D:
        raise ValueError(f"the native {kind} pass handles 1 to {MAX_D} features (got {d})")


def _check_block(X: torch.Tensor, kind: str, num_classes: int) -> torch.Tensor:
    """X itself when its rows are contiguous (any row stride >= d), else a contiguous copy."""
    if X.dim() != 2:
        raise ValueError(f"expected a [n, d] block (got {tuple(X.shape)})")
    if X.dtype not in _DTYPE_ID:
        raise ValueError(f"the native optimization engine supports bf16, fp32 and fp64 blocks (got {X.dtype})")
    n, d = X.shape
    check_width(kind, d, num_classes)
    if (d > 1 and X.stride(1) != 1) or (n > 1 and X.stride(0) < d):
        return X.contiguous()
    return X


def targets(y: torch.Tensor) -> torch.Tensor:
    """The targets as the kernels read them: fp64 [n], contiguous (y itself when it already is)."""
    y = y.reshape(-1)
    return y if y.dtype == torch.float64 and y.is_contiguous() else y.to(torch.float64).contiguous()


def _torch_objective(X, y, kind, num_classes, intercept):
    from ..models import optim as O  # the torch formulas live there: no second mirror here

    if kind == "cross_entropy":
        return O.CrossEntropyLoss(X, y, num_classes, intercept=intercept)
    return (O.MSE if kind == "mse" else O.LogisticLoss)(X, y, intercept=intercept)


def value_grad(X: torch.Tensor, y: torch.Tensor, x: torch.Tensor, kind: str, idx: Optional[torch.Tensor] = None,
               num_classes: int = 0, intercept: bool = True) -> Tuple[torch.Tensor, torch.Tensor, int]:
    """(value, gradient, rows): the sums over the rows of ``X`` (all of them, or the rows ``idx``
    names) of the per-row loss of the argument ``x`` and of its gradient, not normalised.

    ``kind``: ``"mse"`` (``(x0 + x . X_i - y_i)^2 / 2``), ``"logistic"`` (binary cross-entropy of the
    logit against ``y_i`` in {0, 1}) or ``"cross_entropy"`` (``y`` holds class ids, ``x`` is the
    flattened [K, d + 1] coefficient matrix). ``x`` is [intercept, coefficients] when ``intercept``.
    On a HIP device the sums are accumulated in fp64 whatever ``x.dtype`` is and are bitwise
    repeatable; an index outside the block adds nothing there."""
    X = _check_block(X, kind, num_classes)
    n, d = X.shape
    dim = (d + (1 if intercept else 0)) * (num_classes if kind == "cross_entropy" else 1)
    if x.numel() != dim:
        raise ValueError(f"the argument has {x.numel()} entries, the objective {dim}")
    if not _lib.use_native(X):
        return _torch_objective(X, y, kind, num_classes, intercept)._local(x, idx)
    k = _kernels()
    dev = X.device
    m = n if idx is None else idx.numel()
    if m == 0:
        return torch.zeros((), dtype=x.dtype, device=dev), torch.zeros(dim, dtype=x.dtype, device=dev), 0
    y64 = targets(y)
    if y64.numel() != n or y64.device != dev:
        raise ValueError("y must hold one target per row of X, on X's device")
    w = x.detach().to(dev, torch.float64).contiguous()
    if idx is not None:
        idx = idx.reshape(-1).to(dev, torch.int32).contiguous()
    ce = kind == "cross_entropy"
    nb = min(CE_GRID, -(-m // CE_ROWS)) if ce else min(GRID, -(-m // CHUNK))
    partial = torch.empty((nb, 1 + dim), dtype=torch.float64, device=dev)
    record = torch.empty(1 + dim, dtype=torch.float64, device=dev)
    stream = _lib.stream_ptr(dev)
    st = k.harp_glm_pass(X.data_ptr(), _DTYPE_ID[X.dtype], n, X.stride(0) if n > 1 else d, d, y64.data_ptr(),
                         w.data_ptr(), int(intercept), KINDS[kind], num_classes, _lib.ptr(idx), m,
                         partial.data_ptr(), stream)
    _lib.check(st, "glm_pass")
    st = k.harp_glm_reduce(partial.data_ptr(), nb, 1 + dim, record.data_ptr(), stream)
    _lib.check(st, "glm_reduce")
    return record[0].to(x.dtype), record[1:].to(x.dtype), m


def check_run(kind: str, d: int, intercept: bool, batch: int) -> None:
    if kind not in ("mse", "logistic"):
        raise ValueError(f"the one-launch run serves 'mse' and 'logistic' (got {kind!r})")
    check_width(kind, d)
    if d + (1 if intercept else 0) > SOLVER_MAX_DIM:
        raise ValueError(f"the one-launch run handles arguments of at most {SOLVER_MAX_DIM} entries")
    if not 1 <= batch <= SOLVER_MAX_BATCH:
        raise ValueError(f"the one-launch run handles batches of 1 to {SOLVER_MAX_BATCH} rows (got {batch})")


def run(X: torch.Tensor, y: torch.Tensor, kind: str, intercept: bool, x0: torch.Tensor, table: torch.Tensor,
        lr: torch.Tensor, gamma: Optional[torch.Tensor] = None, method: str = "sgd", inner: int = 1,
        momentum: float = 0.0, l2: float = 0.0, threshold: float = 0.0,
        eps: float = 0.0) -> Tuple[torch.Tensor, torch.Tensor]:
    """Every iteration of ``sgd`` or ``adagrad`` in one launch, on a HIP device.

    ``table`` [iterations, batch] holds the rows of every step (host or device, any int dtype; it is
    checked on the host when it lives there), ``lr`` [iterations] the learning rates and ``gamma``
    [iterations] the conservative sequence of mini-batch SGD (None: no proximal term). Returns the
    fp64 minimum and the number of iterations performed (an int32 tensor of one element, on the
    device: reading it is the caller's only synchronisation)."""
    if method not in METHODS:
        raise ValueError(f"method={method!r}: expected 'sgd' or 'adagrad'")
    if table.dim() != 2 or table.shape[0] < 1:
        raise ValueError(f"expected an [iterations, batch] index table (got {tuple(table.shape)})")
    T, batch = table.shape
    Xc = _check_block(X, kind, 0)
    n, d = Xc.shape
    check_run(kind, d, intercept, batch)
    if not _lib.use_native(Xc):
        raise ValueError("the one-launch run needs a HIP device; CPU blocks take the solvers' loops")
    if n < 1:
        raise ValueError("the one-launch run needs at least one row")
    if table.device.type == "cpu" and (int(table.min()) < -n or int(table.max()) >= n):
        raise IndexError(f"a batch index lies outside the block's {n} rows")
    if lr.numel() != T or (gamma is not None and gamma.numel() != T):
        raise ValueError("lr and gamma hold one entry per iteration")
    k = _kernels()
    dev = Xc.device
    y64 = targets(y)
    if y64.numel() != n or y64.device != dev:
        raise ValueError("y must hold one target per row of X, on X's device")
    x = x0.detach().to(dev, torch.float64).clone().contiguous()
    if x.numel() != d + (1 if intercept else 0):
        raise ValueError(f"the argument has {x.numel()} entries, the objective {d + (1 if intercept else 0)}")
    table = table.to(dev, torch.int32).contiguous()
    lr = lr.to(dev, torch.float64).contiguous()
    gamma = None if gamma is None else gamma.to(dev, torch.float64).contiguous()
    niter = torch.zeros(1, dtype=torch.int32, device=dev)
    st = k.harp_solver_run(Xc.data_ptr(), _DTYPE_ID[Xc.dtype], n, Xc.stride(0) if n > 1 else d, d, y64.data_ptr(),
                           int(intercept), KINDS[kind], METHODS[method], table.data_ptr(), T, batch, lr.data_ptr(),
                           _lib.ptr(gamma), max(1, int(inner)), float(momentum), float(l2), float(threshold),
                           float(eps), x.data_ptr(), niter.data_ptr(), _lib.stream_ptr(dev))
    _lib.check(st, "solver_run")
    return x, niter
