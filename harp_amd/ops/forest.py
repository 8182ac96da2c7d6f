"""Level-wise decision-forest engine (``csrc/forest.hip``): binning, counter-based bootstrap,
hashed feature subsets, per-level histograms, split search, row routing and packed-forest
inference. :func:`grow` trains all trees of a batch together, one hist -> split -> route pass
per level, with one device->host read per level (the number of nodes that split).

HIP tensors run the kernels (mandatory: a missing library raises). CPU tensors run the torch
mirror of the same algorithm in this module; it reproduces the kernels bit for bit (the
bootstrap, the feature subsets, the integer histograms and every gain: the gain arithmetic
sums classes in index order and takes log2 from + - * / only), so it is both the gloo path
and the oracle of the GPU tests.

Limits (outside them the launchers return status 1 / 3 and the wrappers raise):
``n_bins <= 256`` (bin ids are uint8), classes ``<= 32`` (``n_bins * classes * 8`` bytes is the
LDS slice of one (node, feature)), ``15 * n_global < 2**32`` (uint32 count cells with
multiplicities capped at 15), and ``trees_per_batch * n < 2**31`` (int32 row order).

Statistics kinds: ``count`` — class label + integer multiplicity, integer cells, exact and
independent of order (int32 storage on the GPU read as uint32, int64 in the mirror);
``real`` — fp64 cells of ``stats[n, C] * multiplicity`` (classification with real weights,
C = classes; regression, C = 3: w, w*y, w*y^2).

Reference hot loops: DAAL ``decision_tree`` / ``decision_forest`` training and prediction
(ml/daal daal_dtree, daal_dforest) and the contrib random forests.
"""
from __future__ import annotations

from typing import Callable, Dict, List, Optional, Tuple

import torch

from . import _lib

_P, _I, _L, _D, _U = _lib.c_void_p, _lib.c_int, _lib.c_long, _lib.c_double, _lib.ctypes.c_uint

_lib.register({
    # X, is64, n, d, th, nth, Xb, dpad, stream
    "harp_forest_bin": [_P, _I, _L, _I, _P, _I, _P, _I, _P],
    # seed, tree0, T, row0, n, table, w, stream
    "harp_forest_bootstrap": [_U, _I, _I, _L, _L, _P, _P, _P],
    # seed, fr_tree, fr_node, M, d, k, mask, stream
    "harp_forest_feature_subset": [_U, _P, _P, _I, _I, _I, _P, _P],
    # Xb, dpad, order, start, cnt, fr_tree, chunk_off, M, max_chunks, mult, n, y, stats, d, B, C, kind, H, stream
    "harp_forest_hist": [_P, _I, _P, _P, _P, _P, _P, _I, _I, _P, _L, _P, _P, _I, _I, _I, _I, _P, _P],
    # H, kind, M, d, B, C, task, min_leaf, mask, cand_gain, cand_bin, stream
    "harp_forest_split_feature": [_P, _I, _I, _I, _I, _I, _I, _D, _P, _P, _P, _P],
    # H, kind, M, d, B, C, cand_gain, cand_bin, out_f, out_bin, out_gain, do_split, L, R, T, stream
    "harp_forest_split_node": [_P, _I, _I, _I, _I, _I, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P],
    # Xb, dpad, order, start, cnt, chunk_off, M, max_chunks, do_split, sf, sbin, nleft, stream
    "harp_forest_route_count": [_P, _I, _P, _P, _P, _P, _I, _I, _P, _P, _P, _P, _P],
    # Xb, dpad, order, start, cnt, chunk_off, M, max_chunks, do_split, sf, sbin, nleft, child_start, cursor,
    # new_order, new_len, stream
    "harp_forest_route_scatter": [_P, _I, _P, _P, _P, _P, _I, _I, _P, _P, _P, _P, _P, _P, _P, _L, _P],
    # X, is64, n, d, feat, thr, left, value, off, ntrees, C, max_steps, out, leaf, stream
    "harp_forest_predict": [_P, _I, _L, _I, _P, _P, _P, _P, _P, _I, _I, _I, _P, _P, _P],
})

MAX_BINS = 256
MAX_CLASSES = 32
MAX_MULT = 15
CHUNK = 2048  # rows per histogram / route workgroup (FOREST_CHUNK in csrc/forest.hip)
HIST_BUDGET_BYTES = 1 << 30  # level histogram of one tree batch

COUNT, REAL = 0, 1
GINI, ENTROPY, MSE = 0, 1, 2
SPLIT_EPS = 1e-12

# floor(P(Poisson(1) <= k) * 2**32), k = 0..14: multiplicity = number of entries <= the hash
POISSON1_TABLE = (1580030168, 3160060337, 3950075421, 4213413783, 4279248373, 4292415291, 4294609777,
                  4294923276, 4294962463, 4294966817, 4294967252, 4294967292, 4294967295, 4294967295,
                  4294967295)

_M32 = 0xFFFFFFFF
_tables: Dict[torch.device, torch.Tensor] = {}


def task_id(task: str, criterion: str) -> int:
    if task == "regression":
        return MSE
    return ENTROPY if criterion == "entropy" else GINI


def check_shape(n_bins: int, n_classes: int) -> None:
    if n_bins > MAX_BINS:
        raise ValueError(f"native forest engine supports n_bins <= {MAX_BINS} (got {n_bins})")
    if n_classes > MAX_CLASSES:
        raise ValueError(f"native forest engine supports <= {MAX_CLASSES} classes (got {n_classes})")


# ---------------------------------------------------------------- hash (uint32 in int64 lanes)
def _mul32(x: torch.Tensor, k: int) -> torch.Tensor:
    return ((x & 0xFFFF) * k + ((((x >> 16) * k) & 0xFFFF) << 16)) & _M32


def _fmix(h: torch.Tensor) -> torch.Tensor:
    h = h ^ (h >> 16)
    h = _mul32(h, 0x85EBCA6B)
    h = h ^ (h >> 13)
    h = _mul32(h, 0xC2B2AE35)
    return h ^ (h >> 16)


def _hash3(a: int, b: torch.Tensor, c: torch.Tensor) -> torch.Tensor:
    h = _fmix(torch.full_like(b, ((a & _M32) + 0x9E3779B9) & _M32))
    h = _fmix(h ^ _mul32(b & _M32, 0x85EBCA77))
    return _fmix(h ^ _mul32(c & _M32, 0xC2B2AE3D))


def _hash4(a: int, b: torch.Tensor, c: torch.Tensor, d: torch.Tensor) -> torch.Tensor:
    return _fmix(_hash3(a, b, c) ^ _mul32(d & _M32, 0x27D4EB2F))


# ---------------------------------------------------------------- bin
def padded_width(d: int) -> int:
    return (d + 15) // 16 * 16


def bin_features(X: torch.Tensor, th: torch.Tensor) -> torch.Tensor:
    """uint8 bin ids [n, dpad] (dpad = d rounded up to 16, padding zero): bin = number of
    thresholds <= x, so ``Xb > b  <=>  x >= th[f, b]``."""
    n, d = X.shape
    check_shape(th.shape[1] + 1, 1)
    dpad = padded_width(d)
    Xb = torch.zeros((n, dpad), dtype=torch.uint8, device=X.device)
    th = th.to(device=X.device, dtype=torch.float64).contiguous()
    if not _lib.use_native(X):
        if th.shape[1] == 0:
            return Xb
        Xb[:, :d] = torch.searchsorted(th, X.double().t().contiguous(), right=True).t().to(torch.uint8)
        return Xb
    if X.dtype not in (torch.float32, torch.float64):
        X = X.double()
    X = X.contiguous()
    st = _lib.kernels().harp_forest_bin(X.data_ptr(), int(X.dtype == torch.float64), n, d, th.data_ptr(), th.shape[1],
                                        Xb.data_ptr(), dpad, _lib.stream_ptr(X.device))
    _lib.check(st, "forest_bin")
    return Xb


# ---------------------------------------------------------------- bootstrap
def bootstrap(seed: int, tree0: int, n_trees: int, row0: int, n: int, device) -> torch.Tensor:
    """Poisson(1) row multiplicities [n_trees, n] uint8 (capped at 15) of trees ``tree0..`` for
    the rows with global index ``row0..``: a function of (seed, tree, global row) alone."""
    device = torch.device(device)
    if MAX_MULT * (row0 + n) >= 1 << 32:
        raise ValueError("native forest engine needs 15 * n_global < 2**32")
    if device.type != "cuda":
        t = torch.arange(tree0, tree0 + n_trees, dtype=torch.int64)[:, None].expand(n_trees, n)
        r = torch.arange(row0, row0 + n, dtype=torch.int64)[None, :].expand(n_trees, n)
        u = _hash3(seed, t.contiguous(), r.contiguous())
        w = torch.zeros((n_trees, n), dtype=torch.int64)
        for k in POISSON1_TABLE:
            w += (u >= k).long()
        return w.to(torch.uint8).to(device)
    _lib.kernels()
    tab = _tables.get(device)
    if tab is None:
        tab = torch.tensor(POISSON1_TABLE, dtype=torch.int64).to(torch.int32).to(device)  # uint32 bit patterns
        _tables[device] = tab
    w = torch.empty((n_trees, n), dtype=torch.uint8, device=device)
    st = _lib.kernels().harp_forest_bootstrap(seed & _M32, tree0, n_trees, row0, n, tab.data_ptr(), w.data_ptr(),
                                              _lib.stream_ptr(device))
    _lib.check(st, "forest_bootstrap")
    return w


# ---------------------------------------------------------------- feature subset
def feature_subset(seed: int, fr_tree: torch.Tensor, fr_node: torch.Tensor, d: int, k: int) -> torch.Tensor:
    """uint8 mask [M, d]: node ``fr_node[j]`` of tree ``fr_tree[j]`` may split on the k features
    with the smallest hash of (seed, tree, node, f), ties to the lower f."""
    M = fr_tree.numel()
    dev = fr_tree.device
    if not _lib.use_native(fr_tree):
        t = fr_tree.long()[:, None].expand(M, d).contiguous()
        nd = fr_node.long()[:, None].expand(M, d).contiguous()
        f = torch.arange(d, dtype=torch.int64)[None, :].expand(M, d).contiguous()
        key = _hash4(seed, t, nd, f) * d + f  # (hash, f) order; < 2**32 * d
        rank = key.argsort(1).argsort(1)
        return (rank < k).to(torch.uint8)
    mask = torch.empty((M, d), dtype=torch.uint8, device=dev)
    st = _lib.kernels().harp_forest_feature_subset(seed & _M32, fr_tree.data_ptr(), fr_node.data_ptr(), M, d, k,
                                                   mask.data_ptr(), _lib.stream_ptr(dev))
    _lib.check(st, "forest_feature_subset")
    return mask


# ---------------------------------------------------------------- frontier plumbing
def chunk_table(cnt: torch.Tensor) -> torch.Tensor:
    """Exclusive scan [M + 1] (int32) of the number of CHUNK-row chunks of every node."""
    nch = (cnt.long() + (CHUNK - 1)) // CHUNK
    off = torch.zeros(cnt.numel() + 1, dtype=torch.int64, device=cnt.device)
    off[1:] = nch.cumsum(0)
    return off.int()


def _starts(cnt: torch.Tensor) -> torch.Tensor:
    c = cnt.long()
    return (c.cumsum(0) - c).int()


def _node_of_pos(cnt: torch.Tensor) -> torch.Tensor:
    return torch.repeat_interleave(torch.arange(cnt.numel(), device=cnt.device), cnt.long())


# ---------------------------------------------------------------- hist
def level_hist(Xb, order, cnt, fr_tree, mult, d: int, B: int, C: int, kind: int, y=None, stats=None,
               max_chunks: Optional[int] = None) -> torch.Tensor:
    """Histograms [M, d, B, C] of the frontier: node j owns rows order[start_j : start_j + cnt_j]
    (start = exclusive scan of cnt) of tree fr_tree[j]. ``count``: cell += mult[tree, row] at
    class y[row]; ``real``: cell[c] += stats[row, c] * mult[tree, row]."""
    check_shape(B, C)
    M = cnt.numel()
    dev = Xb.device
    if not _lib.use_native(Xb):
        H = torch.zeros((M * d * B, C), dtype=torch.int64 if kind == COUNT else torch.float64)
        if M == 0:
            return H.view(M, d, B, C)
        node = _node_of_pos(cnt)
        rows = order[:node.numel()].long()
        m = mult[fr_tree.long()[node], rows]
        idx = ((node[:, None] * d + torch.arange(d)[None, :]) * B + Xb[rows, :d].long()).reshape(-1)
        if kind == COUNT:
            val = torch.nn.functional.one_hot(y[rows].long(), C) * m.long()[:, None]
        else:
            val = stats[rows] * m.double()[:, None]
        H.index_add_(0, idx, val[:, None, :].expand(-1, d, -1).reshape(-1, C))
        return H.view(M, d, B, C)
    H = torch.zeros((M, d, B, C), dtype=torch.int32 if kind == COUNT else torch.float64, device=dev)
    if M == 0:
        return H
    coff = chunk_table(cnt)
    start = _starts(cnt)
    if max_chunks is None:
        max_chunks = order.numel() // CHUNK + M
    st = _lib.kernels().harp_forest_hist(
        Xb.data_ptr(), Xb.shape[1], order.data_ptr(), start.data_ptr(), cnt.data_ptr(), fr_tree.data_ptr(),
        coff.data_ptr(), M, max_chunks, mult.data_ptr(), mult.shape[1], _lib.ptr(y), _lib.ptr(stats), d, B, C, kind,
        H.data_ptr(), _lib.stream_ptr(dev))
    _lib.check(st, "forest_hist")
    return H


def counts_as_int64(H: torch.Tensor) -> torch.Tensor:
    """``count`` histogram as int64 (the GPU stores uint32 cells in an int32 tensor)."""
    return H.long() & _M32 if H.dtype == torch.int32 else H.long()


# ---------------------------------------------------------------- split (torch mirror)
def _ref_log2(p: torch.Tensor) -> torch.Tensor:
    m, e = torch.frexp(p)
    adj = m < 0.70710678118654752
    m = torch.where(adj, m * 2.0, m)
    e = e.double() - adj.double()
    s = (m - 1.0) / (m + 1.0)
    z = s * s
    q = torch.full_like(z, 1.0 / 23.0)
    for k in (21.0, 19.0, 17.0, 15.0, 13.0, 11.0, 9.0, 7.0, 5.0, 3.0):
        q = q * z + 1.0 / k
    q = q * z + 1.0
    return e + (2.0 * s * q) * 1.4426950408889634


def ref_impurity(S: torch.Tensor, task: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """(weighted impurity, weight) of statistics S [..., C] fp64: DecisionTree._impurity with
    the classes summed in index order."""
    if task == MSE:
        w, s, ss = S[..., 0], S[..., 1], S[..., 2]
        return ss - (s * s) / w.clamp_min(1e-300), w
    C = S.shape[-1]
    nn = torch.zeros_like(S[..., 0])
    for c in range(C):
        nn = nn + S[..., c]
    n = nn.clamp_min(1e-300)
    acc = torch.zeros_like(nn)
    for c in range(C):
        p = S[..., c] / n
        acc = acc + (p * _ref_log2(p.clamp_min(1e-300)) if task == ENTROPY else p * p)
    return ((-acc) * n if task == ENTROPY else (1.0 - acc) * n), nn


def _ref_prefix(H: torch.Tensor) -> torch.Tensor:
    if H.dtype != torch.float64:
        return H.cumsum(2)
    out = torch.empty_like(H)
    run = torch.zeros_like(H[:, :, 0])
    for b in range(H.shape[2]):  # sequential, as the kernel sums
        run = run + H[:, :, b]
        out[:, :, b] = run
    return out


def ref_gain_table(H: torch.Tensor, task: int, min_leaf: float, mask: Optional[torch.Tensor]) -> torch.Tensor:
    """Gains [M, d, B-1] of every candidate; -inf where min_samples_leaf or the feature mask
    forbids it."""
    pre = _ref_prefix(H)
    tot = pre[:, :, -1:, :]
    L = pre[:, :, :-1, :]
    R = tot - L
    iT, _ = ref_impurity(tot.double(), task)
    iL, nL = ref_impurity(L.double(), task)
    iR, nR = ref_impurity(R.double(), task)
    gain = (iT - iL) - iR
    ok = (nL >= min_leaf) & (nR >= min_leaf)
    if mask is not None:
        ok = ok & mask.bool()[:, :, None]
    return torch.where(ok, gain, torch.full_like(gain, float("-inf")))


def _first_max(g: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """(max, lowest index attaining it) over the last dim."""
    if g.shape[-1] == 0:
        z = g.new_full(g.shape[:-1], float("-inf"))
        return z, torch.zeros(g.shape[:-1], dtype=torch.int64, device=g.device)
    best = g.max(-1).values
    ar = torch.arange(g.shape[-1], device=g.device).expand_as(g)
    idx = torch.where(g == best[..., None], ar, torch.full_like(ar, g.shape[-1])).min(-1).values
    return best, idx


def split_feature(H: torch.Tensor, kind: int, task: int, min_leaf: float,
                  mask: Optional[torch.Tensor]) -> Tuple[torch.Tensor, torch.Tensor]:
    """Per (node, feature): best gain [M, d] fp64 and its bin [M, d] int32 (lowest bin among
    bitwise-equal gains)."""
    M, d, B, C = H.shape
    check_shape(B, C)
    if not _lib.use_native(H):
        g, b = _first_max(ref_gain_table(H, task, min_leaf, mask))
        return g, b.int()
    cg = torch.empty((M, d), dtype=torch.float64, device=H.device)
    cb = torch.empty((M, d), dtype=torch.int32, device=H.device)
    st = _lib.kernels().harp_forest_split_feature(H.data_ptr(), kind, M, d, B, C, task, float(min_leaf),
                                                  _lib.ptr(mask), cg.data_ptr(), cb.data_ptr(),
                                                  _lib.stream_ptr(H.device))
    _lib.check(st, "forest_split_feature")
    return cg, cb


def split_node(H: torch.Tensor, kind: int, cg: torch.Tensor, cb: torch.Tensor):
    """Per node: (feature, bin, gain, split flag, left stats, right stats, total stats). Ties
    over features go to the lowest feature; a node splits iff its gain > 1e-12."""
    M, d, B, C = H.shape
    dev = H.device
    if not _lib.use_native(H):
        bg, bf = _first_max(cg)
        ar = torch.arange(M)
        bb = cb[ar, bf].long()
        pre = _ref_prefix(H)
        tot = pre[ar, bf, -1]
        L = pre[ar, bf, bb]
        return (bf.int(), bb.int(), bg, (bg > SPLIT_EPS).int(), L.double(), (tot - L).double(),
                pre[:, 0, -1].double())
    of = torch.empty(M, dtype=torch.int32, device=dev)
    ob = torch.empty(M, dtype=torch.int32, device=dev)
    og = torch.empty(M, dtype=torch.float64, device=dev)
    sp = torch.empty(M, dtype=torch.int32, device=dev)
    L, R, T = (torch.empty((M, C), dtype=torch.float64, device=dev) for _ in range(3))
    st = _lib.kernels().harp_forest_split_node(H.data_ptr(), kind, M, d, B, C, cg.data_ptr(), cb.data_ptr(),
                                               of.data_ptr(), ob.data_ptr(), og.data_ptr(), sp.data_ptr(),
                                               L.data_ptr(), R.data_ptr(), T.data_ptr(), _lib.stream_ptr(dev))
    _lib.check(st, "forest_split_node")
    return of, ob, og, sp, L, R, T


# ---------------------------------------------------------------- route
def route_count(Xb, order, cnt, sp, sf, sbin, max_chunks: Optional[int] = None) -> torch.Tensor:
    """Rows of every split node that go left (Xb[row, f] <= bin) [M] int32; 0 for leaves."""
    M = cnt.numel()
    dev = Xb.device
    if not _lib.use_native(Xb):
        node = _node_of_pos(cnt)
        rows = order[:node.numel()].long()
        goes_left = (Xb[rows, sf.long()[node]].long() <= sbin.long()[node]) & sp.bool()[node]
        return torch.zeros(M, dtype=torch.int64).index_add_(0, node, goes_left.long()).int()
    nleft = torch.zeros(M, dtype=torch.int32, device=dev)
    if max_chunks is None:
        max_chunks = order.numel() // CHUNK + M
    start, coff = _starts(cnt), chunk_table(cnt)  # named: a temporary's block could be reused before the launch
    st = _lib.kernels().harp_forest_route_count(Xb.data_ptr(), Xb.shape[1], order.data_ptr(), start.data_ptr(),
                                                cnt.data_ptr(), coff.data_ptr(), M, max_chunks,
                                                sp.data_ptr(), sf.data_ptr(), sbin.data_ptr(), nleft.data_ptr(),
                                                _lib.stream_ptr(dev))
    _lib.check(st, "forest_route_count")
    return nleft


def route_scatter(Xb, order, cnt, sp, sf, sbin, nleft, child_start, max_chunks: Optional[int] = None) -> torch.Tensor:
    """New row order: the rows of split node j moved to [child_start[j], +nleft[j]) (left) and
    the range after it (right); rows of leaves dropped. The order inside a child is free."""
    M = cnt.numel()
    dev = Xb.device
    if not _lib.use_native(Xb):
        node = _node_of_pos(cnt)
        rows = order[:node.numel()].long()
        keep = sp.bool()[node]
        node, rows = node[keep], rows[keep]
        right = Xb[rows, sf.long()[node]].long() > sbin.long()[node]
        dest = torch.where(right, child_start.long()[node] + nleft.long()[node], child_start.long()[node])
        return rows[torch.sort(dest, stable=True).indices].int()
    new_order = torch.empty_like(order)
    cursor = torch.zeros((M, 2), dtype=torch.int32, device=dev)
    if max_chunks is None:
        max_chunks = order.numel() // CHUNK + M
    start, coff = _starts(cnt), chunk_table(cnt)
    st = _lib.kernels().harp_forest_route_scatter(
        Xb.data_ptr(), Xb.shape[1], order.data_ptr(), start.data_ptr(), cnt.data_ptr(),
        coff.data_ptr(), M, max_chunks, sp.data_ptr(), sf.data_ptr(), sbin.data_ptr(), nleft.data_ptr(),
        child_start.data_ptr(), cursor.data_ptr(), new_order.data_ptr(), new_order.numel(), _lib.stream_ptr(dev))
    _lib.check(st, "forest_route_scatter")
    return new_order


# ---------------------------------------------------------------- host loop
def trees_per_batch(n: int, d: int, B: int, C: int, kind: int, max_depth: int) -> int:
    """Trees grown together so that the widest level histogram stays under the budget."""
    per_node = d * B * C * (4 if kind == COUNT else 8)
    nodes = max(1, min(1 << max(0, min(max_depth, 40) - 1), n))
    return int(max(1, min(HIST_BUDGET_BYTES // (per_node * nodes), ((1 << 31) - 1) // max(n, 1))))


def grow(Xb: torch.Tensor, d: int, B: int, C: int, kind: int, mult: torch.Tensor, *, task: int, max_depth: int,
         min_leaf: float = 1, k_sub: Optional[int] = None, seed: int = 0, tree0: int = 0,
         y: Optional[torch.Tensor] = None, stats: Optional[torch.Tensor] = None,
         reduce: Optional[Callable[[torch.Tensor], None]] = None,
         trace: Optional[Callable[[int, dict], None]] = None) -> dict:
    """Grow ``mult.shape[0]`` trees level by level on the binned rows ``Xb`` [n, dpad].

    ``mult`` [T, n] uint8 row multiplicities; ``y`` [n] int32 labels (``count``) or ``stats``
    [n, C] fp64 (``real``); ``k_sub`` features per node (None / >= d: all) drawn by
    :func:`feature_subset` with tree ids ``tree0 + t``; ``reduce(H)`` sums a level histogram in
    place over the workers that hold the other row shards; ``trace(depth, state)`` receives the
    frontier, histogram, decisions and routing of every level that splits (tests). Returns the packed trees (device
    tensors): ``tree`` / ``feature`` (-1 = leaf) / ``bin`` / ``left`` (-1 = leaf) / ``stats``
    [N, C] sorted by (tree, node id), and ``sizes`` (python list, nodes per tree). Node ids are
    level order: children are appended left, then right, in frontier order."""
    check_shape(B, C)
    dev = Xb.device
    T, n = mult.shape
    if T * n >= 1 << 31:
        raise ValueError("native forest engine needs trees_per_batch * n < 2**31")
    mult = mult.contiguous()
    if kind == COUNT:
        y = y.to(device=dev, dtype=torch.int32).contiguous()
    else:
        stats = stats.to(device=dev, dtype=torch.float64).contiguous()
    use_subset = k_sub is not None and k_sub < d
    nz = (mult > 0).nonzero()
    order = nz[:, 1].int().contiguous()
    cnt = torch.bincount(nz[:, 0], minlength=T).int()
    fr_tree = torch.arange(T, dtype=torch.int32, device=dev)
    fr_node = torch.zeros(T, dtype=torch.int32, device=dev)
    fr_stats = None
    tree_nn = torch.ones(T, dtype=torch.int64, device=dev)
    tree_ids = torch.arange(T, device=dev)
    levels: List[tuple] = []
    M = T
    depth = 0
    while M > 0:
        last = depth >= max_depth
        if last and fr_stats is not None:
            break
        max_chunks = order.numel() // CHUNK + M
        H = level_hist(Xb, order, cnt, fr_tree, mult, d, B, C, kind, y=y, stats=stats, max_chunks=max_chunks)
        if reduce is not None:
            reduce(H)
        mask = feature_subset(seed, fr_tree + tree0, fr_node, d, k_sub) if use_subset else None
        cg, cb = split_feature(H, kind, task, min_leaf, mask)
        bf, bb, _, sp, Ls, Rs, Ts = split_node(H, kind, cg, cb)
        if fr_stats is None:
            fr_stats = Ts  # the roots
        if last:  # max_depth == 0: bare roots
            break
        spl = sp.long()
        incl = spl.cumsum(0)
        excl = incl - spl
        ft = fr_tree.long()
        first = torch.searchsorted(ft, tree_ids).clamp_max(M - 1)  # frontier is grouped by tree
        rank = excl - excl[first][ft]
        left = torch.where(sp.bool(), tree_nn[ft] + 2 * rank, torch.full_like(rank, -1))
        levels.append((fr_tree, fr_node, torch.where(sp.bool(), bf, torch.full_like(bf, -1)), bb, left, fr_stats))
        nsplit = int(incl[-1])  # the level's one device -> host read
        if nsplit == 0:
            M = 0
            break
        tree_nn = tree_nn + 2 * torch.zeros_like(tree_nn).index_add_(0, ft, spl)
        nleft = route_count(Xb, order, cnt, sp, bf, bb, max_chunks=max_chunks)
        sidx = torch.empty(nsplit + 1, dtype=torch.int64, device=dev)
        sidx[torch.where(sp.bool(), excl, torch.full_like(excl, nsplit))] = torch.arange(M, device=dev)
        sidx = sidx[:nsplit]
        nl = nleft[sidx]
        new_cnt = torch.stack([nl, cnt[sidx] - nl], 1).reshape(-1).contiguous()
        new_start = _starts(new_cnt)
        child_start = torch.zeros(M, dtype=torch.int32, device=dev)
        child_start[sidx] = new_start[0::2]
        new_order = route_scatter(Xb, order, cnt, sp, bf, bb, nleft, child_start, max_chunks=max_chunks)
        if trace is not None:
            trace(depth, dict(order=order, cnt=cnt, fr_tree=fr_tree, fr_node=fr_node, H=H, mask=mask, split=sp,
                              feature=bf, bin=bb, nleft=nleft, child_start=child_start, new_order=new_order,
                              new_cnt=new_cnt))
        order = new_order
        ll = left[sidx].int()
        fr_tree = fr_tree[sidx].repeat_interleave(2).contiguous()
        fr_node = torch.stack([ll, ll + 1], 1).reshape(-1).contiguous()
        fr_stats = torch.stack([Ls[sidx], Rs[sidx]], 1).reshape(-1, C)
        cnt = new_cnt
        M = 2 * nsplit
        depth += 1
    if M > 0:  # frontier left at max_depth: leaves
        neg = torch.full((M,), -1, dtype=torch.int32, device=dev)
        levels.append((fr_tree, fr_node, neg, torch.zeros_like(neg), neg.long(), fr_stats))
    tr = torch.cat([l[0] for l in levels]).long()
    nd = torch.cat([l[1] for l in levels]).long()
    perm = (tr * (int(nd.max()) + 1) + nd).argsort()
    return {
        "tree": tr[perm],
        "feature": torch.cat([l[2] for l in levels]).long()[perm],
        "bin": torch.cat([l[3] for l in levels]).long()[perm],
        "left": torch.cat([l[4] for l in levels]).long()[perm],
        "stats": torch.cat([l[5] for l in levels])[perm],
        "sizes": tree_nn.tolist(),
    }


# ---------------------------------------------------------------- packed-forest inference
def pack_trees(trees, device) -> dict:
    """Concatenate the arrays of ``trees`` (objects with feature / threshold / left / value and
    max_depth) for :func:`predict_packed`: int32 ``feature`` / ``left`` (ids local to the tree),
    fp64 ``threshold`` / ``value`` [N, C], int64 ``off`` [T + 1]."""
    sizes = [int(t.feature.numel()) for t in trees]
    off = torch.zeros(len(trees) + 1, dtype=torch.int64)
    off[1:] = torch.tensor(sizes, dtype=torch.int64).cumsum(0)
    C = int(trees[0].value.shape[1])
    if C > MAX_CLASSES:
        raise ValueError(f"native forest engine supports <= {MAX_CLASSES} classes (got {C})")
    return {
        "feature": torch.cat([t.feature for t in trees]).to(torch.int32).to(device),
        "threshold": torch.cat([t.threshold for t in trees]).double().to(device),
        "left": torch.cat([t.left for t in trees]).to(torch.int32).to(device),
        "value": torch.cat([t.value for t in trees]).double().contiguous().to(device),
        "off": off.to(device),
        "n_trees": len(trees),
        "C": C,
        "max_steps": max(sizes),  # a walk visits every node at most once
    }


def predict_packed(X: torch.Tensor, pack: dict, proba: bool = True, leaves: bool = False):
    """(mean leaf value over trees [n, C] fp64 or None, local leaf ids [T, n] int64 or None):
    every sample walks every tree on raw ``x >= threshold``; values are summed in tree order."""
    n, d = X.shape
    dev = X.device
    T, C = pack["n_trees"], pack["C"]
    if not _lib.use_native(X):
        Xd = X.double()
        out = torch.zeros((n, C), dtype=torch.float64) if proba else None
        leaf = torch.empty((T, n), dtype=torch.int64) if leaves else None
        for t in range(T):
            a, b = int(pack["off"][t]), int(pack["off"][t + 1])
            f, th, l = pack["feature"][a:b].long(), pack["threshold"][a:b], pack["left"][a:b].long()
            node = torch.zeros(n, dtype=torch.int64)
            for _ in range(b - a):
                lf = l[node]
                inner = lf >= 0
                if not bool(inner.any()):
                    break
                xv = Xd.gather(1, f[node].clamp_min(0)[:, None])[:, 0]
                node = torch.where(inner, lf + (xv >= th[node]).long(), node)
            if proba:
                out = out + pack["value"][a:b][node]
            if leaves:
                leaf[t] = node
        return (out / T if proba else None), leaf
    if X.dtype not in (torch.float32, torch.float64):
        X = X.double()
    X = X.contiguous()
    out = torch.empty((n, C), dtype=torch.float64, device=dev) if proba else None
    leaf = torch.empty((T, n), dtype=torch.int64, device=dev) if leaves else None
    st = _lib.kernels().harp_forest_predict(
        X.data_ptr(), int(X.dtype == torch.float64), n, d, pack["feature"].data_ptr(), pack["threshold"].data_ptr(),
        pack["left"].data_ptr(), pack["value"].data_ptr(), pack["off"].data_ptr(), T, C, pack["max_steps"],
        _lib.ptr(out), _lib.ptr(leaf), _lib.stream_ptr(dev))
    _lib.check(st, "forest_predict")
    return out, leaf
