"""Apriori support counting on vertical bitmaps (``csrc/apriori.hip``).

Transactions are held as one row of bits per item, one bit per local transaction
(:class:`Bitmaps`): 1e6 transactions x 1e4 items are 1.25 GB, and every support is a popcount
of ANDed rows. Nothing here forms an n x items array. Four ops -- :func:`pack` (+
:func:`item_counts`, level 1), :func:`pair_counts` (level 2, a bit "GEMM"), :func:`count`
(level k, candidates in runs that share their first k-1 items) and :func:`prune` (Apriori
property) -- launch the native kernels on a HIP device; on CPU tensors each runs its vectorised
torch mirror (``*_ref``: int64 words, popcount by a byte table), which is also the oracle of
the GPU tests. :func:`join` and :func:`groups` are index arithmetic in torch on both devices.
All counts are integers, so the two paths agree exactly.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Optional

import torch

from . import _lib

_P, _I, _L = _lib.c_void_p, _lib.c_int, _lib.c_long
_lib.register({
    "harp_apriori_pair_tile": [],
    "harp_apriori_pair_kw": [],
    "harp_apriori_ext_cap": [],
    "harp_apriori_max_k": [],
    "harp_apriori_slab4": [],
    "harp_apriori_pack": [_P, _P, _L, _I, _I, _L, _P, _P, _P],
    "harp_apriori_popcount": [_P, _I, _L, _P, _P],
    "harp_apriori_pairs": [_P, _P, _I, _L, _L, _P, _P],
    "harp_apriori_count": [_P, _P, _P, _I, _I, _L, _I, _P, _P],
    "harp_apriori_prune": [_P, _L, _I, _P, _L, _P, _P],
})

PAIR_TILE = 64   # items per side of a pair tile (APRIORI_PAIR_TILE in csrc/apriori.hip)
PAIR_KW = 32     # 32-bit words of a row staged per step
EXT_CAP = 64     # candidates of one count workgroup: longer runs are split
MAX_K = 64       # longest itemset of the native count / prune kernels
SLAB4 = 1024     # 16-byte words of a count slab
# workgroups the slab choices aim at (8 per CU). A choice, not a measurement.
TARGET_WORKGROUPS = 2048
_REF_CHUNK = 1 << 22  # int64 words per slice of the torch mirrors

_POP8 = torch.tensor([bin(i).count("1") for i in range(256)], dtype=torch.uint8)
_checked = False


def _kern():
    global _checked
    lib = _lib.kernels()
    if not _checked:
        assert (lib.harp_apriori_pair_tile(), lib.harp_apriori_pair_kw(), lib.harp_apriori_ext_cap(),
                lib.harp_apriori_max_k(), lib.harp_apriori_slab4()) == (PAIR_TILE, PAIR_KW, EXT_CAP, MAX_K, SLAB4)
        _checked = True
    return lib


@dataclass
class Bitmaps:
    words: torch.Tensor  # int64 [n_items, W64], W64 even (rows are 16-byte multiples), padding bits zero
    n: int               # local transactions

    @property
    def n_items(self) -> int:
        return self.words.shape[0]

    @property
    def W(self) -> int:
        """32-bit words per row (a multiple of 4)."""
        return 2 * self.words.shape[1]

    @property
    def device(self) -> torch.device:
        return self.words.device

    @property
    def nbytes(self) -> int:
        return self.words.numel() * 8


def row_words64(n: int) -> int:
    """int64 words of a row of n bits, padded to 16 bytes."""
    return max(2, (n + 127) // 128 * 2)


def _popcount_rows(X: torch.Tensor) -> torch.Tensor:
    """int64 [r, w] -> popcount of every row (int64 [r]) by a byte table."""
    r, w = X.shape
    out = torch.zeros(r, dtype=torch.int64, device=X.device)
    if r == 0 or w == 0:
        return out
    tab = _POP8.to(X.device)
    step = max(1, _REF_CHUNK // w)
    for a in range(0, r, step):
        b = X[a:a + step].contiguous().view(torch.uint8)
        out[a:a + step] = tab[b.long()].sum(1, dtype=torch.int64)
    return out


# ------------------------------------------------------------------ pack / level 1
def _check_pairs(tids, items, n, n_items):
    assert tids.shape == items.shape and tids.dim() == 1
    assert 0 <= n < 2 ** 31, "a rank holds fewer than 2^31 transactions"


def pack_ref(tids: torch.Tensor, items: torch.Tensor, n: int, n_items: int) -> Bitmaps:
    _check_pairs(tids, items, n, n_items)
    w64 = row_words64(n)
    t, it = tids.long(), items.long()
    if t.numel() and (int(t.min()) < 0 or int(t.max()) >= n or int(it.min()) < 0 or int(it.max()) >= n_items):
        raise ValueError(f"pair outside [0, {n}) x [0, {n_items})")
    key = torch.unique(it * (w64 * 64) + t)  # one key per set bit: the sum below is then an OR
    words = torch.zeros(n_items * w64, dtype=torch.int64, device=tids.device)
    words.index_add_(0, key >> 6, torch.bitwise_left_shift(torch.ones_like(key), key & 63))
    return Bitmaps(words.view(n_items, w64), n)


def pack(tids: torch.Tensor, items: torch.Tensor, n: int, n_items: int) -> Bitmaps:
    """Bitmaps of (dense local tid, item) pairs; a duplicated pair is harmless. A pair outside
    [0, n) x [0, n_items) raises ``ValueError``."""
    if not _lib.use_native(tids):
        return pack_ref(tids, items, n, n_items)
    _check_pairs(tids, items, n, n_items)
    dev = tids.device
    words = torch.zeros((n_items, row_words64(n)), dtype=torch.int64, device=dev)
    B = Bitmaps(words, n)
    if tids.numel():
        t32 = tids.to(torch.int32).contiguous()
        i32 = items.to(dev, torch.int32).contiguous()
        err = torch.zeros(1, dtype=torch.int32, device=dev)
        _lib.check(_kern().harp_apriori_pack(t32.data_ptr(), i32.data_ptr(), t32.numel(), n, n_items, B.W,
                                             words.data_ptr(), err.data_ptr(), _lib.stream_ptr(dev)), "apriori_pack")
        if int(err) != 0:
            raise ValueError(f"pair outside [0, {n}) x [0, {n_items})")
    return B


def pack_dense(T: torch.Tensor) -> Bitmaps:
    """Bitmaps of ``T != 0`` for a dense [n, items] matrix."""
    nz = torch.nonzero(T)
    return pack(nz[:, 0], nz[:, 1], T.shape[0], T.shape[1])


def item_counts_ref(B: Bitmaps) -> torch.Tensor:
    return _popcount_rows(B.words).to(torch.int32)


def item_counts(B: Bitmaps) -> torch.Tensor:
    """Support of every item (int32 [n_items])."""
    if not _lib.use_native(B.words):
        return item_counts_ref(B)
    out = torch.zeros(B.n_items, dtype=torch.int32, device=B.device)
    _lib.check(_kern().harp_apriori_popcount(B.words.data_ptr(), B.n_items, B.W, out.data_ptr(),
                                             _lib.stream_ptr(B.device)), "apriori_popcount")
    return out


# ------------------------------------------------------------------ level 2
def _check_rows(B: Bitmaps, idx: torch.Tensor):
    if idx.numel() and (int(idx.min()) < 0 or int(idx.max()) >= B.n_items):
        raise ValueError(f"item outside [0, {B.n_items})")


def pair_counts_ref(B: Bitmaps, idx: torch.Tensor) -> torch.Tensor:
    R = B.words[idx.long()]
    m, w = R.shape
    S = torch.zeros((m, m), dtype=torch.int32, device=B.device)
    step = max(1, _REF_CHUNK // max(1, m * w))
    for a in range(0, m, step):
        blk = R[a:a + step, None, :] & R[None, :, :]
        S[a:a + step] = _popcount_rows(blk.reshape(-1, w)).view(-1, m).to(torch.int32)
    return torch.triu(S)


def pair_slab_words(m: int, W: int) -> int:
    """Words of a row per workgroup of the pair kernel: rows are split until about
    ``TARGET_WORKGROUPS`` workgroups exist."""
    nt = (m + PAIR_TILE - 1) // PAIR_TILE
    chunks = (W + PAIR_KW - 1) // PAIR_KW
    nslab = max(1, min(chunks, 65535, TARGET_WORKGROUPS // (nt * (nt + 1) // 2)))
    return max(-(-chunks // nslab), -(-chunks // 65535)) * PAIR_KW


def pair_counts(B: Bitmaps, idx: torch.Tensor, slab_words: Optional[int] = None) -> torch.Tensor:
    """``S [m, m]`` (int32): ``S[a, b]`` = transactions that hold items ``idx[a]`` and ``idx[b]``,
    for a <= b. Only the upper triangle is defined (the lower one is zero)."""
    _check_rows(B, idx)
    if not _lib.use_native(B.words):
        return pair_counts_ref(B, idx)
    m = idx.numel()
    S = torch.zeros((m, m), dtype=torch.int32, device=B.device)
    if m:
        i32 = idx.to(B.device, torch.int32).contiguous()
        slab_words = slab_words or pair_slab_words(m, B.W)
        _lib.check(_kern().harp_apriori_pairs(B.words.data_ptr(), i32.data_ptr(), m, B.W, slab_words, S.data_ptr(),
                                              _lib.stream_ptr(B.device)), "apriori_pairs")
    return S


# ------------------------------------------------------------------ join / prune
def join(prev: torch.Tensor) -> torch.Tensor:
    """Candidates of size k from the lexicographically sorted large (k-1)-itemsets ``prev
    [m, k-1]``: every ordered pair of rows that share their first k-2 items, in lexicographic
    order (so runs of candidates share their first k-1 items)."""
    m, k1 = prev.shape
    dev = prev.device
    if m < 2:
        return prev.new_zeros((0, k1 + 1))
    ar = torch.arange(m, device=dev)
    new = torch.ones(m, dtype=torch.bool, device=dev)
    if k1 > 1:
        new[1:] = (prev[1:, :-1] != prev[:-1, :-1]).any(1)
    else:
        new[1:] = False
    gid = torch.cumsum(new.long(), 0) - 1
    end = torch.cat([ar[new][1:], ar.new_tensor([m])])[gid]  # one past the last row of the row's group
    nout = end - 1 - ar
    i = torch.repeat_interleave(ar, nout)
    first = torch.cumsum(nout, 0) - nout
    j = i + 1 + (torch.arange(i.numel(), device=dev) - first[i])
    return torch.cat([prev[i], prev[j, -1:]], 1)


def prune_ref(cand: torch.Tensor, prev: torch.Tensor) -> torch.Tensor:
    c, k = cand.shape
    keep = torch.ones(c, dtype=torch.bool, device=cand.device)
    m = prev.shape[0]
    for drop in range(k - 2):
        sub = torch.cat([cand[:, :drop], cand[:, drop + 1:]], 1)
        inv = torch.unique(torch.cat([prev.to(sub.dtype), sub]), dim=0, return_inverse=True)[1]
        keep &= torch.isin(inv[m:], inv[:m])
    return keep


def prune(cand: torch.Tensor, prev: torch.Tensor) -> torch.Tensor:
    """Apriori property for joined candidates ``cand [c, k]``: a bool flag per candidate, true
    where every (k-1)-subset that drops one of the first k-2 positions is a row of the sorted
    ``prev [m, k-1]``. (Dropping either of the last two positions gives the joined rows.)"""
    c, k = cand.shape
    assert prev.dim() == 2 and prev.shape[1] == k - 1
    if not _lib.use_native(cand):
        return prune_ref(cand, prev)
    dev = cand.device
    keep = torch.ones(c, dtype=torch.uint8, device=dev)
    if c and k > 2:
        c32, p32 = cand.to(torch.int32).contiguous(), prev.to(dev, torch.int32).contiguous()
        _lib.check(_kern().harp_apriori_prune(c32.data_ptr(), c, k, p32.data_ptr(), p32.shape[0], keep.data_ptr(),
                                              _lib.stream_ptr(dev)), "apriori_prune")
    return keep.bool()


# ------------------------------------------------------------------ level k
def groups(cand: torch.Tensor, cap: int = EXT_CAP) -> torch.Tensor:
    """``group_off [g + 1]`` (int32): bounds of the runs of ``cand [c, k]`` that share their
    first k-1 items, runs longer than ``cap`` split into sub-runs."""
    c = cand.shape[0]
    dev = cand.device
    ar = torch.arange(c, device=dev)
    new = torch.ones(c, dtype=torch.bool, device=dev)
    if c > 1:
        new[1:] = (cand[1:, :-1] != cand[:-1, :-1]).any(1)
    start = torch.cummax(torch.where(new, ar, torch.zeros_like(ar)), 0).values if c else ar
    bound = new | ((ar - start) % cap == 0)
    return torch.cat([ar[bound], ar.new_tensor([c])]).to(torch.int32)


def count_ref(B: Bitmaps, cand: torch.Tensor) -> torch.Tensor:
    c, k = cand.shape
    out = torch.zeros(c, dtype=torch.int32, device=B.device)
    w = B.words.shape[1]
    step = max(1, _REF_CHUNK // w)
    cl = cand.long()
    for a in range(0, c, step):
        acc = B.words[cl[a:a + step, 0]]
        for j in range(1, k):
            acc = acc & B.words[cl[a:a + step, j]]
        out[a:a + step] = _popcount_rows(acc).to(torch.int32)
    return out


def count_slab4(g: int, W: int) -> int:
    """16-byte words of a row per workgroup of the count kernel (at most ``SLAB4``)."""
    W4 = W // 4
    least = -(-W4 // SLAB4)
    nslab = max(least, min(-(-TARGET_WORKGROUPS // max(g, 1)), -(-W4 // 64)))
    return -(-W4 // nslab)


def count(B: Bitmaps, cand: torch.Tensor, group_off: Optional[torch.Tensor] = None,
          slab4: Optional[int] = None) -> torch.Tensor:
    """Supports (int32 [c]) of the itemsets ``cand [c, k]``, k >= 2, sorted lexicographically.
    ``group_off``: run bounds from :func:`groups` (computed when None)."""
    c, k = cand.shape
    assert k >= 2
    _check_rows(B, cand)
    if not _lib.use_native(B.words):
        return count_ref(B, cand)
    if k > MAX_K:
        raise ValueError(f"itemsets of {k} items: the native engine takes at most {MAX_K}")
    dev = B.device
    out = torch.zeros(c, dtype=torch.int32, device=dev)
    if c == 0:
        return out
    c32 = cand.to(dev, torch.int32).contiguous()
    if group_off is None:
        group_off = groups(c32)
    group_off = group_off.to(dev, torch.int32).contiguous()
    g = group_off.numel() - 1
    assert int(group_off[0]) == 0 and int(group_off[-1]) == c
    sizes = group_off[1:] - group_off[:-1]
    assert int(sizes.min()) >= 0 and int(sizes.max()) <= EXT_CAP
    slab4 = slab4 or count_slab4(g, B.W)
    _lib.check(_kern().harp_apriori_count(B.words.data_ptr(), c32.data_ptr(), group_off.data_ptr(), g, k, B.W, slab4,
                                          out.data_ptr(), _lib.stream_ptr(dev)), "apriori_count")
    return out
