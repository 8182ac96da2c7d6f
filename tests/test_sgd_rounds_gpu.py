"""Exact multi-round tests of the XCD-blocked MF-SGD kernels (csrc/mf_sgd.hip).

The one-stream-per-cell tests (test_sgd_mf_gpu.py, test_sgd_rank_placement_gpu.py) reach the
LDS round only in its trivial form: one round, one stream, r0 == 0, CH == 128. Here every
cell holds S streams that share no user and no item, so the result does not depend on the
order in which the streams run and the GPU must equal the sequential CPU schedule -- over
several rounds per cell, the round stride of blocks_per_xcd > 1, a last round with idle
subgroups, a last stream shorter than CH, every CH, and wrapping windows."""
import functools

import pytest
import torch

from harp_amd.ops import mf as MF

pytestmark = pytest.mark.gpu

NB = MF.XCDS
# item (0..3) of rating k of a stream: repeats at distance 1 (3 3), 2 (1 2 1), 4 and more, so
# both in-register forwards of sgd_stream_lds (same item as rating i, as rating i - 1) are taken
ITEM_PATTERN = (0, 1, 2, 3, 3, 1, 2, 1, 0)


def _assert_streams_disjoint(rows, cols, stream, cell, users_per_cell):
    """No two streams of one sub-step share a user or an item, and with users_per_cell no two
    cells share a user at all (a wrong fixture fails here, not as a tolerance)."""
    ub, ib = cell // NB, cell % NB
    if users_per_cell:
        big = int(rows.max()) + 1
        assert torch.unique(cell * big + rows.long()).numel() == torch.unique(rows).numel(), "two cells share a user"
    for step in range(NB):
        m = ib == (ub + step) % NB
        for ids in (rows[m].long(), cols[m].long()):
            big = int(ids.max()) + 1
            owners = torch.unique(stream[m] * big + ids).numel()  # distinct (stream, id) pairs
            assert owners == torch.unique(ids).numel(), f"sub-step {step}: an id is used by two streams"


def _ratings(S, CH, short_last, users_per_cell):
    """64 cells of S streams of CH ratings (the last one CH - 3 if short_last). Stream s of cell
    (ub, ib) uses the users ub*UB + 2s, + 2s+1 (switching inside the stream) and the items
    ib*IB + 4s + (0..3); user-sorted inside the cell, stream boundaries at multiples of CH.

    users_per_cell (the flow kernel's cases): the users are private to the cell, ub*UB +
    ib*2S + 2s (+1) with UB = 2*S*8. The per-sub-step kernels order the sub-steps of a user
    block by kernel boundaries; the flow kernel orders sub-step s + 1 of an XCD only behind its
    neighbour's sub-step s (the item block), and a block that finds no more rounds in s moves
    on while its siblings still train rounds of s -- so with more than one block per XCD two
    consecutive sub-steps may touch one user block at the same time, and only users that no
    two cells share make the result independent of the order."""
    UB, IB = 2 * S * (NB if users_per_cell else 1), 4 * S
    lens = [CH] * S
    if short_last:
        lens[-1] = CH - 3
    s_id = torch.cat([torch.full((n,), s) for s, n in enumerate(lens)])
    k = torch.cat([torch.arange(n) for n in lens])
    user = 2 * s_id + (k >= CH // 3).long()
    item = 4 * s_id + torch.tensor(ITEM_PATTERN)[k % len(ITEM_PATTERN)]
    m = k.numel()
    cell = torch.arange(NB * NB)
    rows = ((cell // NB)[:, None] * UB + user[None, :]).reshape(-1)
    if users_per_cell:
        rows = rows + ((cell % NB)[:, None] * 2 * S).expand(-1, m).reshape(-1)
    cols = ((cell % NB)[:, None] * IB + item[None, :]).reshape(-1)
    stream = (cell[:, None] * S + s_id[None, :]).reshape(-1)
    cell_of = cell[:, None].expand(-1, m).reshape(-1)
    off = torch.arange(NB * NB + 1, dtype=torch.int64) * m
    assert bool((rows.view(NB * NB, m)[:, 1:] >= rows.view(NB * NB, m)[:, :-1]).all())  # user-sorted
    _assert_streams_disjoint(rows, cols, stream, cell_of, users_per_cell)
    return rows.int(), cols.int(), off, NB * UB, NB * IB


@functools.lru_cache(maxsize=None)
def _case(r, CH, S, windows=False, users_per_cell=False):
    """Ratings, initial factors and the CPU schedule's result (computed once per shape, shared
    by the cases that differ only in kernel variant, grid or write-back mode; never modified)."""
    R, C, off, nu, ni = _ratings(S, CH, short_last=not windows, users_per_cell=users_per_cell)
    g = torch.Generator().manual_seed(1000 * r + CH)
    V = torch.rand(R.numel(), generator=g) * 4 + 1
    scale = 0.3 * ((16.0 / r) ** 0.5 if r > 256 else 1.0)  # wide ranks: as the neighbouring wide tests
    W0 = torch.rand(nu, r, generator=g) * scale
    H0 = torch.rand(ni, r, generator=g) * scale
    win = None
    if windows:
        # every cell has S*CH ratings; the window starts on a stream boundary past the middle
        # and wraps, so the GPU's stream cuts still fall on the fixture's stream boundaries
        starts = [(S // 2 + 1 + c % 5) * CH for c in range(NB * NB)]
        lens = [(S - 12 + c % 7) * CH + 5 for c in range(NB * NB)]
        assert all(s % CH == 0 and S * CH // 2 < s < S * CH and s + n > S * CH and n < S * CH
                   for s, n in zip(starts, lens))
        win = (starts, lens)
    lr = 0.002 if r > 256 else 0.01
    Wc, Hc = W0.clone(), H0.clone()
    n = MF.sgd_update_blocked(R, C, V, off, Wc, Hc, lr, 0.05, window=win)
    assert n == (sum(win[1]) if windows else R.numel())
    return R, C, V, off, W0, H0, Wc, Hc, win, lr


def _run_and_compare(cuda, r, CH, S, bpx, variant=0, atomic=0, windows=False):
    R, C, V, off, W0, H0, Wc, Hc, win, lr = _case(r, CH, S, windows, users_per_cell=variant == MF.FLOW_VARIANT)
    Wg, Hg = W0.to(cuda), H0.to(cuda)
    n = MF.sgd_update_blocked(R.to(cuda), C.to(cuda), V.to(cuda), off.to(cuda), Wg, Hg, lr, 0.05, chunk=CH,
                              blocks_per_xcd=bpx, variant=variant, atomic=atomic, window=win)
    torch.cuda.synchronize()
    assert n == (sum(win[1]) if windows else R.numel())
    rtol = 1e-4 if r > 256 else 0.0
    dw, dh = (Wg.cpu() - Wc).abs().max().item(), (Hg.cpu() - Hc).abs().max().item()
    print(f"r {r} CH {CH} S {S} bpx {bpx} variant {variant} atomic {atomic}: max |dW| {dw:.3g} |dH| {dh:.3g}")
    assert torch.allclose(Wg.cpu(), Wc, atol=2e-5, rtol=rtol) and torch.allclose(Hg.cpu(), Hc, atol=2e-5, rtol=rtol)


# S = 37: three rounds of 16 streams, the last one with 5 live subgroups and a partial last
# stream; blocks_per_xcd 1: one block takes all rounds, 3: rounds j, j + 3, .. (blocks idle in
# the tail)
S_NARROW = 37
BPX = (1, 3)


@pytest.mark.parametrize("bpx", BPX)
@pytest.mark.parametrize("CH", [8, 16, 32, 64, 128])
@pytest.mark.parametrize("r,atomic", [(16, 0), (16, 3), (48, 0), (48, 3), (128, 0)])
def test_xcd_rounds_match_cpu(cuda, r, atomic, CH, bpx):
    _run_and_compare(cuda, r, CH, S_NARROW, bpx, atomic=atomic)


@pytest.mark.parametrize("bpx", BPX)
@pytest.mark.parametrize("atomic", [0, 3])
@pytest.mark.parametrize("CH", [8, 64])
@pytest.mark.parametrize("r", [16, 48])
def test_placed_rounds_match_cpu(cuda, r, CH, atomic, bpx):
    _run_and_compare(cuda, r, CH, S_NARROW, bpx, variant=MF.PLACED_VARIANT, atomic=atomic)
    assert int(MF._chk(cuda).pws.abs().sum()) == 0  # claim counters reset, no cell drained


@pytest.mark.parametrize("bpx", BPX)
@pytest.mark.parametrize("CH", [8, 32, 128])
@pytest.mark.parametrize("r", [16, 128])
def test_flow_rounds_match_cpu(cuda, r, CH, bpx):
    _run_and_compare(cuda, r, CH, S_NARROW, bpx, variant=MF.FLOW_VARIANT)
    MF.check_flow_errors(cuda)


@pytest.mark.parametrize("bpx", BPX)
@pytest.mark.parametrize("CH", [32, 128])
def test_wide_xcd_rounds_match_cpu(cuda, CH, bpx):
    """One wave per stream: 4 streams per block and round, so S = 9 gives rounds of 4, 4, 1."""
    _run_and_compare(cuda, 260, CH, 9, bpx)


@pytest.mark.parametrize("bpx", BPX)
@pytest.mark.parametrize("variant", [0, MF.FLOW_VARIANT])
def test_window_rounds_match_cpu(cuda, variant, bpx):
    """Wrapping windows of k*CH + 5 ratings from a stream boundary past the middle of the cell."""
    _run_and_compare(cuda, 32, 16, S_NARROW, bpx, variant=variant, windows=True)
    if variant == MF.FLOW_VARIANT:
        MF.check_flow_errors(cuda)
