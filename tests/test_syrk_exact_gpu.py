"""Exact tests of every form of the MFMA SYRK (csrc/syrk.hip) and of its layout kernel.

Inputs are integers in [-4, 4] stored as bf16: every product is an integer of magnitude
<= 16 and every partial sum an integer below 2^24, so MFMA order, split order and atomic
order cannot change a bit of the fp32 result, while any indexing, staging, synchronisation
or coverage error changes an integer. Every comparison is ``torch.equal``.

``G`` is a ``[:, :d_pad]`` view of a ``[d_pad, d_pad + 32]`` buffer (ldg > d_pad), prefilled
with random integers G0 below 2^20, the 32 padding columns with a sentinel. After the call
  * on and above the diagonal G - G0 is the reference,
  * strictly below it every element of G - G0 is 0 or the reference value (the kernel may
    skip lower 32-blocks),
  * the padding columns still hold the sentinel,
  * ``symmetrize_upper(G - G0)`` is the full reference.

Which form a case reaches (tile size, work items, splits, stages per split, workgroups) is
computed by ``tests.syrk_cases.launch_plan``, a Python copy of the launch rules; the tables
in that module name the forms and tests/test_syrk_oracle.py checks them on the CPU. In the
ids below ``s`` lists the stages of each split and ``wg`` is the grid size.

155 cases, 4 s on the MI355X, the slowest 0.5 s (the first one: it loads the library).
"""
import pytest
import torch

from harp_amd.ops import _lib
from harp_amd.ops import linalg as LA
from tests import syrk_cases as SC

pytestmark = pytest.mark.gpu

SENTINEL = -12345.0
_CASES: dict = {}


def _case(cuda, d_pad, d, ld):
    """(FeatureMajor, reference Gram) of the integer case (d_pad, d, ld), built once."""
    key = (d_pad, d, ld)
    if key not in _CASES:
        assert 16 * ld + 2**20 < 2**24 and SC.exact_ok(ld)
        n = ld - 5  # the last 5 samples of the last block are padding
        Xb = SC.int_rows(n, d, seed=d_pad * 100003 + 17 * d + ld, device=cuda)
        XT = SC.feature_major_ref(Xb, n, d, ld, d_pad)
        _CASES[key] = (LA.FeatureMajor(XT, n, d), SC.gram_ref(XT))
    return _CASES[key]


def _check_exact(fm, ref, calls=1, **kw):
    d_pad, dev = fm.d_pad, fm.XT.device
    g = torch.Generator(device=dev).manual_seed(d_pad + fm.ld)
    buf = torch.full((d_pad, d_pad + 32), SENTINEL, dtype=torch.float32, device=dev)
    G = buf[:, :d_pad]
    G0 = torch.randint(-(2**20) + 1, 2**20, (d_pad, d_pad), generator=g, device=dev).float()
    G.copy_(G0)
    for _ in range(calls):
        assert LA.syrk_t(fm, G, **kw) is G
    diff, want = G - G0, ref * calls
    assert torch.equal(torch.triu(diff), torch.triu(want))
    low, wlow = torch.tril(diff, -1), torch.tril(want, -1)
    assert torch.equal(torch.where(low == 0, wlow, low), wlow)  # 0 or the reference, nothing else
    assert torch.equal(buf[:, d_pad:], torch.full_like(buf[:, d_pad:], SENTINEL))
    assert torch.equal(LA.symmetrize_upper(diff), want)


def _plan_id(d_pad, ld, ns=0):
    p = SC.launch_plan(d_pad, ld, ns)
    st = "+".join(map(str, p["stages"])) if len(set(p["stages"])) > 1 else f"{p['splits']}x{p['stages'][0]}"
    return f"dpad{d_pad}-t{p['mt']}-nt{p['nt']}-ld{ld}-s{st}-wg{p['workgroups']}"


# ----------------------------------------------------------------------------- tile forms
@pytest.mark.parametrize("ld", SC.TILE_LDS, ids=lambda v: f"ld{v}")
@pytest.mark.parametrize("d_pad,d,tile,nt,form", SC.TILE_FORMS,
                         ids=[f"dpad{t[0]}-d{t[1]}-t{t[2]}-nt{t[3]}" for t in SC.TILE_FORMS])
def test_tile_forms(cuda, d_pad, d, tile, nt, form, ld):
    """Every padded width of SC.TILE_FORMS (the ``form`` column says what it reaches) with
    auto splits: ld = 192 is one split of 4 stages, ld = 6192 two splits of 65 + 64 stages
    (one of 129 for 5, 85 and 41 work items, see test_tile_forms_more_auto_splits)."""
    p = SC.launch_plan(d_pad, ld)
    assert (p["mt"], p["nt"]) == (tile, nt)
    _check_exact(*_case(cuda, d_pad, d, ld), num_splits=0)


@pytest.mark.parametrize("d_pad,d,ld,stages", SC.TILE_EXTRA, ids=[_plan_id(t[0], t[2]) for t in SC.TILE_EXTRA])
def test_tile_forms_more_auto_splits(cuda, d_pad, d, ld, stages):
    """Several auto splits, the last one short, for the widths whose auto split count falls
    to 1 at ld = 6192; for 1664 and 2304 the split count comes from the target_wg chooser."""
    assert SC.launch_plan(d_pad, ld)["stages"] == stages
    _check_exact(*_case(cuda, d_pad, d, ld), num_splits=0)


# ----------------------------------------------------------------------------- ring edges
@pytest.mark.parametrize("ld,ns,stages", SC.RING_EDGES,
                         ids=[f"ld{e[0]}-ns{e[1]}-s{'+'.join(map(str, e[2]))}" for e in SC.RING_EDGES])
@pytest.mark.parametrize("d_pad", SC.RING_PANELS, ids=lambda v: f"dpad{v}")
def test_ring_edges(cuda, d_pad, ld, ns, stages):
    """1, 2 and 3 stages per split (the prologue and the i + 1 / i + 2 guards at their
    edges), a last split shorter than the others, 7 + 6 stages; d_pad = 128 / 768 hold
    one-panel jobs (vmcnt(3)), 256 / 512 only two-panel jobs (vmcnt(6)), at both tiles."""
    assert SC.launch_plan(d_pad, ld, ns)["stages"] == stages
    _check_exact(*_case(cuda, d_pad, d_pad - 3, ld), num_splits=ns)


# ---------------------------------------------------------------------------------- remap
@pytest.mark.parametrize("d_pad,ld,ns,wg", SC.REMAP, ids=[_plan_id(r[0], r[1], r[2]) for r in SC.REMAP])
def test_xcd_remap_is_a_bijection(cuda, d_pad, ld, ns, wg):
    """Forced splits with a grid of ``wg`` workgroups: wg % 8 != 0 runs the r8 != 0 arm of
    the blockIdx remap over several splits (a tile done twice or never changes an integer)."""
    assert SC.launch_plan(d_pad, ld, ns)["workgroups"] == wg
    _check_exact(*_case(cuda, d_pad, d_pad - 2, ld), num_splits=ns)


# ------------------------------------------------------------------------- lock-step hint
@pytest.mark.parametrize("sync_every", SC.SYNC_EVERY, ids=lambda v: f"sync{v}")
@pytest.mark.parametrize("d_pad,ld,ns,stages", SC.LOCKSTEP, ids=[_plan_id(c[0], c[1], c[2]) for c in SC.LOCKSTEP])
def test_lockstep_hint(cuda, d_pad, ld, ns, stages, sync_every):
    """The split lock-step hint at every stage, every second stage, the default and off,
    with splits of unequal length; twice into the same G gives G0 + 2 ref (the counter
    workspace is reset per launch)."""
    assert SC.launch_plan(d_pad, ld, ns)["stages"] == stages
    fm, ref = _case(cuda, d_pad, d_pad - 9, ld)
    _check_exact(fm, ref, num_splits=ns, sync_every=sync_every)
    _check_exact(fm, ref, calls=2, num_splits=ns, sync_every=sync_every)


# ------------------------------------------------------------------------ argument checks
def _raw_syrk(XT, ld, n, d_pad, G, ldg, variant=0):
    return _lib.kernels().harp_syrk_t_bf16(XT.data_ptr(), ld, n, d_pad, G.data_ptr(), ldg, 0, variant, None, 0,
                                           _lib.stream_ptr(G.device))


@pytest.mark.parametrize("what,ld,n,d_pad,ldg,variant", [
    ("d_pad-not-128k", 48, 48, 192, 256, 0),
    ("ld-not-48k", 72, 48, 128, 256, 0),
    ("n-not-48k", 96, 40, 128, 256, 0),
    ("ldg-below-d_pad", 48, 48, 256, 255, 0),
    ("variant-1", 48, 48, 128, 256, 1),
])
def test_bad_arguments_refused_before_launch(cuda, what, ld, n, d_pad, ldg, variant):
    XT = torch.ones((2, 256, 48), dtype=torch.bfloat16, device=cuda)
    G = torch.full((256, 256), SENTINEL, dtype=torch.float32, device=cuda)
    with pytest.raises(RuntimeError, match="bad argument"):
        _lib.check(_raw_syrk(XT, ld, n, d_pad, G, ldg, variant), "syrk_t")
    torch.cuda.synchronize()
    assert torch.equal(G, torch.full_like(G, SENTINEL))


def test_no_samples_leaves_g_untouched(cuda):
    XT = torch.ones((1, 128, 48), dtype=torch.bfloat16, device=cuda)
    G = torch.full((128, 128), SENTINEL, dtype=torch.float32, device=cuda)
    _lib.check(_raw_syrk(XT, 48, 0, 128, G, 128), "syrk_t")
    torch.cuda.synchronize()
    assert torch.equal(G, torch.full_like(G, SENTINEL))


# --------------------------------------------------------------------------- layout kernel
def _layout(X, n, d, ld, d_pad, ones_row):
    """``harp_to_feature_major_bf16`` as ``from_rows`` calls it, into an XT full of NaN."""
    XT = torch.full((ld // SC.KT, d_pad, SC.KT), float("nan"), dtype=torch.bfloat16, device=X.device)
    st = _lib.kernels().harp_to_feature_major_bf16(X.data_ptr(), n, d, X.stride(0), XT.data_ptr(), ld, d_pad,
                                                   ones_row, _lib.stream_ptr(X.device))
    _lib.check(st, "to_feature_major")
    return XT


def _same_bits(a, b):
    return torch.equal(a.view(torch.int16), b.view(torch.int16))  # a surviving NaN fails


def _real_rows(n, d, cuda):
    g = torch.Generator(device=cuda).manual_seed(n * 131 + d)
    return torch.randn(n, d, generator=g, device=cuda).to(torch.bfloat16)


@pytest.mark.parametrize("d", [1, 31, 32, 33, 127, 128])
@pytest.mark.parametrize("n", [1, 31, 32, 33, 47, 48, 49, 191, 192, 193])
def test_layout_kernel_writes_every_element(cuda, n, d):
    """n at the 32 (transpose tile) / 48 (sample block) / 192 (padding) edges, d at the 32
    and 128 edges; ld padded to 192 as from_rows does and to 48 only."""
    X = _real_rows(n, d, cuda)
    d_pad, ld192 = LA.FeatureMajor.dims(n, d)
    for ld in (ld192, (n + 47) // 48 * 48):
        assert _same_bits(_layout(X, n, d, ld, d_pad, d), SC.feature_major_ref(X, n, d, ld, d_pad))


def test_layout_kernel_row_stride(cuda):
    """X a column slice of a wider tensor: ldx > d."""
    n, d = 100, 33
    Xw = _real_rows(n, d + 9, cuda)
    X = Xw[:, 4:4 + d]
    assert X.stride(0) == d + 9
    d_pad, ld = LA.FeatureMajor.dims(n, d)
    assert _same_bits(_layout(X, n, d, ld, d_pad, d), SC.feature_major_ref(X.contiguous(), n, d, ld, d_pad))


def test_layout_kernel_ones_row_elsewhere(cuda):
    """ones_row beyond d but inside d_pad."""
    n, d, ones = 70, 20, 77
    X = _real_rows(n, d, cuda)
    d_pad, ld = LA.FeatureMajor.dims(n, d)
    assert _same_bits(_layout(X, n, d, ld, d_pad, ones), SC.feature_major_ref(X, n, d, ld, d_pad, ones_row=ones))


@pytest.mark.parametrize("n,d", [(193, 127), (49, 128)])
def test_from_rows_gram_stats_exact(cuda, n, d):
    X = SC.int_rows(n, d, seed=n + d, device=cuda)
    cnt, s, G = LA.gram_stats(LA.FeatureMajor.from_rows(X.float()))
    Xd = X.double()
    assert cnt.item() == n
    assert torch.equal(s, Xd.sum(0).float())
    assert torch.equal(G, (Xd.t() @ Xd).float())


@pytest.mark.parametrize("lo,hi", [(0.0, 1.0), (-1.0, 3.0)])
@pytest.mark.parametrize("d", [5, 127])
@pytest.mark.parametrize("n", [47, 48, 96 + 5])
def test_uniform_layout(cuda, n, d, lo, hi):
    fm = LA.FeatureMajor.uniform(n, d, lo, hi, seed=n + d, device=cuda)
    assert fm.XT.shape == (192 // SC.KT, 128, SC.KT)
    D = fm.dense().float()
    vals = D[:d, :n]
    assert bool((vals >= lo).all()) and bool((vals < hi).all()), (vals.min().item(), vals.max().item())
    assert vals.unique().numel() > 16  # random data, not a constant
    assert bool((D[d, :n] == 1).all())
    D[: d + 1, :n] = 0
    assert int((D != 0).sum()) == 0
    cnt, _, _ = LA.gram_stats(fm)
    assert cnt.item() == n


# ----------------------------------------------------------------------- real-valued data
@pytest.mark.parametrize("n,d", [(192 * 3, 127), (3120, 300), (6192, 1000)])
def test_real_valued_within_summation_bound(cuda, n, d):
    """Non-integer data against the any-order summation bound with u = 2^-23:
    |G - ref| <= (ld + 2) 2^-23 (|Xb|^T |Xb|) elementwise, ref in fp64 on the same
    bf16-rounded data. Measured worst error / bound on the MI355X: 6.4e-3 at (576, 127),
    2.4e-3 at (3120, 300), 8.7e-4 at (6192, 1000): the bound is a worst case that grows with
    ld, the measured error behaves like a few roundings."""
    g = torch.Generator(device=cuda).manual_seed(n + d)
    X = torch.rand(n, d, generator=g, device=cuda) * 4 - 1
    fm = LA.FeatureMajor.from_rows(X)
    G = LA.symmetrize_upper(LA.syrk_t(fm))
    ratio = SC.bound_ratio(G, X, fm.ld)
    print(f"syrk real-valued n={n} d={d}: worst error / bound = {ratio:.3e}")
    assert ratio <= 1.0
    assert int((G[d + 1:] != 0).sum()) == 0 and int((G[:, d + 1:] != 0).sum()) == 0
