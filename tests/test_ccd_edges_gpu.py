"""MF-CCD HIP kernels (csrc/ccd.hip) at every path boundary against the fp64 CPU phase:
fp32 W and every residual, per row class, within the tolerances of tests/mf_cases.py (four
times the fp32 rounding error of the CPU formulation of the same phase, never anything
measured on a kernel). tests/test_mf_cases.py shows that a dropped border nonzero or a
skipped residual update sits at >= 4 of these tolerances in every case used here.

The lockstep grid cap (65,536 chunks) would need 2.7e8 nonzeros and is out of scope. A
residual launch past its 65,536 x 256-thread grid cap needs 1.7e7 nonzeros, whose transfer
and CPU reference alone take over a second, so that one is left out as well."""
import pytest
import torch

from harp_amd.ops import ccd as C
from tests import mf_cases as MC

pytestmark = pytest.mark.gpu

KEYS = MC.all_ccd_case_keys()


def _dev(case, cuda):
    d = lambda x: x.to(cuda).contiguous()
    return d(case.rows), d(case.cols), d(case.ptr), d(case.res0), d(case.W0), d(case.H)


def _check(name, case, ref, W0, Wg, rg):
    torch.cuda.synchronize()
    ratios = MC.ccd_compare(case, ref, Wg, rg)
    for c, (rw, rr) in ratios.items():
        print(f"MFRATIO {name} {c} W {rw:.3f} res {rr:.3f}")
    empty = case.lens == 0
    assert torch.equal(Wg.cpu()[empty], W0[empty])  # empty rows: bit-identical
    return ratios


def _run(name, cuda, plan_of=None):
    case, ref = MC.ccd_reference(*KEYS[name])
    rows, cols, ptr, res, W, H = _dev(case, cuda)
    assert MC.class_limits() == (C.LONG_ROW, C.block_max(), C.block_max(True))
    plan = plan_of(ptr) if plan_of else None
    for _ in range(case.phases):
        C.phase(rows, ptr, cols, res, W, H, case.lam, plan)
    _check(name, case, ref, case.W0, W, res)
    return case, ref, W, res, plan


@pytest.mark.parametrize("lam", MC.BOUNDARY_LAMS)
@pytest.mark.parametrize("k", MC.BOUNDARY_KS)
def test_path_boundaries(cuda, k, lam):
    """Rows of 0 .. 20481 nonzeros on both sides of every path limit in one matrix: the wave,
    mid, wide and lockstep kernels each own the rows next to their limits."""
    case, ref, W, res, _ = _run(f"boundary-k{k}-lam{lam}", cuda)
    plan = C.RowPlan(case.ptr.to(cuda))
    lim = MC.class_limits()
    lens = case.lens
    assert sorted(lens[plan.mid.cpu().long()].tolist()) == sorted(n for n in MC.BOUNDARY_LENS if lim[0] < n <= lim[1])
    assert sorted(lens[plan.wide.cpu().long()].tolist()) == sorted(n for n in MC.BOUNDARY_LENS if lim[1] < n <= lim[2])
    longs = [n for n in MC.BOUNDARY_LENS if n > lim[2]]
    assert plan.n_long == len(longs) >= 3 and plan.chunks.shape[0] == sum(-(-n // C.CHUNK) for n in longs)
    assert int((plan.chunks[:, 2] - plan.chunks[:, 1]).min()) == 1  # the one-element chunk


@pytest.mark.parametrize("k", MC.LOCK_SMALL_KS)
def test_lockstep_small_rows(cuda, k):
    """RowPlan(block_rows=False): rows of 257, 4095, 4096, 4097 and 8193 nonzeros run through
    ccd_lockstep_kernel (ring acc[t % 3] wraps at k < 3, k = 3 and k > 3)."""
    case, ref, W, res, plan = _run(f"lockstep-k{k}", cuda, lambda ptr: C.RowPlan(ptr, block_rows=False))
    assert plan.n_long == 5 and plan.mid.numel() == 0 and plan.wide.numel() == 0
    assert float(plan.acc.abs().max()) == 0.0  # the ring is left clear for the next phase


@pytest.mark.parametrize("name,block_rows", [("reuse-k3", False), ("reuse-boundary-k4", True)])
def test_plan_reuse(cuda, name, block_rows):
    """Two phases with one plan (its acc and hbuf reused) equal two reference phases."""
    case, ref, W, res, plan = _run(name, cuda, lambda ptr: C.RowPlan(ptr, block_rows=block_rows))
    assert plan.hbuf.numel() == res.numel()


@pytest.mark.parametrize("k", [4, 5])
def test_only_short_rows(cuda, k):
    """No long row: skip_long = 0 and the 256-nonzero rows take the register path."""
    case, ref, W, res, plan = _run(f"short-k{k}", cuda, lambda ptr: C.RowPlan(ptr))
    assert plan.n_long == 0 and plan.mid.numel() == 0 and plan.wide.numel() == 0 and int(case.lens.max()) == C.LONG_ROW


@pytest.mark.parametrize("k,t", MC.ZERO_DIM_CASES)
def test_zero_denominator_keeps_w(cuda, k, t):
    """lam = 0 and an all-zero dimension t of the other factor: D = 0, so W[:, t] comes back
    bit-identical on every path, and every residual equals the reference's."""
    case, ref, W, res, _ = _run(f"zero-k{k}-t{t}", cuda)
    assert torch.equal(W[:, t].cpu(), case.W0[:, t])
    assert torch.equal(ref.W64[:, t], case.W0[:, t].double())


def test_grid_stride_wave_rows(cuda):
    """70,000 rows: more than the 65,536 waves of the capped ccd_phase_kernel grid."""
    case, _, _, _, _ = _run("stride-wave", cuda)
    assert case.lens.numel() > 16384 * 4


def test_grid_stride_block_rows(cuda):
    """8,200 rows of 257 nonzeros: more than the 8,192-block cap of harp_ccd_block."""
    case, _, _, _, plan = _run("stride-block", cuda, lambda ptr: C.RowPlan(ptr))
    assert plan.mid.numel() == 8200 > 8192


def test_long_rows_of_plan(cuda):
    """The plan as the models build it (long_rows_of), passed in explicitly."""
    name = "boundary-k3-lam0.05"
    case, ref = MC.ccd_reference(*KEYS[name])
    rows, cols, ptr, res, W, H = _dev(case, cuda)
    C.phase(rows, ptr, cols, res, W, H, case.lam, C.long_rows_of(ptr))
    _check(name, case, ref, case.W0, W, res)


@pytest.mark.parametrize("inplace", [False, True])
@pytest.mark.parametrize("nnz", [1, 255, 256, 257, 70001])
@pytest.mark.parametrize("k", [1, 3, 4, 5, 8, 37])
def test_residual_exact(cuda, k, nnz, inplace):
    """Integer-valued factors and ratings: ccd_residual_kernel is exact against fp64, also
    when it writes over its own input (out is val), as the rotation mode calls it."""
    rows, cols, val, Fr, Fc, want = MC.residual_exact_case(nnz, k)
    d = lambda x: x.to(cuda).contiguous()
    vg = d(val)
    canary = torch.full((nnz + 64,), 7.5, device=cuda)
    out = vg if inplace else canary[:nnz]
    got = C.residual(d(rows), d(cols), vg, d(Fr), d(Fc), out)
    torch.cuda.synchronize()
    assert got is out
    assert torch.equal(got.cpu().double(), want)
    if not inplace:
        assert torch.equal(vg.cpu(), val) and bool((canary[nnz:] == 7.5).all())
