"""csrc/pqr.hip and ``stats.pivoted_qr(engine="native")`` on the GPU against scipy / numpy fp64.

Widths: every register width of the wave form (1, 7, 8 | 9 | 33 | 64), both sides of the form
boundary (64, 65), a padded workgroup width (96) and the LDS limit (128). Rows: one TSQR block
(n = d), one block plus a row (257), a two-level tree (1000). Inputs and bounds are those of
tests/test_pqr.py.
"""
import numpy as np
import pytest
import torch

from harp_amd.models import stats as ST
from harp_amd.ops import pqr as PQ

from tests.test_pqr import check_invariants, check_planted, exact_ties, planted, rank_deficient
from tests.test_reference_fixtures import rel

pytestmark = pytest.mark.gpu

WIDTHS = (1, 7, 8, 9, 33, 64, 65, 96, 128)


@pytest.mark.parametrize("rows", ("d", 257, 1000))
@pytest.mark.parametrize("d", WIDTHS)
def test_planted_order(d, rows):
    X, pi, dg = planted(d, d if rows == "d" else rows)
    check_planted(X, pi, dg, ST.pivoted_qr(X.cuda(), engine="native"))


@pytest.mark.parametrize("d", WIDTHS[1:])
def test_rank_deficient(d):
    X = rank_deficient(d)
    out = ST.pivoted_qr(X.cuda(), engine="native")
    assert out["Q"].is_cuda and out["R"].is_cuda and out["permutation"].is_cuda
    check_invariants(X, out, rank=d // 2)


@pytest.mark.parametrize("ties", (False, True))
@pytest.mark.parametrize("d", WIDTHS)
def test_kernel_equals_mirror_and_repeats(d, ties):
    A = exact_ties(d) if ties else planted(d, d)[0]
    Qm, Rm, pm = PQ.qrcp_small(A)
    first = PQ.qrcp_small(A.cuda())
    again = PQ.qrcp_small(A.cuda())
    assert all(torch.equal(a, b) for a, b in zip(first, again))
    Q, R, perm = (t.cpu() for t in first)
    assert perm.dtype == torch.int32 and torch.equal(perm, pm)
    assert rel(R, Rm) <= 1e-12 and rel(Q, Qm) <= 1e-12
    assert np.abs(np.tril(R.numpy(), -1)).max() == 0
