"""csrc/jsvd.hip and ``stats.svd(engine="native")`` on the GPU against numpy fp64 and mpmath.

Widths: every register width of the wave form (1, 7, 8 | 9 | 33 | 64), both sides of the form
boundary (64, 65), a padded workgroup width (96) and the limit (128); odd widths exercise the
bye slot of the tournament. Rows: one block (n = d), one block plus a row (257), a two-level
tree (1000). Inputs and the 1e-12 bound are those of tests/test_svd_native.py.

Relative accuracy: on the column-graded ``B D`` theory gives c d eps cond(B) for every
singular value, a few 1e-15 at cond(B) = 2, so all of them (they span 2^-40 = 9e-13 of the
largest) are held to 1e-12 of their own size against a 50-digit mpmath SVD.
"""
import mpmath
import numpy as np
import pytest
import torch

from harp_amd.models import stats as ST
from harp_amd.ops import jsvd as JS

from tests.test_svd_native import TOL, block, check_factors, check_svd, graded, rank_deficient

pytestmark = pytest.mark.gpu

WIDTHS = (1, 7, 8, 9, 33, 64, 65, 96, 128)


def factor_t(d):
    """M = R^T of a random block, as stats.svd hands it to the kernel."""
    return torch.linalg.qr(block(2 * d + 3, d, seed=d), mode="r")[1].t().contiguous()


@pytest.mark.parametrize("want_w", (True, False))
@pytest.mark.parametrize("d", WIDTHS)
def test_kernel_invariants_repeat_and_mirror(d, want_w):
    M = factor_t(d)
    first = JS.svd_small(M.cuda(), want_w=want_w)
    again = JS.svd_small(M.cuda(), want_w=want_w)
    assert all(a is b is None or torch.equal(a, b) for a, b in zip(first, again))
    Z, s, W, sweeps = first
    assert (W is None) == (not want_w) and 0 < int(sweeps) <= JS.MAX_SWEEPS
    # M = Z S W^T: Z in the place of U and W^T in that of V^T; without W, Z^T Z = I is what is left
    check_factors(M, Z if want_w else None, s, W.t() if want_w else Z.t())
    sm = JS.svd_small(M, want_w=False)[1]
    assert (s.cpu() - sm).abs().max() <= TOL * sm[0]


@pytest.mark.parametrize("d", (9, 33, 65))
def test_relative_accuracy_on_a_graded_matrix(d):
    M = graded(d)
    s = JS.svd_small(M.cuda(), want_w=False)[1].cpu().numpy()
    mpmath.mp.dps = 50
    ref = mpmath.svd_r(mpmath.matrix(M.tolist()), compute_uv=False)
    ref = np.array(sorted((float(x) for x in ref), reverse=True))
    err = np.abs(s - ref) / ref
    print(f"d={d}: max relative error {err.max():.3e}, s[-1]/s[0] = {ref[-1] / ref[0]:.3e}")
    assert err.max() <= TOL


@pytest.mark.parametrize("rows", ("d", 257, 1000))
@pytest.mark.parametrize("d", (9, 64, 128))
def test_svd_end_to_end(d, rows):
    n = d if rows == "d" else rows
    X = block(n, d, seed=d + 1).cuda()
    ST.svd(X, engine="native")  # library workspaces are allocated by now
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    out = ST.svd(X, engine="native")
    torch.cuda.synchronize()
    assert all(v.is_cuda for v in out.values())
    if n == 1000:  # no [n, n]-sized temporary
        assert torch.cuda.max_memory_allocated() - before < n * n * 8
    check_svd(X, out)


@pytest.mark.parametrize("d", (9, 64, 128))
def test_svd_rank_deficient(d):
    X = rank_deficient(d)
    out = ST.svd(X.cuda(), engine="native")
    assert all(v.is_cuda for v in out.values())
    check_svd(X, out, rank=d // 2)
