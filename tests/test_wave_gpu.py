"""The wave, row and block primitives of csrc/wave.h, one at a time (wave_test_kernel of
csrc/testutil.hip applies one primitive to the lanes it is given), against torch on the same
64-value rows.

Exact cases use values every summation order adds without rounding, and are compared with
torch.equal. The random rows use derived bounds: a sum of 64 terms in any order is within
64 * u * sum(|x|) of the exact sum (u = 2**-53 for fp64, 2**-24 for fp32), a product within
64 * u * prod(|x|); the exact references are math.fsum and a product of Fractions.

NaN: a NaN never replaces a number and a number never replaces a NaN (csrc/wave.h), so a lane
that enters an arg-reduction with a NaN hides whatever it would have passed on. Lane 40 is a
lane both forms read exactly once, as an original value and never as a carrier: the xor form's
lanes below 32 and the DPP form's uniform result are then the extremum of the other 63 lanes.
"""
import math
from fractions import Fraction

import pytest
import torch

from harp_amd.ops.testutil import wave_op

pytestmark = pytest.mark.gpu

EDGES = (0, 15, 16, 31, 32, 47, 48, 63)  # first and last lane of every 16-lane DPP row
INF = float("inf")
LANES = torch.arange(64)
SMALL = ((LANES * 37 + 11) % 23 - 11).double()  # integers in [-11, 11]
PERM = ((LANES * 29 + 5) % 64).int()  # a permutation of 0..63 (29 is odd)


def run(cuda, op, x, idx=None):
    x = torch.as_tensor(x, dtype=torch.float64).contiguous()
    idx = torch.arange(x.numel(), dtype=torch.int32) if idx is None else torch.as_tensor(idx, dtype=torch.int32)
    d, i = wave_op(op, x.to(cuda), idx.contiguous().to(cuda))
    return d.cpu(), i.cpu()


def spike(lane, base=3.0, val=7.0, n=64):
    x = torch.full((n,), base, dtype=torch.float64)
    x[lane] = val
    return x


def uniform(t, value):
    """every entry of t holds exactly `value` (bitwise for numbers)"""
    return torch.equal(t, torch.full_like(t, value))


def rows16(x, fn):
    """fn over each 16-lane row, broadcast back to the row's lanes"""
    return torch.stack([fn(r) for r in x.view(-1, 16)]).repeat_interleave(16)


def arg_ref(x, idx, maximum):
    """extremum of the numbers of x and the lowest index that holds it"""
    ok = ~torch.isnan(x)
    m = x[ok].max() if maximum else x[ok].min()
    return float(m), int(idx[ok & (x == m)].min())


EXACT_ROWS = [SMALL, SMALL.abs(), torch.zeros(64, dtype=torch.float64), torch.full((64,), 5.0, dtype=torch.float64)] + [
    spike(lane) for lane in EDGES] + [spike(lane, 3.0, -7.0) for lane in EDGES]


def test_wave_reductions_exact(cuda):
    for x in EXACT_ROWS:
        s, mx, mn = float(x.sum()), float(x.max()), float(x.min())
        for op, want in (("wave_sum", s), ("wave_sum_d", s), ("wave_sum_d_dpp", s), ("wave_sum_rows", s),
                         ("wave_total", s), ("wave_max_d", mx), ("wave_max_f", mx), ("wave_min_d", mn),
                         ("wave_min_f", mn), ("wave_min_d_dpp", mn)):
            assert uniform(run(cuda, op, x)[0], want), (op, x)
        assert torch.equal(run(cuda, "wave_scan_incl", x)[0], x.cumsum(0)), x
        assert torch.equal(run(cuda, "sub16_sum", x)[0], rows16(x, torch.sum)), x
        assert torch.equal(run(cuda, "row_min_d", x)[0], rows16(x, torch.min)), x
        if mn >= 0:  # the order of the bit patterns is the order of the values
            assert uniform(run(cuda, "wave_min_u64", x)[0], mn), x


def test_wave_product_exact(cuda):
    for lane in EDGES:  # powers of two multiply without rounding in any order
        x = torch.tensor([2.0, 0.5] * 32, dtype=torch.float64)
        x[lane] *= -4.0
        assert uniform(run(cuda, "wave_prod_d", x)[0], -4.0), lane


def test_int_sum_with_negative_values(cuda):
    for v in ((LANES * 37) % 41 - 20, (LANES % 3 - 1) * (1 << 20), -LANES - 1):
        out = run(cuda, "wave_sum_i", torch.zeros(64), v.int())[1]
        assert uniform(out, int(v.sum())), v


def test_scan_and_total_on_integers_below_2_24(cuda):
    for x in (((LANES * 13) % 50).double(), ((LANES * 7919) % (1 << 17)).double(), spike(63, 0.0, float((1 << 24) - 1))):
        assert float(x.sum()) < 2 ** 24
        assert torch.equal(run(cuda, "wave_scan_incl", x)[0], x.cumsum(0))
        assert uniform(run(cuda, "wave_total", x)[0], float(x.sum()))


def test_readlane_every_row_edge(cuda):
    x = SMALL * 0.5 + LANES.double() * 64  # all different
    for src in EDGES:
        assert uniform(run(cuda, "readlane_d", x, torch.full((64,), src))[0], float(x[src])), src


def test_infinities(cuda):
    for lane in EDGES:
        hi, lo = spike(lane, 3.0, INF), spike(lane, 3.0, -INF)
        for op in ("wave_max_d", "wave_max_f"):
            assert uniform(run(cuda, op, hi)[0], INF) and uniform(run(cuda, op, lo)[0], 3.0)
        for op in ("wave_min_d", "wave_min_f", "wave_min_d_dpp"):
            assert uniform(run(cuda, op, lo)[0], -INF) and uniform(run(cuda, op, hi)[0], 3.0)
        for op in ("wave_sum", "wave_sum_d", "wave_sum_d_dpp", "wave_sum_rows"):
            assert uniform(run(cuda, op, hi)[0], INF) and uniform(run(cuda, op, lo)[0], -INF)
        for op, x, want in (("wave_argmax_xor", hi, INF), ("wave_argmax_dpp", hi, INF), ("wave_argmin_xor", lo, -INF),
                            ("wave_argmin_dpp", lo, -INF)):
            d, i = run(cuda, op, x, PERM)
            assert uniform(d, want) and uniform(i, int(PERM[lane])), (op, lane)


def arg_cases():
    """(values, indices) rows for the arg-reductions"""
    out = [(SMALL, PERM), (SMALL, LANES.int())]
    out += [(spike(lane), PERM) for lane in EDGES] + [(spike(lane, 3.0, -7.0), PERM) for lane in EDGES]
    for a, b in ((17, 40), (63, 0)):  # two equal extrema: the lower INDEX wins, whatever its lane
        for val in (100.0, -100.0):
            x = SMALL.clone()
            x[a] = x[b] = val
            out += [(x, PERM), (x, PERM.flip(0)), (x, LANES.int())]
    return out


@pytest.mark.parametrize("maximum", [True, False])
def test_arg_reductions_tie_rule(cuda, maximum):
    sfx = "max" if maximum else "min"
    for x, idx in arg_cases():
        v, i = arg_ref(x, idx, maximum)
        for op in ("wave_arg%s_xor" % sfx, "wave_arg%s_dpp" % sfx):
            d, k = run(cuda, op, x, idx)
            assert uniform(d, v) and uniform(k, i), (op, x, idx)
        d, k = run(cuda, "row_arg" + sfx, x, idx)
        want = [arg_ref(x[r:r + 16], idx[r:r + 16], maximum) for r in range(0, 64, 16)]
        assert torch.equal(d, torch.tensor([w[0] for w in want], dtype=torch.float64).repeat_interleave(16))
        assert torch.equal(k, torch.tensor([w[1] for w in want], dtype=torch.int32).repeat_interleave(16))


@pytest.mark.parametrize("maximum", [True, False])
def test_arg_reductions_all_equal_give_index_zero(cuda, maximum):
    sfx = "max" if maximum else "min"
    x = torch.full((64,), 2.5, dtype=torch.float64)
    for idx in (LANES.int(), PERM, PERM.flip(0)):
        for op in ("wave_arg%s_xor" % sfx, "wave_arg%s_dpp" % sfx):
            d, k = run(cuda, op, x, idx)
            assert uniform(d, 2.5) and uniform(k, 0), (op, idx)


@pytest.mark.parametrize("maximum", [True, False])
def test_arg_reductions_one_nan_among_numbers(cuda, maximum):
    sfx = "max" if maximum else "min"
    for base in (SMALL, spike(41, 3.0, 7.0 if maximum else -7.0), spike(8, 3.0, 7.0 if maximum else -7.0)):
        x = base.clone()
        x[40] = float("nan")  # see the module docstring for the lane
        v, i = arg_ref(x, PERM, maximum)
        d, k = run(cuda, "wave_arg%s_xor" % sfx, x, PERM)
        assert uniform(d[:32], v) and uniform(k[:32], i), base
        d, k = run(cuda, "wave_arg%s_dpp" % sfx, x, PERM)
        assert uniform(d, v) and uniform(k, i), base


@pytest.mark.parametrize("nwaves", [4, 16])
def test_block_reductions(cuda, nwaves):
    n = 64 * nwaves
    t = torch.arange(n)
    perm = ((t * 29 + 5) % n).int()
    small = ((t * 37 + 11) % 23 - 11).double()
    rows = [small, small.abs(), torch.zeros(n, dtype=torch.float64)]
    rows += [spike(lane, 3.0, 7.0, n) for lane in (0, 63, 64, n - 64, n - 1)]
    for x in rows:
        for op in ("block_sum_d", "block_sum_d_pre"):
            assert uniform(run(cuda, op, x)[0], float(x.sum())), (op, x)
        # block_max_d_pre reduces magnitudes: it starts from 0
        assert uniform(run(cuda, "block_max_d_pre", x.abs())[0], float(x.abs().max())), x
    ties = small.clone()
    ties[17] = ties[n - 24] = 100.0
    ties[63] = ties[64] = -100.0
    for x, idx in [(r, perm) for r in rows] + [(ties, perm), (ties, perm.flip(0)), (ties, t.int())]:
        for op, maximum in (("block_argmax", True), ("block_argmin", False)):
            v, i = arg_ref(x, idx, maximum)
            d, k = run(cuda, op, x, idx)
            assert uniform(d, v) and uniform(k, i), (op, x, idx)


def test_random_rows_within_derived_bounds(cuda):
    g = torch.Generator().manual_seed(7)
    x64 = torch.randn(64, generator=g, dtype=torch.float64) * 1e3
    x32 = (torch.randn(64, generator=g, dtype=torch.float32) * 1e3).double()  # fp32 values, held exactly
    for x, u, xor_op, dpp_op in ((x64, 2.0 ** -53, "wave_sum_d", "wave_sum_d_dpp"), (x32, 2.0 ** -24, "wave_sum", "wave_sum_rows")):
        exact, tol = math.fsum(x.tolist()), 64 * u * float(x.abs().sum())
        a, b = run(cuda, xor_op, x)[0], run(cuda, dpp_op, x)[0]
        print(f"{xor_op}: max error {float((a - exact).abs().max()):.3e}, {dpp_op}: {float((b - exact).abs().max()):.3e}, "
              f"forms differ by {float((a - b).abs().max()):.3e}, bound {tol:.3e}")
        assert float((a - exact).abs().max()) <= tol and float((b - exact).abs().max()) <= tol
        assert float((a - b).abs().max()) <= tol  # the shuffle form and the DPP form agree
        if dpp_op == "wave_sum_d_dpp":
            assert uniform(b, float(b[0]))  # one fixed order of steps: the same bits in every lane
    tol, v = 64 * 2.0 ** -24 * float(x32.abs().sum()), x32.tolist()
    row = torch.tensor([math.fsum(v[r:r + 16]) for r in range(0, 64, 16)], dtype=torch.float64).repeat_interleave(16)
    assert float((run(cuda, "sub16_sum", x32)[0] - row).abs().max()) <= tol
    pre = torch.tensor([math.fsum(v[:k + 1]) for k in range(64)], dtype=torch.float64)
    assert float((run(cuda, "wave_scan_incl", x32)[0] - pre).abs().max()) <= tol
    p = torch.rand(64, generator=g, dtype=torch.float64) * 1.5 + 0.5  # [0.5, 2]
    exact = Fraction(1)
    for v in p.tolist():
        exact *= Fraction(v)
    out = run(cuda, "wave_prod_d", p)[0]
    err = max(abs(Fraction(v) - exact) for v in out.tolist())
    print(f"wave_prod_d: max error {float(err):.3e}, bound {64 * 2.0 ** -53 * float(exact):.3e}")
    assert err <= Fraction(64 * 2.0 ** -53) * exact
    for nwaves in (4, 16):  # a sum of 64 * nwaves terms: the bound grows with the count
        x = torch.randn(64 * nwaves, generator=g, dtype=torch.float64) * 1e3
        exact, tol = math.fsum(x.tolist()), 64 * nwaves * 2.0 ** -53 * float(x.abs().sum())
        for op in ("block_sum_d", "block_sum_d_pre"):
            out = run(cuda, op, x)[0]
            assert uniform(out, float(out[0])) and abs(float(out[0]) - exact) <= tol, op
