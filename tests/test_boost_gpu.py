"""Native boosting kernels (``csrc/boost.hip``) against their torch mirror in
``harp_amd/ops/boost.py`` (run on CPU tensors), rounds through the forest split kernels, the
BrownBoost sums and t search, and GPU fits end to end.

Shapes: n in {1, 63, 257, 2049, 4097} (below a wave, past a block, past one and two 2048-row
chunks), d in {1, 7, 17, 33} (row padding to 16, more than one 16-byte segment), B in {2, 3,
256}, C in {2, 3, 32}. B * C * 8 bytes per feature decides the feature groups: 256 x 3 gives
10 features per group, 256 x 32 one.

Summation bound: an fp64 sum of m terms taken in any order differs from the exact sum by at
most m * 2**-53 * sum|x| to first order; two such sums differ by at most twice that.

Chosen split indices are never compared between a GPU run and an independent CPU run."""
import math

import pytest
import torch

from harp_amd.models import trees as T
from harp_amd.ops import _lib
from harp_amd.ops import boost as BO
from harp_amd.ops import forest as F

from tests.test_boost import make_boost_data

pytestmark = pytest.mark.gpu

# n, d, B, C
CLASS_SHAPES = [(1, 1, 2, 2), (63, 7, 3, 3), (257, 17, 256, 2), (2049, 33, 256, 32), (4097, 17, 256, 3),
                (4097, 33, 2, 32), (2049, 7, 3, 2)]
# n, d, B, K: 256 x 12 forces two class groups, 256 x 32 four; 2049 x 17 x 256 x 3 has 3 feature groups
LOGIT_SHAPES = [(1, 1, 2, 2), (63, 7, 3, 3), (257, 33, 256, 2), (2049, 17, 256, 3), (4097, 7, 256, 12),
                (2049, 3, 256, 32), (4097, 33, 2, 32)]
EPS = 2.0 ** -53


def _ids(s):
    return "x".join(map(str, s))


def _binned(n, d, B, C, seed):
    """Random bins and labels, with a few bins >= B (where B < 256) and labels outside [0, C)."""
    g = torch.Generator().manual_seed(seed)
    Xb = torch.zeros((n, F.padded_width(d)), dtype=torch.uint8)
    Xb[:, :d] = torch.randint(0, B, (n, d), generator=g).to(torch.uint8)
    y = torch.randint(0, C, (n,), generator=g).int()
    if n > 8:
        if B < 256:
            Xb[3::29, 0] = B
            Xb[5::31, d - 1] = 255
        y[1::37] = -1
        y[2::41] = C
    return Xb, y, g


def _stumps(d, C):
    """Previous stumps: none, one on feature 0, one on the last feature (outside group 0 when
    the features split into groups)."""
    return [(-1, 0, 0, 0), (0, 0, 1, 0), (d - 1, 1, C - 1, 0)]


@pytest.mark.parametrize("shape", CLASS_SHAPES, ids=_ids)
def test_class_round_exact(cuda, shape):
    n, d, B, C = shape
    Xb, y, g = _binned(n, d, B, C, 1)
    w = torch.randint(0, 16, (n,), generator=g).double()  # integer weights and multipliers: exact sums
    mul = torch.tensor([2.0, 3.0], dtype=torch.float64)
    for rec in _stumps(d, C):
        rec = torch.tensor(rec, dtype=torch.int32)
        wo = torch.empty(n, dtype=torch.float64)
        want = BO.class_round(Xb, y, w, wo, rec, mul, d, B, C)
        wg = torch.full((n,), -1.0, dtype=torch.float64, device=cuda)
        got = BO.class_round(Xb.to(cuda), y.to(cuda), w.to(cuda), wg, rec.to(cuda), mul.to(cuda), d, B, C)
        assert torch.equal(wg.cpu(), wo), rec
        assert torch.equal(got.cpu(), want), rec
        assert float(want.sum()) > 0 or n == 1


@pytest.mark.parametrize("shape", CLASS_SHAPES, ids=_ids)
def test_class_round_real_weights(cuda, shape):
    n, d, B, C = shape
    Xb, y, g = _binned(n, d, B, C, 2)
    w = torch.rand(n, generator=g, dtype=torch.float64) + 0.25
    mul = torch.tensor([0.7312, 1.9177], dtype=torch.float64)
    none = torch.tensor([-1, 0, 0, 0], dtype=torch.int32)
    for rec in _stumps(d, C):
        rec = torch.tensor(rec, dtype=torch.int32)
        wo = torch.empty(n, dtype=torch.float64)
        want = BO.class_round(Xb, y, w, wo, rec, mul, d, B, C)
        m = BO.class_round(Xb, y, torch.ones(n, dtype=torch.float64), torch.empty(n, dtype=torch.float64), none, mul,
                           d, B, C)  # rows per cell
        wg = torch.empty(n, dtype=torch.float64, device=cuda)
        got = BO.class_round(Xb.to(cuda), y.to(cuda), w.to(cuda), wg, rec.to(cuda), mul.to(cuda), d, B, C)
        assert torch.equal(wg.cpu(), wo), rec  # element-wise, contraction off
        assert bool(((got.cpu() - want).abs() <= 2 * m * EPS * want).all()), rec  # weights > 0: sum|x| = want


def test_class_round_brownboost_weights(cuda):
    n, d, B = 4097, 17, 256
    Xb, y, g = _binned(n, d, B, 2, 3)
    r = 0.5 * torch.randn(n, generator=g, dtype=torch.float64)
    scal = torch.tensor([0.8, 2.0], dtype=torch.float64)
    wo = torch.empty(n, dtype=torch.float64)
    want = BO.class_round(Xb, y, None, wo, None, None, d, B, 2, r=r, scal=scal)
    wg = torch.empty(n, dtype=torch.float64, device=cuda)
    got = BO.class_round(Xb.to(cuda), y.to(cuda), None, wg, None, None, d, B, 2, r=r.to(cuda), scal=scal.to(cuda))
    assert float(((wg.cpu() - wo).abs() / wo).max()) <= 1e-14  # exp: a few ulp between the libraries
    m = BO.class_round(Xb, y, torch.ones(n, dtype=torch.float64), torch.empty(n, dtype=torch.float64),
                       torch.tensor([-1, 0, 0, 0], dtype=torch.int32), torch.ones(2, dtype=torch.float64), d, B, 2)
    assert bool(((got.cpu() - want).abs() <= (2 * m * EPS + 1e-14) * want).all())


def test_shape_outside_the_limits_is_a_status(cuda):
    k = _lib.kernels()
    z = torch.zeros(64, dtype=torch.float64, device=cuda)
    Xb = torch.zeros((4, 16), dtype=torch.uint8, device=cuda)
    y = torch.zeros(4, dtype=torch.int32, device=cuda)
    s = _lib.stream_ptr(cuda)
    assert k.harp_boost_class_round(Xb.data_ptr(), 16, 4, y.data_ptr(), z.data_ptr(), z[8:].data_ptr(), y.data_ptr(),
                                    z.data_ptr(), None, None, 1, 257, 2, z.data_ptr(), s) == 3
    assert k.harp_boost_logit_round(Xb.data_ptr(), 16, 4, y.data_ptr(), z.data_ptr(), z[8:].data_ptr(), y.data_ptr(),
                                    z.data_ptr(), 4.0, 1, 2, 33, z.data_ptr(), None, s) == 3
    with pytest.raises(ValueError):
        BO._status(3, "x")
    with pytest.raises(ValueError):
        BO.class_round(Xb, y, z, z[8:], y, z, 1, 257, 2)


# ---------------------------------------------------------------- logit round
@pytest.mark.parametrize("shape", LOGIT_SHAPES, ids=_ids)
def test_logit_round(cuda, shape):
    n, d, B, K = shape
    Xb, y, g = _binned(n, d, B, K, 4)
    Fi = 8 * torch.rand((n, K), generator=g, dtype=torch.float64) - 4  # |F_out| <= 5 with |v| <= 0.5
    rec_i = torch.stack([torch.randint(-1, d, (K,), generator=g), torch.randint(0, max(B - 1, 1), (K,), generator=g)],
                        1).int()
    rec_i[0, 0] = d - 1
    rec_v = torch.rand((K, 2), generator=g, dtype=torch.float64) - 0.5
    Fo, wz = torch.empty_like(Fi), torch.empty((n, K, 2), dtype=torch.float64)
    BO.logit_round(Xb, y, Fi, Fo, rec_i, rec_v, 4.0, d, B, K, wz=wz)
    assert float(Fo.abs().max()) <= 5
    Fg = torch.empty_like(Fi, device=cuda)
    wzg = torch.empty((n, K, 2), dtype=torch.float64, device=cuda)
    Xg = Xb.to(cuda)
    H = BO.logit_round(Xg, y.to(cuda), Fi.to(cuda), Fg, rec_i.to(cuda), rec_v.to(cuda), 4.0, d, B, K, wz=wzg)
    for got, want in ((Fg.cpu(), Fo), (wzg.cpu(), wz)):  # 1e-9 relative; zeros get an absolute floor
        floor = torch.where(want == 0, 1e-12, 0.0)
        assert bool(((got - want).abs() <= 1e-9 * want.abs() + floor).all())
    # H against the histogram of the kernel's own (w, z); rows without a valid label add nothing
    w, z = wzg.cpu()[..., 0], wzg.cpu()[..., 1]
    want = BO.logit_hist(Xb, w, z, d, B, y)
    mag = BO.logit_hist(Xb, w, z.abs(), d, B, y)
    m = BO.logit_hist(Xb, torch.ones_like(w), torch.zeros_like(z), d, B, y)[..., :1]
    if n > 8:
        every = BO.logit_hist(Xb, torch.ones_like(w), torch.zeros_like(z), d, B, torch.zeros_like(y))[..., :1]
        assert float(every.sum()) > float(m.sum())  # the set holds such rows
    assert bool(((H.cpu() - want).abs() <= 2 * m * EPS * mag).all())
    # without the per-row output the histogram is built the same way
    H2 = BO.logit_round(Xg, y.to(cuda), Fi.to(cuda), Fg, rec_i.to(cuda), rec_v.to(cuda), 4.0, d, B, K)
    assert bool(((H2.cpu() - want).abs() <= 2 * m * EPS * mag).all())


# ---------------------------------------------------------------- rounds through the split kernels
def _first_max(H, task):
    g = F.ref_gain_table(H, task, 1.0, None)  # [M, d, B-1]
    M, d, nb = g.shape
    best, arg = F._first_max(g.reshape(M, d * nb))
    return best, arg // nb, arg % nb


def _counts(Xb, y, d, B, C):
    n = Xb.shape[0]
    return BO.class_round(Xb, y, torch.ones(n, dtype=torch.float64), torch.empty(n, dtype=torch.float64),
                          torch.tensor([-1, 0, 0, 0], dtype=torch.int32), torch.ones(2, dtype=torch.float64), d, B, C)


def test_adaboost_rounds_trace(cuda):
    n, d, K, B = 4097, 17, 3, 256
    X, y = make_boost_data(n, d, K)
    th = T._bins(X, B)
    Xb, yi = F.bin_features(X, th), y.int()
    steps = []
    T.AdaBoost(8, engine="native").fit(X.to(cuda), y.to(cuda), thresholds=th.to(cuda),
                                       trace=lambda t, s: steps.append({k: (v.cpu() if torch.is_tensor(v) else v)
                                                                        for k, v in s.items()}))
    assert len(steps) == 8
    m = _counts(Xb, yi, d, B, K)
    w = [torch.ones(n, dtype=torch.float64), torch.empty(n, dtype=torch.float64)]
    rec, mul = BO.new_class_state("cpu")
    for t, s in enumerate(steps):
        H = s["H"]
        best, f, b = _first_max(H, F.GINI)
        assert s["split"] == bool(best[0] > F.SPLIT_EPS) and (int(f[0]), int(b[0])) == (s["feature"], s["bin"])
        pre = F._ref_prefix(H)
        L, tot, Tt = pre[0, s["feature"], s["bin"]], pre[0, s["feature"], -1], pre[0, 0, -1]
        S = 0.0
        for c in range(K):
            S = S + float(Tt[c])
        err = 1.0 - (float(L.max()) + float((tot - L).max())) / S
        assert abs(err - s["err"]) <= 1e-12
        assert abs(math.log((1 - err) / max(err, 1e-12)) + math.log(K - 1) - s["alpha"]) <= 1e-12
        # replay: the GPU's stump and multipliers through the mirror's weight update
        want = BO.class_round(Xb, yi, w[t & 1], w[(t + 1) & 1], rec, mul, d, B, K)
        if t == 0:
            assert torch.equal(H, want)  # weights exactly 1.0
        assert bool(((H - want).abs() <= 2 * m * EPS * want).all()), t
        rec, mul = s["rec"], s["mul"]
        assert abs(float(w[(t + 1) & 1].sum()) - n) <= 1e-9 * n


def test_logitboost_rounds_trace(cuda):
    """Every class's split is the first maximum of the gain table of the GPU's own histogram;
    the histograms follow from the GPU's stumps by replay through the mirror. The per-row
    (w, z) of the two differ by the exp of the two libraries (1e-9 relative, as in
    test_logit_round), on top of the summation bound."""
    n, d, K, B = 4097, 17, 3, 256
    X, y = make_boost_data(n, d, K)
    th = T._bins(X, B)
    Xb, yi = F.bin_features(X, th), y.int()
    steps = []
    T.LogitBoost(5, engine="native").fit(X.to(cuda), y.to(cuda), thresholds=th.to(cuda),
                                         trace=lambda t, s: steps.append({k: v.cpu() for k, v in s.items()}))
    assert len(steps) == 5
    Fb = [torch.zeros((n, K), dtype=torch.float64), torch.empty((n, K), dtype=torch.float64)]
    rec_i, rec_v = BO.new_logit_state(K, "cpu")
    for t, s in enumerate(steps):
        H = s["H"]
        best, f, b = _first_max(H, F.MSE)
        assert torch.equal(s["split"].bool(), best > F.SPLIT_EPS)
        assert torch.equal(f.int(), s["feature"]) and torch.equal(b.int(), s["bin"])
        wz = torch.empty((n, K, 2), dtype=torch.float64)
        want = BO.logit_round(Xb, yi, Fb[t & 1], Fb[(t + 1) & 1], rec_i, rec_v, 4.0, d, B, K, wz=wz)
        mag = BO.logit_hist(Xb, wz[..., 0], wz[..., 1].abs(), d, B, yi)
        m = BO.logit_hist(Xb, torch.ones((n, K), dtype=torch.float64), torch.zeros((n, K), dtype=torch.float64), d,
                          B, yi)[..., :1]
        assert bool(((H - want).abs() <= (2 * m * EPS + 1e-9) * mag).all()), t
        rec_i, rec_v, _ = BO.logit_records(s["feature"], s["bin"], s["split"], s["L"], s["R"], s["T"])


# ---------------------------------------------------------------- BrownBoost sums and t search
def _brown_state(n, seed):
    g = torch.Generator().manual_seed(seed)
    r = 0.4 * torch.randn(n, generator=g, dtype=torch.float64)
    u = torch.where(torch.rand(n, generator=g, dtype=torch.float64) < 0.7, 1.0, -1.0).double()
    return r, u, g


@pytest.mark.parametrize("n", [1, 63, 4097])
@pytest.mark.parametrize("J", [1, 64])
def test_brown_sums(cuda, n, J):
    r, u, g = _brown_state(n, n + J)
    s, c = 0.9, 2.0
    scal = torch.tensor([s, c], dtype=torch.float64)
    # |z| / sqrt(c) stays below 2, so that no term 1 - erf(.) is itself a cancellation
    cand = torch.stack([0.5 * torch.rand(J, generator=g, dtype=torch.float64),
                        s * torch.rand(J, generator=g, dtype=torch.float64)], 1)
    z = r[:, None] + s - cand[None, :, 1] + cand[None, :, 0] * u[:, None]
    pot = (1 - torch.erf(z / math.sqrt(c))).sum(0)  # terms >= 0
    e = torch.exp(-z * z / c)
    cor = (e * u[:, None]).sum(0)
    got = BO.brown_sums(r.to(cuda), u.to(cuda), scal.to(cuda), cand.to(cuda))
    again = BO.brown_sums(r.to(cuda), u.to(cuda), scal.to(cuda), cand.to(cuda))
    assert torch.equal(got, again)
    for what, col in ((BO.POT, 0), (BO.COR, 1)):  # one sum alone: the same bits, the other one 0
        part = BO.brown_sums(r.to(cuda), u.to(cuda), scal.to(cuda), cand.to(cuda), what)
        assert torch.equal(part[:, col], got[:, col]) and not bool(part[:, 1 - col].any())
    got = got.cpu()
    assert bool(((got[:, 0] - pot).abs() <= 1e-12 * pot).all())
    assert bool(((got[:, 1] - cor).abs() <= 1e-12 * e.sum(0)).all())


def test_brown_t_search(cuda):
    n, c = 4097, 2.0
    r, u, _ = _brown_state(n, 7)
    pot = lambda z: float((1 - torch.erf(z / math.sqrt(c))).sum())

    def t_of(a, s):  # the torch engine's bisection
        target, lo, hi = pot(r + s), 0.0, s
        if pot(r + s - hi + a * u) <= target:
            return hi
        for _ in range(60):
            mid = 0.5 * (lo + hi)
            if pot(r + s - mid + a * u) < target:
                lo = mid
            else:
                hi = mid
        return 0.5 * (lo + hi)

    rg, ug = r.to(cuda), u.to(cuda)
    seen = set()
    for s, a in ((2.0, 0.3), (1.0, 0.05), (1.0, 1.5), (2e-3, 4.0)):
        scal = torch.tensor([s, c], dtype=torch.float64, device=cuda)
        target = BO.brown_sums(rg, ug, scal, torch.zeros((1, 2), dtype=torch.float64, device=cuda))[0, 0]
        t = float(BO.brown_t_search(rg, ug, scal, a, target)[4])
        want = t_of(a, s)
        seen.add(want == s)
        if want == s:
            assert t == s  # time runs out: exactly s
        else:
            assert abs(t - want) <= 1e-9 * s
    assert seen == {True, False}


# ---------------------------------------------------------------- end to end
def _acc(m, X, y):
    return float((m.predict(X) == y).double().mean())


def test_fits_end_to_end(cuda):
    n, d, K = 4097, 17, 3
    X, y = make_boost_data(n, d, K)
    Xg, yg = X.to(cuda), y.to(cuda)
    ada_c, ada_g = T.AdaBoost(20, engine="native").fit(X, y), T.AdaBoost(20, engine="native").fit(Xg, yg)
    assert _acc(ada_g, Xg, yg) >= _acc(ada_c, X, y) - 0.01
    assert _acc(ada_g, Xg, yg) > _acc(T.stump(Xg, yg, engine="native"), Xg, yg)
    lb_c, lb_g = T.LogitBoost(8, engine="native").fit(X, y), T.LogitBoost(8, engine="native").fit(Xg, yg)
    assert _acc(lb_g, Xg, yg) >= _acc(lb_c, X, y) - 0.01
    for m in (ada_g, lb_g):  # the packed-forest route against the per-learner loop
        assert float((m.decision(Xg) - m._decision_loop(Xg)).abs().max()) <= 1e-12
    yb, ybg = (y > 0).long(), (yg > 0).long()
    bb_c = T.BrownBoost(c=2.0, max_rounds=4, engine="native").fit(X, yb)
    bb_g = T.BrownBoost(c=2.0, max_rounds=4, engine="native").fit(Xg, ybg)
    assert len(bb_g.learners) == 4 and _acc(bb_g, Xg, ybg) >= _acc(bb_c, X, yb) - 0.01
