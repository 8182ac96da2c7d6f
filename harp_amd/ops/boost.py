"""Boosting rounds on binned rows (``csrc/boost.hip``): decision stump, AdaBoost (SAMME),
LogitBoost and the BrownBoost line search. The features are binned once per fit
(:func:`harp_amd.ops.forest.bin_features`); a round is one pass over the binned rows that
applies the previous round's learner (weight multipliers, or the K centred regression stumps)
and accumulates the root histogram, followed by the forest engine's split kernels
(:func:`harp_amd.ops.forest.split_feature` / ``split_node``) on that histogram.

HIP tensors run the kernels (mandatory: a missing library raises). CPU tensors run the torch
mirror of the same algorithm in this module: the gloo path and the oracle of the GPU tests.
The per-row outputs (``w_out``, ``F_out``) of the class round are element-wise and equal the
mirror bit for bit; fp64 histogram cells depend on the order of the adds in the last bits.

Limits are those of the forest engine (``n_bins <= 256``, classes ``<= 32``); outside them
the launchers return status 3 and the wrappers raise ``ValueError``.

Everything a round needs from the previous split stays on the device (stump record,
multipliers); :func:`ada_fit` reads one small record per round for the stop tests,
:func:`logit_fit` reads nothing until the end.

Reference hot loops: DAAL ``stump`` / ``adaboost`` / ``logitboost`` / ``brownboost`` training
(ml/daal daal_stump, daal_adaboost, daal_logitboost, daal_brownboost).
"""
from __future__ import annotations

import math
from typing import Callable, List, Optional, Tuple

import torch

from . import _lib
from . import forest as F

_P, _I, _L, _D = _lib.c_void_p, _lib.c_int, _lib.c_long, _lib.c_double

_lib.register({
    # Xb, dpad, n, y, w_in, w_out, rec, mul, r, scal, d, B, C, H, stream
    "harp_boost_class_round": [_P, _I, _L, _P, _P, _P, _P, _P, _P, _P, _I, _I, _I, _P, _P],
    # Xb, dpad, n, y, w_in, w_out, rec, mul, d, stream
    "harp_boost_class_update": [_P, _I, _L, _P, _P, _P, _P, _P, _I, _P],
    # bf, bb, sp, L, R, T, C, n, rec, mul, info, stream
    "harp_boost_class_finish": [_P, _P, _P, _P, _P, _P, _I, _D, _P, _P, _P, _P],
    # Xb, dpad, n, y, F_in, F_out, rec_i, rec_v, zmax, d, B, K, H, wz, stream
    "harp_boost_logit_round": [_P, _I, _L, _P, _P, _P, _P, _P, _D, _I, _I, _I, _P, _P, _P],
    # n -> number of partial blocks
    "harp_boost_brown_blocks": [_L],
    # r, u, n, scal, cand, J, what, part, out, stream
    "harp_boost_brown_sums": [_P, _P, _L, _P, _P, _I, _I, _P, _P, _P],
    # sums, srch, a, cand, pass, stream
    "harp_boost_brown_step": [_P, _P, _D, _P, _I, _P],
})

CHUNK = 2048  # rows per round workgroup (BOOST_CHUNK in csrc/boost.hip)
MAX_CAND = 64  # candidates of one brown_sums pass = section width of the t search
T_PASSES = 10  # 64**10 = 2**60: the width 60 bisection steps reach
INFO = 8  # info = (split, feature, bin, left class, right class, err, alpha, S, L[C], R[C])


def _status(st: int, what: str) -> None:
    if st == 3:
        raise ValueError(f"{what}: shape outside the limits of the native boosting engine "
                         f"(n_bins <= {F.MAX_BINS}, classes <= {F.MAX_CLASSES})")
    _lib.check(st, what)


def _aligned(Xb: torch.Tensor) -> torch.Tensor:
    Xb = Xb.contiguous()
    return Xb if Xb.data_ptr() % 16 == 0 else Xb.clone()


# ---------------------------------------------------------------- class round
def new_class_state(device) -> Tuple[torch.Tensor, torch.Tensor]:
    """(stump record (feature, bin, left class, right class) with feature = -1, multipliers
    (mul_hit, mul_miss) = 1): the state before round 0."""
    return (torch.tensor([-1, 0, 0, 0], dtype=torch.int32, device=device),
            torch.ones(2, dtype=torch.float64, device=device))


def class_round(Xb, y, w_in, w_out, rec, mul, d: int, B: int, C: int, r=None, scal=None) -> torch.Tensor:
    """Root histogram [1, d, B, C] fp64 of the updated weights, which are stored to ``w_out``:
    ``w = w_in * (miss ? mul[1] : mul[0])`` with ``miss = ((Xb[row, f] > bin ? right : left) !=
    y[row])`` for the stump ``rec = (f, bin, left, right)``; ``f < 0``: ``w = w_in``. With ``r``
    (BrownBoost) ``w = exp(-(r + scal[0])**2 / scal[1])`` instead and ``w_out`` may be None. A
    row whose bin is >= B or whose label is outside [0, C) adds nothing."""
    F.check_shape(B, C)
    n = Xb.shape[0]
    dev = Xb.device
    if not _lib.use_native(Xb):
        yl = y.long()
        if r is not None:
            q = r + scal[0]
            w = torch.exp((-(q * q)) / scal[1])
        else:
            f = int(rec[0])
            if f >= d:
                f = -1
            w = w_in.clone()
            if f >= 0:
                pred = torch.where(Xb[:, f].long() > int(rec[1]), int(rec[3]), int(rec[2]))
                w = w_in * torch.where(pred != yl, mul[1], mul[0])
        if w_out is not None:
            w_out.copy_(w)
        bins = Xb[:, :d].long()
        ok = ((yl >= 0) & (yl < C))[:, None] & (bins < B)
        idx = (torch.arange(d)[None, :] * B + bins) * C + yl[:, None]
        H = torch.zeros(d * B * C, dtype=torch.float64)
        H.index_add_(0, idx[ok], w[:, None].expand(-1, d)[ok])
        return H.view(1, d, B, C)
    Xb = _aligned(Xb)
    H = torch.zeros((1, d, B, C), dtype=torch.float64, device=dev)
    st = _lib.kernels().harp_boost_class_round(
        Xb.data_ptr(), Xb.shape[1], n, y.data_ptr(), _lib.ptr(w_in), _lib.ptr(w_out), _lib.ptr(rec), _lib.ptr(mul),
        _lib.ptr(r), _lib.ptr(scal), d, B, C, H.data_ptr(), _lib.stream_ptr(dev))
    _status(st, "boost_class_round")
    return H


def class_update(Xb, y, w_in, w_out, rec, mul, d: int) -> None:
    """The weight update of :func:`class_round` alone (the unfused A/B of the benchmark)."""
    if not _lib.use_native(Xb):
        class_round(Xb, y, w_in, w_out, rec, mul, d, 1, 1)
        return
    st = _lib.kernels().harp_boost_class_update(Xb.data_ptr(), Xb.shape[1], Xb.shape[0], y.data_ptr(), w_in.data_ptr(),
                                                w_out.data_ptr(), rec.data_ptr(), mul.data_ptr(), d,
                                                _lib.stream_ptr(Xb.device))
    _status(st, "boost_class_update")


def class_finish(bf, bb, sp, L, R, T, n: float, rec, mul) -> torch.Tensor:
    """From ``split_node``'s outputs of the root: writes the next round's stump record ``rec``
    (feature -1 if the root does not split; leaf classes = first arg-max of L and R) and
    multipliers ``mul`` in place and returns ``info`` [8 + 2 C] fp64 = (split, feature, bin,
    left class, right class, err, alpha, S, L, R) with ``err = 1 - (max L + max R) / S``,
    ``S = sum T``, ``alpha = log((1 - err) / max(err, 1e-12)) + log(C - 1)``,
    ``mul_hit = n / (S ((1 - err) + err e^alpha))``, ``mul_miss = mul_hit e^alpha``."""
    C = L.shape[1]
    dev = L.device
    info = torch.empty(INFO + 2 * C, dtype=torch.float64, device=dev)
    if not _lib.use_native(L):
        Ls, Rs, Ts = L[0].tolist(), R[0].tolist(), T[0].tolist()
        S, mL, mR, lc, rc = 0.0, Ls[0], Rs[0], 0, 0
        for c in range(C):
            S = S + Ts[c]
            if Ls[c] > mL:
                mL, lc = Ls[c], c
            if Rs[c] > mR:
                mR, rc = Rs[c], c
        err = 1.0 - (mL + mR) / S
        alpha = math.log((1.0 - err) / max(err, 1e-12)) + math.log(C - 1)
        ea = math.exp(alpha)
        hit = n / (S * ((1.0 - err) + err * ea))
        split = int(sp[0])
        rec.copy_(torch.tensor([int(bf[0]) if split else -1, int(bb[0]), lc, rc], dtype=torch.int32))
        mul.copy_(torch.tensor([hit, hit * ea], dtype=torch.float64))
        info.copy_(torch.tensor([float(split), float(bf[0]), float(bb[0]), float(lc), float(rc), err, alpha, S]
                                + Ls + Rs, dtype=torch.float64))
        return info
    st = _lib.kernels().harp_boost_class_finish(bf.data_ptr(), bb.data_ptr(), sp.data_ptr(), L.data_ptr(),
                                                R.data_ptr(), T.data_ptr(), C, float(n), rec.data_ptr(),
                                                mul.data_ptr(), info.data_ptr(), _lib.stream_ptr(dev))
    _status(st, "boost_class_finish")
    return info


def root_split(H: torch.Tensor, task: int):
    """The forest engine's split search on root histograms [M, d, B, C] (min_leaf 1.0 in weight
    units): ``split_node``'s tuple (feature, bin, gain, split, L, R, T)."""
    cg, cb = F.split_feature(H, F.REAL, task, 1.0, None)
    return F.split_node(H, F.REAL, cg, cb)


def ada_fit(Xb, y, d: int, B: int, C: int, rounds: int, n_total: Optional[int] = None,
            w0: Optional[torch.Tensor] = None, reduce: Optional[Callable[[torch.Tensor], None]] = None,
            trace: Optional[Callable[[int, dict], None]] = None) -> List[List[float]]:
    """SAMME rounds with stumps on the binned rows ``Xb`` [n, dpad], labels ``y`` int32.
    Weights are kept at sum ``n_total`` (rows over all shards; ``w0`` defaults to ones).
    ``reduce(H)`` sums a round's histogram in place over the workers holding the other row
    shards: every decision, error and multiplier comes from the reduced ``H`` alone, so all
    workers end with the same learners. ``trace(round, state)`` receives ``H`` and the round's
    record (tests). Returns the ``info`` rows (:func:`class_finish`) of the learners kept, by
    the rules of the torch engine: ``err >= 1 - 1/C`` discards the learner and stops,
    ``err < 1e-12`` keeps it and stops; a root that does not split stops."""
    F.check_shape(B, C)
    dev = Xb.device
    n = Xb.shape[0]
    y = y.to(device=dev, dtype=torch.int32).contiguous()
    w = [torch.ones(n, dtype=torch.float64, device=dev) if w0 is None else w0.to(dev).double().contiguous().clone(),
         torch.empty(n, dtype=torch.float64, device=dev)]
    rec, mul = new_class_state(dev)
    kept: List[List[float]] = []
    for t in range(rounds):
        H = class_round(Xb, y, w[t & 1], w[(t + 1) & 1], rec, mul, d, B, C)
        if reduce is not None:
            reduce(H)
        bf, bb, _, sp, L, R, T = root_split(H, F.GINI)
        row = class_finish(bf, bb, sp, L, R, T, float(n_total or n), rec, mul).tolist()  # the round's one read
        if trace is not None:
            trace(t, dict(H=H, split=bool(row[0]), feature=int(row[1]), bin=int(row[2]), err=row[5], alpha=row[6],
                          info=row, rec=rec.clone(), mul=mul.clone()))
        if not row[0] or row[5] >= 1 - 1.0 / C:
            break
        kept.append(row)
        if row[5] < 1e-12:
            break
    return kept


# ---------------------------------------------------------------- logit round
def new_logit_state(K: int, device) -> Tuple[torch.Tensor, torch.Tensor]:
    """K constant-zero stumps: (rec_i [K, 2] int32 (feature, bin), rec_v [K, 2] fp64 (v_left, v_right))."""
    rec_i = torch.zeros((K, 2), dtype=torch.int32, device=device)
    rec_i[:, 0] = -1
    return rec_i, torch.zeros((K, 2), dtype=torch.float64, device=device)


def logit_round(Xb, y, F_in, F_out, rec_i, rec_v, zmax: float, d: int, B: int, K: int,
                wz: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Histograms [K, d, B, 3] fp64 of (w, w z, w z^2) for every class after the update
    ``F_out = F_in + (K-1)/K (g - mean g)``, ``g_k`` the previous round's stump k (``rec_i[k] =
    (feature, bin)``, ``rec_v[k] = (v_left, v_right)``, feature < 0: the constant v_left);
    ``p`` = max-subtracted softmax of F_out, ``w = max(p (1 - p), 1e-12)``, ``z = clamp(((y ==
    k) - p) / w, +-zmax)``. ``wz`` [n, K, 2], if given, receives (w, z). A row whose bin is >= B
    or whose label is outside [0, K) adds nothing to the histograms; its ``F_out`` and ``wz``
    are still written."""
    F.check_shape(B, K)
    n = Xb.shape[0]
    dev = Xb.device
    if not _lib.use_native(Xb):
        yl = y.long()
        g = torch.empty((n, K), dtype=torch.float64)
        for k in range(K):
            f = int(rec_i[k, 0])
            if f >= d:
                f = -1
            right = (Xb[:, f].long() > int(rec_i[k, 1])) if f >= 0 else torch.zeros(n, dtype=torch.bool)
            g[:, k] = torch.where(right, rec_v[k, 1], rec_v[k, 0])
        gs = torch.zeros(n, dtype=torch.float64)
        for k in range(K):
            gs = gs + g[:, k]
        Fn = F_in + ((K - 1) / K) * (g - (gs / K)[:, None])
        F_out.copy_(Fn)
        e = torch.exp(Fn - Fn.max(1, keepdim=True).values)
        se = torch.zeros(n, dtype=torch.float64)
        for k in range(K):
            se = se + e[:, k]
        p = e / se[:, None]
        Y = (yl[:, None] == torch.arange(K)[None, :]).double()
        w = (p * (1.0 - p)).clamp_min(1e-12)
        z = ((Y - p) / w).clamp(-zmax, zmax)
        if wz is not None:
            wz.copy_(torch.stack([w, z], 2))
        return logit_hist(Xb, w, z, d, B, y)
    Xb = Xb.contiguous()
    H = torch.zeros((K, d, B, 3), dtype=torch.float64, device=dev)
    st = _lib.kernels().harp_boost_logit_round(
        Xb.data_ptr(), Xb.shape[1], n, y.data_ptr(), F_in.data_ptr(), F_out.data_ptr(), rec_i.data_ptr(),
        rec_v.data_ptr(), float(zmax), d, B, K, H.data_ptr(), _lib.ptr(wz), _lib.stream_ptr(dev))
    _status(st, "boost_logit_round")
    return H


def logit_hist(Xb, w, z, d: int, B: int, y) -> torch.Tensor:
    """[K, d, B, 3] histogram of (w, w z, (w z) z) [n, K] in plain torch (the mirror's, and
    the tests' from the kernel's own (w, z)). A row whose bin is >= B or whose label ``y`` is
    outside [0, K) adds nothing."""
    n, K = w.shape
    bins = Xb[:, :d].long()
    ok = (bins < B) & ((y >= 0) & (y < K))[:, None]
    wzv = w * z
    val = torch.stack([w, wzv, wzv * z], 2)  # [n, K, 3]
    H = torch.zeros((K * d * B, 3), dtype=torch.float64, device=w.device)
    base = torch.arange(d, device=w.device)[None, :] * B + bins
    for k in range(K):
        H.index_add_(0, (k * d * B + base)[ok], val[:, k][:, None, :].expand(-1, d, -1)[ok])
    return H.view(K, d, B, 3)


def logit_records(bf, bb, sp, L, R, T):
    """The K regression stumps of a round from ``split_node``'s outputs (device ops, no host
    read): rec_i [K, 2], rec_v [K, 2] and the root values [K]."""
    split = sp.bool()
    root = T[:, 1] / T[:, 0].clamp_min(1e-300)
    vl = torch.where(split, L[:, 1] / L[:, 0].clamp_min(1e-300), root)
    vr = torch.where(split, R[:, 1] / R[:, 0].clamp_min(1e-300), root)
    rec_i = torch.stack([torch.where(split, bf, torch.full_like(bf, -1)), bb], 1).contiguous()
    return rec_i, torch.stack([vl, vr], 1).contiguous(), root


def logit_fit(Xb, y, d: int, B: int, K: int, rounds: int, zmax: float,
              reduce: Optional[Callable[[torch.Tensor], None]] = None,
              trace: Optional[Callable[[int, dict], None]] = None):
    """LogitBoost rounds with one regression stump per class. Returns CPU tensors
    (rec_i [rounds, K, 2] int64, rec_v [rounds, K, 2], root [rounds, K]): one host read per
    fit. ``reduce`` / ``trace`` as in :func:`ada_fit`."""
    F.check_shape(B, K)
    dev = Xb.device
    n = Xb.shape[0]
    y = y.to(device=dev, dtype=torch.int32).contiguous()
    Fb = [torch.zeros((n, K), dtype=torch.float64, device=dev), torch.empty((n, K), dtype=torch.float64, device=dev)]
    rec_i, rec_v = new_logit_state(K, dev)
    out = []
    for t in range(rounds):
        H = logit_round(Xb, y, Fb[t & 1], Fb[(t + 1) & 1], rec_i, rec_v, zmax, d, B, K)
        if reduce is not None:
            reduce(H)
        bf, bb, _, sp, L, R, T = root_split(H, F.MSE)
        rec_i, rec_v, root = logit_records(bf, bb, sp, L, R, T)
        out.append((rec_i, rec_v, root))
        if trace is not None:
            trace(t, dict(H=H, split=sp, feature=bf, bin=bb, L=L, R=R, T=T))
    return (torch.stack([o[0] for o in out]).long().cpu(), torch.stack([o[1] for o in out]).cpu(),
            torch.stack([o[2] for o in out]).cpu())


# ---------------------------------------------------------------- BrownBoost line search
POT, COR = 1, 2  # which sums brown_sums evaluates


def brown_sums(r, u, scal, cand, what: int = POT | COR) -> torch.Tensor:
    """[J, 2] = (pot_j, cor_j) of the J <= 64 candidate steps ``cand`` [J, 2] = (a_j, t_j):
    ``pot = sum(1 - erf(z / sqrt(c)))``, ``cor = sum(exp(-z^2 / c) u)``, ``z = r + s - t_j + a_j
    u``, ``scal = (s, c)``; a sum ``what`` leaves out is returned as 0. On the GPU per-block
    partials are summed in block order, so two launches return the same bits."""
    J = cand.shape[0]
    if J > MAX_CAND:
        raise ValueError(f"brown_sums takes at most {MAX_CAND} candidates (got {J})")
    n = r.numel()
    if not _lib.use_native(r):
        s, c = float(scal[0]), float(scal[1])
        z = ((r[:, None] + s) - cand[None, :, 1]) + cand[None, :, 0] * u[:, None]
        zero = torch.zeros(J, dtype=torch.float64)
        pot = (1.0 - torch.erf(z / math.sqrt(c))).sum(0) if what & POT else zero
        cor = (torch.exp((-(z * z)) / c) * u[:, None]).sum(0) if what & COR else zero
        return torch.stack([pot, cor], 1)
    k = _lib.kernels()
    cand = cand.contiguous()
    part = torch.empty((k.harp_boost_brown_blocks(n), J, 2), dtype=torch.float64, device=r.device)
    out = torch.empty((J, 2), dtype=torch.float64, device=r.device)
    st = k.harp_boost_brown_sums(r.data_ptr(), u.data_ptr(), n, scal.data_ptr(), cand.data_ptr(), J, what,
                                 part.data_ptr(), out.data_ptr(), _lib.stream_ptr(r.device))
    _status(st, "boost_brown_sums")
    return out


def _section_point(lo, hi, j: int):
    return hi if j >= MAX_CAND - 1 else (lo if j < 0 else lo + (hi - lo) * ((j + 1) / MAX_CAND))


def brown_step(sums, srch, a: float, cand, pas: int) -> None:
    """One step of the 64-way section for t. ``srch`` = (lo, hi, target, done, t) fp64 [5] and
    ``cand`` [64, 2] are updated in place: pass 0 tests "time runs out" (pot(hi) <= target:
    done, t = hi); every pass narrows [lo, hi] to the first sub-interval whose upper end has
    pot >= target; then t = (lo + hi) / 2 and the next candidates are the 64 section points
    (the last one is hi itself). ``pas < 0`` only writes the candidates."""
    if not _lib.use_native(srch):
        lo, hi, target, done = float(srch[0]), float(srch[1]), float(srch[2]), bool(srch[3])
        if pas >= 0 and not done:
            pot = sums[:, 0].tolist()
            if pas == 0 and pot[-1] <= target:
                done = True
            else:
                js = next((j for j in range(MAX_CAND) if pot[j] >= target), MAX_CAND - 1)
                lo, hi = _section_point(lo, hi, js - 1), _section_point(lo, hi, js)
        srch.copy_(torch.tensor([lo, hi, target, float(done), hi if done else 0.5 * (lo + hi)], dtype=torch.float64))
        cand[:, 0] = a
        cand[:, 1] = torch.tensor([_section_point(lo, hi, j) for j in range(MAX_CAND)], dtype=torch.float64)
        return
    st = _lib.kernels().harp_boost_brown_step(_lib.ptr(sums), srch.data_ptr(), float(a), cand.data_ptr(), pas,
                                              _lib.stream_ptr(srch.device))
    _status(st, "boost_brown_step")


def brown_t_search(r, u, scal, a: float, target) -> torch.Tensor:
    """The t in [0, s] at which the potential of the step (a, t) equals ``target`` (a device
    scalar): ``srch`` [5] with t in ``srch[4]`` (exactly s when time runs out). No host read."""
    srch = torch.zeros(5, dtype=torch.float64, device=r.device)
    srch[1] = scal[0]
    srch[2] = target
    cand = torch.empty((MAX_CAND, 2), dtype=torch.float64, device=r.device)
    brown_step(None, srch, a, cand, -1)
    for p in range(T_PASSES):
        brown_step(brown_sums(r, u, scal, cand, POT), srch, a, cand, p)
    return srch


def brown_solve(r, u, s: float, c: float, iters: int, nu: float):
    """The BrownBoost step (alpha, t) of ``harp_amd.models.trees.brown_line_search`` with the t
    search on the device; the a search keeps that function's control flow on the host at one
    read per probe. Returns (alpha, t, host reads)."""
    dev = r.device
    scal = torch.tensor([s, c], dtype=torch.float64, device=dev)
    target = brown_sums(r, u, scal, torch.zeros((1, 2), dtype=torch.float64, device=dev), POT)[0, 0]
    reads = 0

    def corr(a):
        nonlocal reads
        srch = brown_t_search(r, u, scal, a, target)
        one = torch.stack([torch.full((), a, dtype=torch.float64, device=dev), srch[4]]).reshape(1, 2)
        g, t = torch.stack([brown_sums(r, u, scal, one, COR)[0, 1], srch[4]]).tolist()  # the probe's one read
        reads += 1
        return g, t

    a_lo, a_hi = 0.0, 1.0
    g_hi, t_hi = corr(a_hi)
    while g_hi > 0 and t_hi < s and a_hi < 1e3:
        a_lo, a_hi = a_hi, a_hi * 2
        g_hi, t_hi = corr(a_hi)
    if g_hi > 0:  # time runs out before the correlation vanishes
        return a_hi, t_hi, reads
    for _ in range(iters):
        mid = 0.5 * (a_lo + a_hi)
        g, _t = corr(mid)
        if g > 0:
            a_lo = mid
        else:
            a_hi = mid
        if a_hi - a_lo < nu * 1e-3:
            break
    a = 0.5 * (a_lo + a_hi)
    t = float(brown_t_search(r, u, scal, a, target)[4])
    return a, t, reads + 1
