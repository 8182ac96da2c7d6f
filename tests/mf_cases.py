"""Shared cases, references and mutants for the MF-CCD and ALS kernel edge tests
(csrc/ccd.hip, csrc/als.hip). No GPU and no test functions here.

CCD. The reference of a coordinate phase is ``harp_amd.ops.ccd.phase`` on CPU tensors (the
vectorised torch formulation, which shares no code with the kernels): in fp64 it is the
reference, in fp32 it is the rounding yardstick. A case is one CSR whose row lengths are
given; the nonzeros at the structural borders of every row (first, last, 64q - 1 / 64q,
1024q - 1 / 1024q, 4096c - 1 / 4096c) are sentinels: their other-factor rows are SENTINEL
times larger than the rest, and so is the part of their residual that the factors explain;
the part that no dimension explains (what is left after the update, and what a dropped
nonzero moves z by) is SENTINEL_RES times larger. A kernel that drops or skips exactly such
a nonzero moves the result far out of tolerance. Per row class (wave / mid / wide / lock,
from LONG_ROW, block_max(), block_max(True) and CHUNK as the library reports them; the
documented 8192 / 12288 when no GPU library is present)

    tol_W[class]   = 4 * max |W_fp32cpu - W_fp64|        (floor 4 * 2^-23 * max(1, |W_fp64|))
    tol_res[class] = the same on the residuals of the class's rows

never anything measured on a kernel. Mutants of the fp64 reference: (a) one border nonzero
left out of both sums of every dimension, (b) its residual left un-updated for one
dimension. Every mutant (a) has to move its row's W by >= 4 * tol_W, every mutant (b) its
residual by >= 4 * tol_res (tests/test_mf_cases.py asserts it for every case; mutants are
evaluated through the row's k x k Gram matrix, cross-checked against a plain per-row loop).
Mutant (b) is taken at every dimension, except in the cases of B_AT_LARGEST_STEP (below).

Measured on the CPU over all cases of tests/test_mf_cases.py (SENTINEL = 8, SENTINEL_RES =
32), the smallest mutant shift in units of the tolerance, per class (required: >= 4):

    class   (a) shift_W / tol_W   (b) shift_res / tol_res   (b) in the B_AT_LARGEST_STEP cases
    wave         1117.2                  23.5                      228.2
    mid           178.7                  55.8                      360.8
    wide           73.4                 110.1                     1068.8
    lock           26.9                 185.6                      242.0

(With sentinels scaled by 8 alone, residual included, class lock reached only 2.2: a
sentinel whose unexplained residual happens to be near zero can be dropped unseen, hence
the separate scale bounded away from zero.)

ALS. The exact cases hold small integers (F in -2..2, ratings 0..3, alpha = 2, lam = 0.25),
so every product and partial sum of a normal-equation entry is a multiple of 0.25 below
2^24: any summation order gives the same bits in fp32 and fp64, and A / rhs are compared
with ``torch.equal``.
"""
from __future__ import annotations

import functools
from dataclasses import dataclass, field

import torch

from harp_amd.ops import ccd as C

CLASSES = ("wave", "mid", "wide", "lock")
DOCUMENTED_BLOCK_MAX = (8192, 12288)  # csrc/ccd.hip BT * 8, BT * 12
SENTINEL = 8.0  # scale of a sentinel's other-factor row
SENTINEL_RES = 32.0  # scale of the part of a sentinel's residual that no dimension explains
N_NORMAL, N_SENT = 448, 64  # other-factor rows: ordinary ones, then the sentinel pool
MUTANT_FACTOR = 4.0


def class_limits(block_rows: bool = True) -> tuple:
    """Longest row of the wave, mid and wide classes. ``block_rows`` False: the plan sends
    every row above LONG_ROW to the lockstep kernel (RowPlan(block_rows=False))."""
    if not block_rows:
        return (C.LONG_ROW, C.LONG_ROW, C.LONG_ROW)
    b, w = C.block_max(), C.block_max(True)
    if b == 0:  # no GPU library on this machine: the documented values
        b, w = DOCUMENTED_BLOCK_MAX
    return (C.LONG_ROW, b, w)


def border_indices(n: int) -> list:
    """In-row indices of the structural borders of a row of n nonzeros."""
    s = set()
    if n:
        s.update((0, n - 1))
    for step in (64, 1024, C.CHUNK):
        for q in range(step, n + 1, step):
            s.add(q - 1)
            if q < n:
                s.add(q)
    return sorted(s)


@dataclass
class CCDCase:
    lens: torch.Tensor  # [n_rows] int64
    k: int
    lam: float
    limits: tuple
    phases: int
    zero_dim: object
    rows: torch.Tensor  # [nnz] int32
    cols: torch.Tensor  # [nnz] int32
    ptr: torch.Tensor  # [n_rows + 1] int64
    pos: torch.Tensor  # [nnz] index inside the row
    border: torch.Tensor  # [nnz] bool
    W0: torch.Tensor  # fp32
    H: torch.Tensor  # fp32
    res0: torch.Tensor  # fp32
    row_cls: torch.Tensor = field(default=None)  # [n_rows] 0..3
    nz_cls: torch.Tensor = field(default=None)  # [nnz]


@functools.lru_cache(maxsize=None)
def ccd_case(lens: tuple, k: int, lam: float, seed: int = 0, block_rows: bool = True, zero_dim=None,
             phases: int = 1) -> CCDCase:
    g = torch.Generator().manual_seed(1000 * seed + k)
    lens_t = torch.tensor(lens, dtype=torch.int64)
    n_rows = lens_t.numel()
    ptr = torch.zeros(n_rows + 1, dtype=torch.int64)
    ptr[1:] = torch.cumsum(lens_t, 0)
    nnz = int(ptr[-1])
    rows = torch.repeat_interleave(torch.arange(n_rows), lens_t)
    pos = torch.arange(nnz) - ptr[rows]
    border = (pos == 0) | (pos == lens_t[rows] - 1)
    for step in (64, 1024, C.CHUNK):
        border |= (pos % step == 0) | (pos % step == step - 1)
    cols = torch.where(border, N_NORMAL + torch.randint(0, N_SENT, (nnz,), generator=g),
                       torch.randint(0, N_NORMAL, (nnz,), generator=g))
    sign = lambda *shape: torch.randint(0, 2, shape, generator=g).double() * 2 - 1
    uni = lambda lo, hi, *shape: lo + (hi - lo) * torch.rand(*shape, generator=g, dtype=torch.float64)
    H = sign(N_NORMAL + N_SENT, k) * uni(0.2, 0.3, N_NORMAL + N_SENT, k)
    H[N_NORMAL:] *= SENTINEL
    if zero_dim is not None:
        H[:, zero_dim] = 0.0
    # residuals with a large component along every dimension (so every |delta_t| is large:
    # W starts far from its fixed point) plus noise; the phase does not need val - W.H
    # (a dropped nonzero j moves z_t by r_j h_jt / down_t, r_j its residual after the update,
    # which is the unexplained part: bounded away from 0 and largest on the sentinels)
    cvec = sign(k) * uni(1.0, 2.0, k)
    noise = sign(nnz) * uni(0.5, 1.0, nnz) * torch.where(border, SENTINEL_RES, 1.0)
    res0 = H[cols] @ cvec + noise
    W0 = sign(n_rows, k) * uni(1.0, 2.0, n_rows, k)
    limits = class_limits(block_rows)
    row_cls = sum((lens_t > lim).long() for lim in limits)
    return CCDCase(lens_t, k, lam, limits, phases, zero_dim, rows.int(), cols.int(), ptr, pos, border, W0.float(),
                   H.float(), res0.float(), row_cls, row_cls[rows])


@dataclass
class CCDRef:
    W64: torch.Tensor
    res64: torch.Tensor
    Wpre: torch.Tensor  # fp64 state before the last phase
    respre: torch.Tensor
    errW: dict
    errR: dict
    tolW: dict
    tolR: dict


def _run_phases(case: CCDCase, dt):
    W, r, H = case.W0.to(dt).clone(), case.res0.to(dt).clone(), case.H.to(dt)
    pre = None
    for p in range(case.phases):
        if p == case.phases - 1:
            pre = (W.clone(), r.clone())
        C.phase(case.rows, case.ptr, case.cols, r, W, H, case.lam)
    return W, r, pre


_EPS32 = 2.0 ** -23


@functools.lru_cache(maxsize=None)
def _ccd_reference(case_key) -> CCDRef:
    case = ccd_case(*case_key)
    W64, r64, (Wpre, rpre) = _run_phases(case, torch.float64)
    W32, r32, _ = _run_phases(case, torch.float32)
    dW = (W32.double() - W64).abs().amax(1)
    dR = (r32.double() - r64).abs()
    errW, errR, tolW, tolR = {}, {}, {}, {}
    for ci, name in enumerate(CLASSES):
        rm, zm = case.row_cls == ci, case.nz_cls == ci
        if not bool((rm & (case.lens > 0)).any()):
            continue
        errW[name], errR[name] = float(dW[rm].max()), float(dR[zm].max())
        tolW[name] = 4.0 * max(errW[name], _EPS32 * max(1.0, float(W64[rm].abs().max())))
        tolR[name] = 4.0 * max(errR[name], _EPS32 * max(1.0, float(r64[zm].abs().max())))
    return CCDRef(W64, r64, Wpre, rpre, errW, errR, tolW, tolR)


def ccd_reference(lens: tuple, k: int, lam: float, seed: int = 0, block_rows: bool = True, zero_dim=None,
                  phases: int = 1):
    """(case, reference), both cached: computed once, shared, never modified."""
    key = (lens, k, lam, seed, block_rows, zero_dim, phases)
    return ccd_case(*key), _ccd_reference(key)


def ccd_compare(case: CCDCase, ref: CCDRef, W: torch.Tensor, res: torch.Tensor) -> dict:
    """Assert W and every residual within the class tolerances of the fp64 reference;
    returns {class: (max |dW| / tol_W, max |dres| / tol_res)}."""
    W, res = W.detach().cpu().double(), res.detach().cpu().double()
    assert W.shape == ref.W64.shape and res.shape == ref.res64.shape
    dW, dR = (W - ref.W64).abs(), (res - ref.res64).abs()
    dW[torch.isnan(dW)] = float("inf")
    dR[torch.isnan(dR)] = float("inf")
    out, bad = {}, []
    for ci, name in enumerate(CLASSES):
        if name not in ref.tolW:
            continue
        ri = torch.nonzero(case.row_cls == ci).reshape(-1)
        zi = torch.nonzero(case.nz_cls == ci).reshape(-1)
        ew, er = dW[ri], dR[zi]
        out[name] = (float(ew.max()) / ref.tolW[name], float(er.max()) / ref.tolR[name])
        if not float(ew.max()) <= ref.tolW[name]:
            a = int(ew.argmax())
            r, t = int(ri[a // case.k]), a % case.k
            bad.append(f"W[{name}] row {r} (len {int(case.lens[r])}) dim {t}: |dW| {float(ew.max()):.3e} > tol "
                       f"{ref.tolW[name]:.3e} (got {float(W[r, t])!r}, want {float(ref.W64[r, t])!r})")
        if not float(er.max()) <= ref.tolR[name]:
            j = int(zi[int(er.argmax())])
            r = int(case.rows[j])
            bad.append(f"res[{name}] row {r} (len {int(case.lens[r])}) index {int(case.pos[j])}: |dres| "
                       f"{float(er.max()):.3e} > tol {ref.tolR[name]:.3e}")
    assert not bad, "; ".join(bad)
    return out


def ccd_mutant_row(case: CCDCase, ref: CCDRef, row: int, j: int, kind: str, tb: int = 0):
    """The fp64 reference with one mutated row, as a plain loop: kind "a" leaves nonzero j of
    the row out of both sums of every dimension, "b" leaves its residual un-updated in
    dimension tb. Returns full (W, res) of the last phase."""
    a, b = int(case.ptr[row]), int(case.ptr[row + 1])
    n = b - a
    h = case.H.double()[case.cols[a:b].long()]
    r, w = ref.respre[a:b].clone(), ref.Wpre[row].clone()
    keep = torch.ones(n, dtype=torch.bool)
    if kind == "a":
        keep[j] = False
    for t in range(case.k):
        ht = h[:, t]
        up = ((r + w[t] * ht) * ht)[keep].sum()
        dn = case.lam * n + (ht * ht)[keep].sum()
        z = up / dn if dn > 0 else w[t]
        old = r[j].clone()
        r -= (z - w[t]) * ht
        if kind == "b" and t == tb:
            r[j] = old
        w[t] = z
    W, res = ref.W64.clone(), ref.res64.clone()
    W[row], res[a:b] = w, r
    return W, res


def ccd_mutant_shifts(case: CCDCase, ref: CCDRef) -> dict:
    """For every row of >= 2 nonzeros and every border index: the shift of the row's W under
    mutant (a) (max over dimensions) and of that residual under mutant (b) (min over the
    dimensions it can be applied to). Rows of equal length are evaluated together through
    their Gram matrices G = Hr^T Hr and c = Hr^T res: with delta_s the steps so far,
    up_t = c_t - sum_{s<t} delta_s G_st + w_t G_tt, down_t = lam n + G_tt.
    Returns {class: dict(a=min shift_W, b=min shift_res over every dimension, b1=min shift_res
    at each border's most sensitive dimension, self=max formula error)}."""
    k, lam = case.k, case.lam
    H64 = case.H.double()
    out = {}
    for n in torch.unique(case.lens).tolist():
        if n < 2:
            continue
        rws = torch.nonzero(case.lens == n).reshape(-1)
        name = CLASSES[int(case.row_cls[rws[0]])]
        idx = case.ptr[rws][:, None] + torch.arange(n)[None, :]
        Hr = H64[case.cols[idx].long()]  # [R, n, k]
        r0 = ref.respre[idx]  # [R, n]
        G = torch.einsum("rnk,rnl->rkl", Hr, Hr)
        c = torch.einsum("rn,rnk->rk", r0, Hr)
        w0 = ref.Wpre[rws]  # [R, k]
        B = torch.tensor(border_indices(n))
        assert torch.equal(torch.nonzero(case.border[idx[0]]).reshape(-1), B)
        hb, rb = Hr[:, B, :], r0[:, B]  # [R, M, k], [R, M]
        R, M = rb.shape

        def sweep(t, delta, up_extra, dn_extra):
            up = (c[:, None, t] - torch.einsum("rms,rs->rm", delta[:, :, :t], G[:, :t, t])
                  + w0[:, None, t] * G[:, None, t, t] + up_extra)
            dn = lam * n + G[:, None, t, t] + dn_extra
            wt = w0[:, None, t].expand(R, M)
            return torch.where(dn > 0, up / dn.clamp_min(1e-300), wt) - wt

        zero = torch.zeros(R, M, dtype=torch.float64)
        # the formula itself, unmutated, against the reference
        delta = torch.zeros(R, M, k, dtype=torch.float64)
        for t in range(k):
            delta[:, :, t] = sweep(t, delta, zero, zero)
        dref = ref.W64[rws] - w0  # [R, k]
        selferr = float((delta - dref[:, None, :]).abs().max() / max(1.0, float(dref.abs().max())))
        # (a)
        delta = torch.zeros(R, M, k, dtype=torch.float64)
        for t in range(k):
            resb = rb - (delta[:, :, :t] * hb[:, :, :t]).sum(-1)
            delta[:, :, t] = sweep(t, delta, -(resb + w0[:, None, t] * hb[:, :, t]) * hb[:, :, t], -hb[:, :, t] ** 2)
        shift_a = (delta - dref[:, None, :]).abs().amax(-1)  # [R, M]
        # (b)
        final_ref = ref.res64[idx][:, B]
        shift_b = torch.full((R, M), float("inf"), dtype=torch.float64)
        shift_b1 = torch.zeros(R, M, dtype=torch.float64)
        for tb in range(k):
            if tb == case.zero_dim:
                continue  # delta is exactly 0 there: skipping that update is no mutation
            delta = dref[:, None, :].expand(R, M, k).clone()
            extra = delta[:, :, tb] * hb[:, :, tb]
            for t in range(tb + 1, k):
                delta[:, :, t] = sweep(t, delta, extra * hb[:, :, t], zero)
            dh = delta * hb
            final = rb - dh.sum(-1) + dh[:, :, tb]
            shift_b = torch.minimum(shift_b, (final - final_ref).abs())
            shift_b1 = torch.maximum(shift_b1, (final - final_ref).abs())
        o = out.setdefault(name, dict(a=float("inf"), b=float("inf"), b1=float("inf"), self=0.0))
        o["a"], o["b"] = min(o["a"], float(shift_a.min())), min(o["b"], float(shift_b.min()))
        o["b1"] = min(o["b1"], float(shift_b1.min()))
        o["self"] = max(o["self"], selferr)
    return out


# ---------------------------------------------------------------- CCD case lists
BOUNDARY_LENS = (0, 1, 63, 64, 65, 128, 193, 255, 256, 257, 1023, 1024, 1025, 8191, 8192, 8193, 12287, 12288, 12289,
                 16384, 20481)
LOCK_SMALL_LENS = (0, 3, 257, 4095, 4096, 4097, 8193, 256, 1)
SHORT_LENS = (0, 1, 2, 63, 64, 65, 127, 128, 129, 191, 192, 193, 255, 256, 256, 0, 256)
STRIDE_WAVE_LENS = tuple(1 + (i * 7 + i // 3) % 3 for i in range(70000))
STRIDE_BLOCK_LENS = (257,) * 8200

BOUNDARY_KS, BOUNDARY_LAMS = (1, 2, 3, 4, 5, 8), (0.05, 0.0)
LOCK_SMALL_KS = (1, 2, 3, 4, 7)
ZERO_DIM_CASES = ((3, 0), (5, 4), (8, 2))  # (k, zeroed dimension of the other factor)


# Cases in which some step delta_t is tiny by necessity, so that skipping exactly that update
# is no observable mutation: the second phase of the reuse cases starts next to the fixed
# point, and among the 70,000 (8,200) rows of the stride cases some step lands next to zero
# by chance. There mutant (b) is asked at the dimension of each border's largest delta_t h_jt
# instead of at every dimension.
B_AT_LARGEST_STEP = ("reuse-k3", "reuse-boundary-k4", "stride-wave", "stride-block")


def all_ccd_case_keys() -> dict:
    """id -> arguments of ccd_reference for every case the GPU tests use."""
    keys = {}
    for k in BOUNDARY_KS:
        for lam in BOUNDARY_LAMS:
            keys[f"boundary-k{k}-lam{lam}"] = (BOUNDARY_LENS, k, lam)
    for k in LOCK_SMALL_KS:
        keys[f"lockstep-k{k}"] = (LOCK_SMALL_LENS, k, 0.05, 1, False)
    keys["reuse-k3"] = (LOCK_SMALL_LENS, 3, 0.05, 2, False, None, 2)
    keys["reuse-boundary-k4"] = (BOUNDARY_LENS, 4, 0.05, 2, True, None, 2)
    for k in (4, 5):
        keys[f"short-k{k}"] = (SHORT_LENS, k, 0.05, 3)
    for k, t in ZERO_DIM_CASES:
        keys[f"zero-k{k}-t{t}"] = (BOUNDARY_LENS, k, 0.0, 4, True, t)
    keys["stride-wave"] = (STRIDE_WAVE_LENS, 4, 0.05, 5)
    keys["stride-block"] = (STRIDE_BLOCK_LENS, 4, 0.05, 6)
    return keys


# ---------------------------------------------------------------- CCD residual (exact)
def residual_exact_case(nnz: int, k: int, seed: int = 0):
    """Integer-valued factors (-2..2) and ratings (0..5): <w, h> and val - <w, h> are small
    integers, exact in fp32 in any order. Returns fp32 (rows int32, cols int32, val, Fr, Fc)
    and the fp64 reference."""
    g = torch.Generator().manual_seed(77 * seed + 1000 * k + nnz)
    n_r, n_c = 37, 53
    rows = torch.randint(0, n_r, (nnz,), generator=g).int()
    cols = torch.randint(0, n_c, (nnz,), generator=g).int()
    rows[-1], cols[-1] = n_r - 1, n_c - 1
    rows[0], cols[0] = 0, 0
    val = torch.randint(0, 6, (nnz,), generator=g).float()
    Fr = torch.randint(-2, 3, (n_r, k), generator=g).float()
    Fc = torch.randint(-2, 3, (n_c, k), generator=g).float()
    want = C.residual(rows, cols, val.double(), Fr.double(), Fc.double())
    return rows, cols, val, Fr, Fc, want


# ---------------------------------------------------------------- ALS exact cases
ALS_LENS = (0, 1, 31, 32, 33, 63, 64, 65, 96, 97, 130)
ALS_ALPHA, ALS_LAM = 2.0, 0.25
ALS_N_COLS = 200


@dataclass
class ALSCase:
    f: int
    crow: torch.Tensor  # int64 [n_rows + 1]
    cols: torch.Tensor  # int64
    vals: torch.Tensor  # fp64, integers 0..3
    F: torch.Tensor  # fp64, integers -2..2
    G: torch.Tensor  # F^T F


@functools.lru_cache(maxsize=None)
def als_exact_case(f: int, seed: int = 0) -> ALSCase:
    g = torch.Generator().manual_seed(31 * seed + f)
    lens = torch.tensor(ALS_LENS)
    crow = torch.zeros(lens.numel() + 1, dtype=torch.int64)
    crow[1:] = torch.cumsum(lens, 0)
    nnz = int(crow[-1])
    cols = torch.randint(0, ALS_N_COLS, (nnz,), generator=g)
    vals = torch.randint(0, 4, (nnz,), generator=g).double()
    vals[::5] = 0.0
    for r in range(lens.numel()):
        a, b = int(crow[r]), int(crow[r + 1])
        if b - a >= 2:
            cols[a + 1] = cols[a]  # a duplicate column inside the row
        if b - a >= 31:
            cols[b - 1], cols[a + 2] = ALS_N_COLS - 1, 0
            vals[b - 1], vals[a + 2] = 3.0, 1.0
    F = torch.randint(-2, 3, (ALS_N_COLS, f), generator=g).double()
    F[(F == 0).all(1), 0] = 1.0
    # the ratings at the chunk and buffer edges count in every mode (nonzero weight, nonzero row)
    for r in range(lens.numel()):
        a, n = int(crow[r]), int(lens[r])
        for p in (0, 31, 32, 63, 64, 95, 96, 127, 128, n - 1):
            if 0 <= p < n:
                vals[a + p] = max(float(vals[a + p]), 1.0)
    return ALSCase(f, crow, cols, vals, F, F.t() @ F)


def als_exact_reference(case: ALSCase, implicit: bool, scale_lam: bool, use_G: bool, lam: float = ALS_LAM,
                        alpha: float = ALS_ALPHA):
    """A [n_rows, f, f], rhs [n_rows, f] in fp64 by plain per-row outer products, and the
    largest sum of absolute values of the terms of any entry (bounds every partial sum)."""
    n_rows, f = case.crow.numel() - 1, case.f
    A = torch.zeros(n_rows, f, f, dtype=torch.float64)
    rhs = torch.zeros(n_rows, f, dtype=torch.float64)
    bound = 0.0
    eye = torch.eye(f, dtype=torch.float64)
    for r in range(n_rows):
        a, b = int(case.crow[r]), int(case.crow[r + 1])
        Fc, v = case.F[case.cols[a:b]], case.vals[a:b]
        aw = alpha * v if implicit else torch.ones_like(v)
        bw = torch.where(v > 0, 1 + alpha * v, torch.zeros_like(v)) if implicit else v
        lr = lam * max(b - a, 1) if scale_lam else lam
        for j in range(b - a):
            A[r] += aw[j] * torch.outer(Fc[j], Fc[j])
            rhs[r] += bw[j] * Fc[j]
        if use_G:
            A[r] += case.G
        A[r] += lr * eye
        mag = Fc.abs().t() @ (aw.abs()[:, None] * Fc.abs()) + (case.G.abs() if use_G else 0) + lr
        bound = max(bound, float(mag.max()), float((Fc.abs().t() @ bw.abs()).max()) if b > a else 0.0)
    return A, rhs, bound


def backward_error(A: torch.Tensor, x: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    """Normwise backward error ||b - A x|| / (||A|| ||x|| + ||b||) per system, in fp64
    (Frobenius / 2-norms); 0 where the residual is exactly 0; inf for a non-finite x."""
    A, x, b = A.double(), x.double(), b.double()
    num = (b - torch.einsum("rik,rk->ri", A, x)).norm(dim=1)
    den = A.flatten(1).norm(dim=1) * x.norm(dim=1) + b.norm(dim=1)
    eta = torch.where(num == 0, torch.zeros_like(num), num / den)
    eta[~torch.isfinite(x).all(1) | torch.isnan(eta)] = float("inf")
    return eta


def lapack_backward_error(A: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    """Backward error of LAPACK Cholesky (potrf + potrs) on the CPU in A's precision."""
    L, info = torch.linalg.cholesky_ex(A)
    assert int(info.abs().sum()) == 0
    x = torch.cholesky_solve(b[:, :, None], L)[:, :, 0]
    return backward_error(A, x, b)


def roundoff(dt) -> float:
    return 2.0 ** -24 if dt == torch.float32 else 2.0 ** -53


def spd_batch(m: int, f: int, seed: int):
    """m random SPD fp32 systems (A [m, f, f], rhs [m, f]); fp32 values are the exact inputs."""
    g = torch.Generator().manual_seed(seed)
    B = torch.randn(m, f, f + 3, generator=g, dtype=torch.float64)
    A = (B @ B.transpose(1, 2) + 0.5 * torch.eye(f, dtype=torch.float64)).float()
    A = (A + A.transpose(1, 2)) * 0.5
    rhs = torch.randn(m, f, generator=g, dtype=torch.float64).float()
    return A.contiguous(), rhs.contiguous()
