"""Oracle, launch rules and inputs of the exact SYRK tests (no GPU needed to import).

* ``feature_major_ref``: the blocked feature-major layout of csrc/syrk.hip in plain torch;
* ``launch_plan``: the launch rules of ``launch_syrk`` / ``harp_syrk_t_bf16`` in Python, so
  the form a case reaches (tile size, work items, splits, stages per split, workgroups) is
  computed, not guessed, and tests/test_syrk_oracle.py checks the case tables on the CPU;
* ``int_rows``: integer data in [-4, 4], for which every bf16 product and every fp32
  partial sum is exact in any order.
"""
import torch

KT = 48  # samples per stage = the layout's sample block


def feature_major_ref(Xb, n, d, ld, d_pad, ones_row=None):
    """XT [ld/48, d_pad, 48] from bf16 X [n, d]: (k // 48, f, k % 48) = X[k, f] for k < n,
    f < d; 1 at f == ones_row (default d) for k < n; 0 everywhere else."""
    assert ld % KT == 0 and ld >= n and d_pad >= d and Xb.dtype == torch.bfloat16
    ones_row = d if ones_row is None else ones_row
    D = torch.zeros((d_pad, ld), dtype=torch.bfloat16, device=Xb.device)
    D[:d, :n] = Xb[:n, :d].t()
    if 0 <= ones_row < d_pad:
        D[ones_row, :n] = 1
    return D.reshape(d_pad, ld // KT, KT).permute(1, 0, 2).contiguous()


def dense(XT):
    """The dense [d_pad, ld] feature-major matrix of a blocked XT."""
    nb, d_pad, kt = XT.shape
    return XT.permute(1, 0, 2).reshape(d_pad, nb * kt)


def gram_ref(XT):
    """D D^T in fp64, cast to fp32 (exact for the integer inputs used here)."""
    D = dense(XT).double()
    return (D @ D.t()).float()


def bound_ratio(G, X, ld):
    """Worst |G - ref| / bound over G[:d+1, :d+1] for row-major X [n, d] (ones column
    appended): ref = Xb^T Xb in fp64 on the bf16-rounded data, bound = (ld + 2) 2^-23
    (|Xb|^T |Xb|), the any-order summation bound with u = 2^-23 (it holds whether the matrix
    core's internal adds round or truncate). An error where the bound is 0 gives inf."""
    n, d = X.shape
    Xb = torch.cat([X.to(torch.bfloat16).double(), torch.ones(n, 1, dtype=torch.float64, device=X.device)], 1)
    ref = Xb.t() @ Xb
    bound = (ld + 2) * 2.0**-23 * (Xb.abs().t() @ Xb.abs())
    err = (G[: d + 1, : d + 1].double() - ref).abs()
    ratio = torch.where(bound > 0, err / bound, torch.where(err > 0, float("inf"), 0.0).to(err.dtype))
    return float(ratio.max())


def int_rows(n, d, seed, device="cpu"):
    """[n, d] integers uniform in [-4, 4] as bf16 (fixed seed; drawn on ``device``)."""
    g = torch.Generator(device=device).manual_seed(seed)
    return torch.randint(-4, 5, (n, d), generator=g, device=device, dtype=torch.int8).to(torch.bfloat16)


def exact_ok(ld):
    """|product| <= 16, so a partial sum is at most 16 ld; with a prefilled G0 below 2^20
    (and twice the sum for the call-twice cases) everything stays an integer below 2^24."""
    return 2 * 16 * ld + 2**20 < 2**24


def launch_plan(d_pad, ld, num_splits=0):
    """What ``harp_syrk_t_bf16(XT, ld, n=ld, d_pad, ..., num_splits)`` launches."""
    big = d_pad >= 512 and d_pad % 256 == 0
    mt, target_wg = (256, 1024) if big else (128, 2048)
    nt = d_pad // mt
    noff = nt * (nt - 1) // 2
    ntiles = noff + (nt + 1) // 2
    n = ld
    branch = "forced"
    if num_splits <= 0:
        per_xcd = 32 if big else 64
        if ntiles <= per_xcd:
            branch = "per_xcd"
            num_splits = 8 * (per_xcd // ntiles)
        else:
            branch = "target_wg"
            s0 = (target_wg + ntiles - 1) // ntiles
            num_splits, best = s0, 0.0
            for sp in range(s0, 2 * s0 + 1):
                B = ntiles * sp
                eff = B / float((B + 255) // 256 * 256)
                if eff > best + 1e-9:
                    best, num_splits = eff, sp
                if eff > 0.999:
                    break
        while num_splits > 1 and (n + num_splits - 1) // num_splits < 64 * KT:
            num_splits //= 2
    chunk = (n + num_splits - 1) // num_splits
    chunk = (chunk + KT - 1) // KT * KT
    splits = (n + chunk - 1) // chunk
    stages = [(min(chunk, n - s * chunk)) // KT for s in range(splits)]
    return dict(mt=mt, nt=nt, noff=noff, pairs=nt // 2, lone=nt % 2, ntiles=ntiles, branch=branch, splits=splits,
                stages=stages, workgroups=ntiles * splits)


# ------------------------------------------------------------------------------ case tables
# Tile forms: (d_pad, d, tile, nt, form). The ones row sits at feature d; features d+1 ..
# d_pad-1 are zero.
TILE_FORMS = [
    (128, 127, 128, 1, "lone diagonal tile, one panel (vmcnt(3) path); ones = last row of the only tile"),
    (256, 128, 128, 2, "1 off-diagonal + 1 pair (NB = 4); ones = first row of the second tile"),
    (256, 255, 128, 2, "1 off-diagonal + 1 pair (NB = 4); ones = last row"),
    (384, 300, 128, 3, "3 off-diagonal + pair + lone; 83 zero features"),
    (512, 511, 256, 2, "1 off-diagonal + 1 pair (NB = 8, all four tri_step modes)"),
    (640, 636, 128, 5, "10 off-diagonal + 2 pairs + lone"),
    (768, 767, 256, 3, "3 off-diagonal + pair + lone 256 tile (i0 > j0 + 31 skip)"),
    (896, 890, 128, 7, "21 off-diagonal + 3 pairs + lone = 25 work items"),
    (1024, 1000, 256, 4, "the bench shape: 6 off-diagonal + 2 pairs"),
    (1280, 1275, 256, 5, "10 off-diagonal + 2 pairs + lone"),
    (1664, 1660, 128, 13, "85 work items > 64: the target_wg branch"),
    (2304, 2300, 256, 9, "41 work items > 32: the target_wg branch on the 256-tile kernel"),
]
TILE_LDS = [192, 3072 * 2 + 48]  # 4 stages in one split / auto splits over 129 stages
# ld = 6192 ends in ONE split where the halving of the auto split count skips 2 (5, 85 and
# 41 work items): those widths get a longer ld with three or six auto splits, the last short
TILE_EXTRA = [
    (384, 300, 3072 * 3 + 96, [65, 65, 64]),
    (768, 767, 3072 * 3 + 96, [65, 65, 64]),
    (1664, 1660, 48 * 419, [70, 70, 70, 70, 70, 69]),  # 510 workgroups: two rounds of the 256 CUs
    (2304, 2300, 48 * 419, [140, 140, 139]),           # 123 workgroups
]

# Ring edges: (ld, num_splits, stages per split)
RING_PANELS = [128, 256, 512, 768]  # one- and two-panel jobs at both tile sizes
RING_EDGES = [
    (48, 1, [1]),
    (96, 1, [2]),
    (144, 1, [3]),
    (384, 3, [3, 3, 2]),
    (384, 5, [2, 2, 2, 2]),
    (384, 8, [1] * 8),
    (48 * 13, 2, [7, 6]),
]

# Remap: (d_pad, ld, num_splits, workgroups); workgroups % 8 != 0 is the r8 != 0 arm
REMAP = [
    (640, 384, 3, 39),
    (384, 384, 3, 15),
    (1280, 384, 3, 39),
    (896, 384, 5, 100),
    (1024, 384, 3, 24),  # a multiple of 8
    (256, 384, 8, 16),   # a multiple of 8
]

# Lock-step hint (256-tile kernel only): (d_pad, ld, num_splits, stages per split)
LOCKSTEP = [
    (1024, 48 * 13, 2, [7, 6]),
    (512, 48 * 13, 4, [4, 4, 4, 1]),
]
SYNC_EVERY = [0, 1, 2, 64]
