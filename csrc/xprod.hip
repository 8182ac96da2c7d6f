// Dense cross-products in fp64 for gfx950 (MI355X / CDNA4): the step-1 partial result of the
// DAAL covariance / low-order moments / correlation PCA / linear and ridge regression family,
// from one pass over the rows. X [n, d] and an optional second block Y [n, m] (bf16, fp32 or
// fp64 each, unit column stride, any row stride) are read in place and widened in registers; no
// fp64 copy, no shifted copy and no joined [X | Y] copy is built.
//
// Reference: ml/daal daal_cov/densedistri, daal_mom/densedistri, daal_pca/cordensedistr,
// daal_linreg/normaleq, daal_ridgereg (step 1, Double throughout). harp_amd/ops/xprod.py drives
// the kernels and undoes the shift.
//
// gram_kernel<NT>. For the joined row z = [x | y] of width W = d + m <= 256 and a shift c [W]:
//   S = sum (z - c)(z - c)^T, s = sum (z - c), min z, max z.
//  * The width is padded to WP = 16 NT columns (NT = 1 .. 16; padded columns are zero). A
//    workgroup of 8 waves owns ALL NB = NT (NT + 1) / 2 upper 16 x 16 blocks of S in accumulator
//    registers over all of its row chunks, so X is read from HBM exactly once.
//  * The blocks are dealt to the waves as BG block groups x KS k-phases (BG KS = 8): a wave of
//    block group b holds the blocks [b BPW, (b + 1) BPW) of the row-major upper triangle and
//    multiplies the k-steps (four rows each) kw, kw + KS, .. of a chunk. Up to 5 tiles KS = 8:
//    every wave holds every block, the block list is a compile-time one and each operand tile is
//    read once per k-step. Up to 8 tiles KS = 2, beyond KS = 1 (17 blocks = 136 accumulator
//    registers per lane at NT = 16): the wave's block list sits in registers as operand offsets,
//    so all waves run one instruction stream and no accumulator crosses a branch. The KS
//    partial accumulators of a block are added in phase order at the end.
//  * Staging. Thread t owns column t % WP for the rows t / WP, t / WP + TR, .. of a chunk (TR =
//    512 / WP): a wave-instruction reads runs of WP consecutive elements in the input dtype.
//    The loads of chunk k + 1 are issued before the MFMAs of chunk k and land in LDS after them
//    as z - c in fp64 (two buffers, one barrier per chunk). Rows past n are zero in the tile.
//    The column's running s, min and max live in the staging thread's registers.
//  * v_mfma_f64_16x16x4_f64: for block (t1, t2) operand A is columns 16 t1 .. and operand B
//    columns 16 t2 .. of the same four rows of the tile; lane l reads row l >> 4, column l & 15
//    (16 lanes cover one 128-byte run: no bank conflict, no padding). Register r of lane l then
//    holds S[16 t1 + (l >> 4) + 4 r][16 t2 + (l & 15)].
//  * Chunks are dealt statically: workgroup b takes chunks b, b + G, ... One record per
//    workgroup, plain stores: the accumulator fragments [NB][4][64], then s, min, max [WP] each.
//
// moments_kernel: the any-d form without the Gram: per column s, sum (x - c)^2, min, max. A
// workgroup of 256 threads owns a tile of up to 256 columns and the row chunks of its split;
// narrow shapes fold several rows into the workgroup (CW = the power of two >= d columns, 256 /
// CW row phases), eight loads in flight per lane.
//
// reduce kernels: one thread per cell adds the workgroup records in workgroup order (min / max
// by compare) and the Gram one mirrors the upper blocks into the lower triangle: the result is
// bitwise repeatable. A NaN propagates into min and max as torch.min / torch.max do.
#include "common.h"

#define XP_MAX_D 256
#define XP_THREADS 512
#define XP_GRID 512        // gram workgroups while NT <= 5
#define XP_GRID_WIDE 256   // gram workgroups beyond (one fits a CU; the record is large)
#define XP_ELEMS 4096      // staged elements of a chunk, about
#define XM_THREADS 256
#define XM_TILE 256        // columns of a moments workgroup
#define XM_CHUNK 1024      // rows of a moments chunk
#define XM_GRID 512
#define XM_FLIGHT 8

namespace {

typedef double doublex4 __attribute__((ext_vector_type(4)));

// ---- elements: raw bits in, fp64 out -------------------------------------------------------------
// N elements, element i at p + off[i], as raw bits: one branch on the dtype around all the loads
template <int N>
__device__ __forceinline__ void load_raw(uint64_t (&raw)[N], const char* p, const long (&off)[N], int dt) {
  if (dt == 2) {
#pragma unroll
    for (int i = 0; i < N; ++i) raw[i] = *reinterpret_cast<const uint64_t*>(p + off[i]);
  } else if (dt == 1) {
#pragma unroll
    for (int i = 0; i < N; ++i) raw[i] = *reinterpret_cast<const uint32_t*>(p + off[i]);
  } else {
#pragma unroll
    for (int i = 0; i < N; ++i) raw[i] = *reinterpret_cast<const uint16_t*>(p + off[i]);
  }
}
__device__ __forceinline__ double wide(uint64_t raw, int dt) {
  const double a = __longlong_as_double((long long)raw);
  const double b = (double)__uint_as_float((uint32_t)raw);
  const double c = (double)__uint_as_float((uint32_t)raw << 16);
  return dt == 2 ? a : dt == 1 ? b : c;
}
__device__ __forceinline__ int elem_bytes(int dt) { return dt == 2 ? 8 : dt == 1 ? 4 : 2; }

// torch.min / torch.max: the first NaN sticks
__device__ __forceinline__ void take_min(double& m, double v) { m = (v < m || v != v) ? v : m; }
__device__ __forceinline__ void take_max(double& m, double v) { m = (v > m || v != v) ? v : m; }

// row-major upper triangle of NT x NT: unit g -> (t1, t2), t1 <= t2
__host__ __device__ constexpr int unit_row(int g, int nt) {
  int t1 = 0;
  while (g >= nt - t1) {
    g -= nt - t1;
    ++t1;
  }
  return t1;
}
__host__ __device__ constexpr int unit_col(int g, int nt) {
  int t1 = 0;
  while (g >= nt - t1) {
    g -= nt - t1;
    ++t1;
  }
  return t1 + g;
}

template <int NT>
struct Shape {
  static constexpr int WP = 16 * NT;
  static constexpr int NB = NT * (NT + 1) / 2;
  static constexpr int KS = NT <= 5 ? 8 : NT <= 8 ? 2 : 1;                 // k-phases
  static constexpr int BG = 8 / KS;                                        // block groups
  static constexpr int BPW = (NB + BG - 1) / BG;                           // blocks of a wave
  static constexpr int KQ = 4 * KS;                                        // rows of a round of k-steps
  static constexpr int CH = (XP_ELEMS / WP) / KQ > 0 ? (XP_ELEMS / WP) / KQ * KQ : KQ;  // rows of a chunk
  static constexpr int TR = XP_THREADS / WP;                               // row phases of the staging
  static constexpr int RPT = (CH + TR - 1) / TR;                           // rows of a chunk per thread
  static constexpr int TILE = CH * WP;                                     // doubles of one buffer
  static constexpr int FRAG = NB * 256;                                    // doubles of the fragments
  static constexpr int RECORD = FRAG + 3 * WP;
  static constexpr int GRID = NT <= 5 ? XP_GRID : XP_GRID_WIDE;
  static constexpr int EPI = KS > 1 ? BG * BPW * 256 : 0;                  // doubles of the phase merge
  static constexpr int COLS = 3 * TR * WP;
  static constexpr int LDS_D = 2 * TILE > EPI ? (2 * TILE > COLS ? 2 * TILE : COLS) : (EPI > COLS ? EPI : COLS);
  static constexpr int LDS = LDS_D * 8;
  static_assert(CH % KQ == 0 && BPW * 8 <= 144 && LDS <= 160 * 1024, "accumulators and tiles fit");
};

template <int NT, int BGI, int I>
__device__ __forceinline__ void mfma_units(const double* rp, doublex4 (&acc)[Shape<NT>::BPW]) {
  typedef Shape<NT> SH;
  if constexpr (I < SH::BPW && BGI * SH::BPW + I < SH::NB) {
    constexpr int g = BGI * SH::BPW + I;
    constexpr int t1 = unit_row(g, NT), t2 = unit_col(g, NT);
    acc[I] = __builtin_amdgcn_mfma_f64_16x16x4f64(rp[16 * t1], rp[16 * t2], acc[I], 0, 0, 0);
    mfma_units<NT, BGI, I + 1>(rp, acc);
  }
}

template <int NT, int BGI>
__device__ __forceinline__ void mfma_chunk(const double* tile, int kw, int lane, doublex4 (&acc)[Shape<NT>::BPW]) {
  typedef Shape<NT> SH;
  const double* rp = tile + (lane >> 4) * SH::WP + (lane & 15);
#pragma unroll 1
  for (int kk = kw; kk < SH::CH / 4; kk += SH::KS) mfma_units<NT, BGI, 0>(rp + kk * 4 * SH::WP, acc);
}

// the same with the wave's block list in registers (BG > 1): operand offsets oa / ob per slot, so
// the eight waves run one instruction stream and the accumulators never cross a branch
template <int NT>
__device__ __forceinline__ void mfma_listed(const double* tile, int kw, int lane, const int (&oa)[Shape<NT>::BPW],
                                            const int (&ob)[Shape<NT>::BPW], doublex4 (&acc)[Shape<NT>::BPW]) {
  typedef Shape<NT> SH;
  const double* rp = tile + (lane >> 4) * SH::WP + (lane & 15);
#pragma unroll 1
  for (int kk = kw; kk < SH::CH / 4; kk += SH::KS) {
    const double* q = rp + kk * 4 * SH::WP;
#pragma unroll
    for (int i = 0; i < SH::BPW; ++i)
      acc[i] = __builtin_amdgcn_mfma_f64_16x16x4f64(q[oa[i]], q[ob[i]], acc[i], 0, 0, 0);
  }
}

template <int NT>
__global__ __launch_bounds__(XP_THREADS) void gram_kernel(const char* __restrict__ X, int dtx, long ldx, int d,
                                                          const char* __restrict__ Y, int dty, long ldy, int m,
                                                          long n, const double* __restrict__ c,
                                                          double* __restrict__ partial) {
  typedef Shape<NT> SH;
  extern __shared__ __attribute__((aligned(16))) double lds[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int bg = wv / SH::KS, kw = wv % SH::KS;

  // the staging thread's column
  const int tc = tid % SH::WP, tr = tid / SH::WP;
  const bool staging = tr < SH::TR;
  const bool in_x = tc < d, live = staging && tc < d + m;
  const int dt = in_x || !live ? dtx : dty;
  const long stride = (in_x || !live ? ldx : ldy) * elem_bytes(dt);
  const char* base = !live ? X : in_x ? X + (long)tc * elem_bytes(dt) : Y + (long)(tc - d) * elem_bytes(dt);
  const double cc = live ? c[tc] : 0.0;
  double s = 0.0, mn = __builtin_inf(), mx = -__builtin_inf();

  const long nchunks = (n + SH::CH - 1) / SH::CH;
  uint64_t raw[SH::RPT];
  auto fetch = [&](long k) {
    const long r0 = k * SH::CH;
    long off[SH::RPT];
#pragma unroll
    for (int i = 0; i < SH::RPT; ++i) {
      const int row = tr + i * SH::TR;
      const bool ok = live && row < SH::CH && r0 + row < n;
      off[i] = ok ? (r0 + row) * stride : 0;  // out of range: a valid address, the value dropped
    }
    load_raw(raw, base, off, dt);
  };
  auto stash = [&](double* tile, long k) {
    const long r0 = k * SH::CH;
#pragma unroll
    for (int i = 0; i < SH::RPT; ++i) {
      const int row = tr + i * SH::TR;
      const bool ok = live && row < SH::CH && r0 + row < n;
      const double v = wide(raw[i], dt);
      const double z = ok ? v - cc : 0.0;
      if (staging && row < SH::CH) tile[row * SH::WP + tc] = z;
      s += z;
      if (ok) {
        take_min(mn, v);
        take_max(mx, v);
      }
    }
  };

  doublex4 acc[SH::BPW];
  int oa[SH::BPW], ob[SH::BPW];  // a slot past the last block repeats block 0 and is never stored
#pragma unroll
  for (int i = 0; i < SH::BPW; ++i) {
    acc[i] = doublex4{0.0, 0.0, 0.0, 0.0};
    const int g = bg * SH::BPW + i < SH::NB ? bg * SH::BPW + i : 0;
    oa[i] = 16 * unit_row(g, NT);
    ob[i] = 16 * unit_col(g, NT);
  }

  long k = blockIdx.x;
  int buf = 0;
  fetch(k);
  stash(lds, k);
  __syncthreads();
  for (; k < nchunks; k += gridDim.x) {
    const long kn = k + gridDim.x;
    const bool more = kn < nchunks;
    if (more) fetch(kn);
    if constexpr (SH::BG == 1)
      mfma_chunk<NT, 0>(lds + buf * SH::TILE, kw, lane, acc);
    else
      mfma_listed<NT>(lds + buf * SH::TILE, kw, lane, oa, ob, acc);
    if (more) stash(lds + (buf ^ 1) * SH::TILE, kn);
    __syncthreads();
    buf ^= 1;
  }

  double* out = partial + (long)blockIdx.x * SH::RECORD;
  // the columns: the row phases in order
  if (staging) {
    lds[(0 * SH::TR + tr) * SH::WP + tc] = s;
    lds[(1 * SH::TR + tr) * SH::WP + tc] = mn;
    lds[(2 * SH::TR + tr) * SH::WP + tc] = mx;
  }
  __syncthreads();
  if (tid < SH::WP) {
    double a = 0.0, lo = __builtin_inf(), hi = -__builtin_inf();
    for (int q = 0; q < SH::TR; ++q) {
      a += lds[(0 * SH::TR + q) * SH::WP + tid];
      take_min(lo, lds[(1 * SH::TR + q) * SH::WP + tid]);
      take_max(hi, lds[(2 * SH::TR + q) * SH::WP + tid]);
    }
    out[SH::FRAG + tid] = a;
    out[SH::FRAG + SH::WP + tid] = lo;
    out[SH::FRAG + 2 * SH::WP + tid] = hi;
  }
  // the blocks: the k-phases of a block group in order, then the fragments as they lie
  if constexpr (SH::KS > 1) {
    double* mine = lds + bg * SH::BPW * 256 + lane;
    for (int ks = 1; ks < SH::KS; ++ks) {
      __syncthreads();
      if (kw == ks) {
#pragma unroll
        for (int i = 0; i < SH::BPW; ++i)
#pragma unroll
          for (int r = 0; r < 4; ++r) mine[(i * 4 + r) * 64] = acc[i][r];
      }
      __syncthreads();
      if (kw == 0) {
#pragma unroll
        for (int i = 0; i < SH::BPW; ++i)
#pragma unroll
          for (int r = 0; r < 4; ++r) acc[i][r] += mine[(i * 4 + r) * 64];
      }
    }
  }
  if (kw == 0) {
#pragma unroll
    for (int i = 0; i < SH::BPW; ++i) {
      const int g = bg * SH::BPW + i;
      if (g < SH::NB) {
#pragma unroll
        for (int r = 0; r < 4; ++r) out[(g * 4 + r) * 64 + lane] = acc[i][r];
      }
    }
  }
}

// out = xtx [W, W], then sum, min, max [W] each, from nb records of gram_kernel<nt>
__global__ __launch_bounds__(256) void gram_reduce_kernel(const double* __restrict__ partial, int nb, int nt, int W,
                                                          double* __restrict__ out) {
  const int wp = 16 * nt, frag = nt * (nt + 1) / 2 * 256, len = frag + 3 * wp;
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e >= len) return;
  const double* p = partial + e;
  if (e < frag) {
    double a = 0.0;
    for (int b = 0; b < nb; ++b) a += p[(long)b * len];
    const int g = e >> 8, r = (e >> 6) & 3, l = e & 63;
    const int t1 = unit_row(g, nt), t2 = unit_col(g, nt);
    const int i = 16 * t1 + (l >> 4) + 4 * r, j = 16 * t2 + (l & 15);
    if (i < W && j < W) {
      out[(long)i * W + j] = a;
      if (t1 != t2) out[(long)j * W + i] = a;
    }
    return;
  }
  const int sec = (e - frag) / wp, col = (e - frag) % wp;
  if (col >= W) return;
  double a = sec == 0 ? 0.0 : sec == 1 ? __builtin_inf() : -__builtin_inf();
  for (int b = 0; b < nb; ++b) {
    const double v = p[(long)b * len];
    if (sec == 0) a += v;
    else if (sec == 1) take_min(a, v);
    else take_max(a, v);
  }
  out[(long)W * W + (long)sec * W + col] = a;
}

// ---- the any-d moments form ----------------------------------------------------------------------
inline int mom_tiles(int d) { return (d + XM_TILE - 1) / XM_TILE; }
inline int mom_splits(long n, int d) {
  const long chunks = (n + XM_CHUNK - 1) / XM_CHUNK;
  const long cap = XM_GRID / mom_tiles(d) > 0 ? XM_GRID / mom_tiles(d) : 1;
  return (int)(chunks < cap ? (chunks > 0 ? chunks : 1) : cap);
}
inline int mom_shift(int d) {  // log2 of the columns of a row phase
  int sh = 4;
  while (sh < 8 && (1 << sh) < d) ++sh;
  return sh;
}

// partial [splits, 4, d]: s, sum (x - c)^2, min, max of each split's rows
__global__ __launch_bounds__(XM_THREADS) void moments_kernel(const char* __restrict__ X, int dt, long ldx, int d,
                                                             long n, const double* __restrict__ c, int sh,
                                                             int splits, double* __restrict__ partial) {
  __shared__ double red[4][XM_THREADS];
  const int tid = threadIdx.x, split = blockIdx.y;
  const int tc = tid & ((1 << sh) - 1), tr = tid >> sh, phases = XM_THREADS >> sh;
  const int col = blockIdx.x * XM_TILE + tc;
  const bool live = col < d;
  const long stride = ldx * elem_bytes(dt);
  const char* base = X + (live ? (long)col * elem_bytes(dt) : 0);
  const double cc = live ? c[col] : 0.0;
  double s = 0.0, q = 0.0, mn = __builtin_inf(), mx = -__builtin_inf();
  const long chunks = (n + XM_CHUNK - 1) / XM_CHUNK;
  for (long k = split; k < chunks; k += splits) {
    const long r1 = (k + 1) * XM_CHUNK < n ? (k + 1) * XM_CHUNK : n;
    for (long r = k * XM_CHUNK + tr; r < r1; r += (long)XM_FLIGHT * phases) {
      uint64_t raw[XM_FLIGHT];
      long off[XM_FLIGHT];
#pragma unroll
      for (int i = 0; i < XM_FLIGHT; ++i) {
        const long row = r + (long)i * phases;
        off[i] = row < r1 ? row * stride : 0;
      }
      load_raw(raw, base, off, dt);
#pragma unroll
      for (int i = 0; i < XM_FLIGHT; ++i) {
        const bool ok = live && r + (long)i * phases < r1;
        const double v = wide(raw[i], dt);
        const double z = ok ? v - cc : 0.0;
        s += z;
        q = fma(z, z, q);
        if (ok) {
          take_min(mn, v);
          take_max(mx, v);
        }
      }
    }
  }
  red[0][tid] = s;
  red[1][tid] = q;
  red[2][tid] = mn;
  red[3][tid] = mx;
  __syncthreads();
  if (tr == 0 && live) {
    double a = 0.0, b = 0.0, lo = __builtin_inf(), hi = -__builtin_inf();
    for (int p = 0; p < phases; ++p) {
      const int t = (p << sh) + tc;
      a += red[0][t];
      b += red[1][t];
      take_min(lo, red[2][t]);
      take_max(hi, red[3][t]);
    }
    double* out = partial + (long)split * 4 * d + col;
    out[0] = a;
    out[d] = b;
    out[2L * d] = lo;
    out[3L * d] = hi;
  }
}

// out [4, d] = the splits of partial in split order
__global__ __launch_bounds__(256) void moments_reduce_kernel(const double* __restrict__ partial, int splits, int d,
                                                             double* __restrict__ out) {
  const long e = (long)blockIdx.x * 256 + threadIdx.x;
  if (e >= 4L * d) return;
  const int sec = (int)(e / d);
  double a = sec < 2 ? 0.0 : sec == 2 ? __builtin_inf() : -__builtin_inf();
  for (int k = 0; k < splits; ++k) {
    const double v = partial[(long)k * 4 * d + e];
    if (sec < 2) a += v;
    else if (sec == 2) take_min(a, v);
    else take_max(a, v);
  }
  out[e] = a;
}

inline long gram_chunks(long n, int nt) {
  const int wp = 16 * nt, ks = nt <= 5 ? 8 : nt <= 8 ? 2 : 1;
  const int ch = (XP_ELEMS / wp) / (4 * ks) > 0 ? (XP_ELEMS / wp) / (4 * ks) * (4 * ks) : 4 * ks;
  return (n + ch - 1) / ch;
}
inline int gram_grid(long n, int nt) {
  const long chunks = gram_chunks(n, nt), cap = nt <= 5 ? XP_GRID : XP_GRID_WIDE;
  return (int)(chunks < cap ? chunks : cap);
}

template <int NT>
int launch_gram(const void* X, int dtx, long ldx, int d, const void* Y, int dty, long ldy, int m, long n,
                const double* c, double* partial, hipStream_t s) {
  typedef Shape<NT> SH;
  static_assert(SH::GRID == (NT <= 5 ? XP_GRID : XP_GRID_WIDE), "gram_grid mirrors Shape");
  if (SH::LDS > 65536 && hipFuncSetAttribute((const void*)gram_kernel<NT>,
                                             hipFuncAttributeMaxDynamicSharedMemorySize, SH::LDS) != hipSuccess)
    return HARP_ELAUNCH;
  if (gram_chunks(n, NT) != (n + SH::CH - 1) / SH::CH) return HARP_ELAUNCH;
  gram_kernel<NT><<<dim3((unsigned)gram_grid(n, NT)), dim3(XP_THREADS), SH::LDS, s>>>(
      (const char*)X, dtx, ldx, d, (const char*)(m ? Y : X), m ? dty : dtx, m ? ldy : ldx, m, n, c, partial);
  return harp_launch_status();
}

}  // namespace

HARP_EXPORT int harp_xprod_max_d() { return XP_MAX_D; }

// Workgroups (= records) of harp_xprod_pass for n rows of joined width w (0: a shape it rejects)
HARP_EXPORT int harp_xprod_grid(long n, int w) {
  if (n < 1 || w < 1 || w > XP_MAX_D) return 0;
  return gram_grid(n, (w + 15) / 16);
}

// Doubles of one workgroup record of harp_xprod_pass at joined width w (0: a width it rejects)
HARP_EXPORT int harp_xprod_record(int w) {
  if (w < 1 || w > XP_MAX_D) return 0;
  const int nt = (w + 15) / 16;
  return nt * (nt + 1) / 2 * 256 + 3 * 16 * nt;
}

// partial [harp_xprod_grid(n, d + m), harp_xprod_record(d + m)] (fp64, every element written) =
// the per-workgroup S, s, min and max of the joined rows [X | Y] shifted by c [d + m] (fp64). X
// [n, d] and Y [n, m] (m = 0: no second block): dtype 0 bf16 / 1 fp32 / 2 fp64, unit column
// stride, row strides ldx >= d and ldy >= m elements, n > 0.
HARP_EXPORT int harp_xprod_pass(const void* X, int dtx, long ldx, int d, const void* Y, int dty, long ldy, int m,
                                long n, const double* c, double* partial, hipStream_t s) {
  if (n < 1 || d < 1 || m < 0 || ldx < d || !X || !c || !partial || (m > 0 && (!Y || ldy < m))) return HARP_EBADARG;
  if (d + m > XP_MAX_D || dtx < 0 || dtx > 2 || (m > 0 && (dty < 0 || dty > 2))) return HARP_EUNSUPPORTED;
  switch ((d + m + 15) / 16) {
#define XP_CASE(NT) \
  case NT: return launch_gram<NT>(X, dtx, ldx, d, Y, dty, ldy, m, n, c, partial, s);
    XP_CASE(1) XP_CASE(2) XP_CASE(3) XP_CASE(4) XP_CASE(5) XP_CASE(6) XP_CASE(7) XP_CASE(8)
    XP_CASE(9) XP_CASE(10) XP_CASE(11) XP_CASE(12) XP_CASE(13) XP_CASE(14) XP_CASE(15) XP_CASE(16)
#undef XP_CASE
  }
  return HARP_EUNSUPPORTED;
}

// out = xtx [w, w] (both triangles), then sum, min, max [w] each (fp64, every element written) =
// the records of harp_xprod_pass combined in workgroup order
HARP_EXPORT int harp_xprod_reduce(const double* partial, int records, int w, double* out, hipStream_t s) {
  if (!partial || !out || records < 1 || w < 1 || w > XP_MAX_D) return HARP_EBADARG;
  const int nt = (w + 15) / 16;
  const int len = harp_xprod_record(w);
  gram_reduce_kernel<<<dim3((unsigned)((len + 255) / 256)), dim3(256), 0, s>>>(partial, records, nt, w, out);
  return harp_launch_status();
}

// Row splits of harp_xprod_moments for n rows of d columns (0: a shape it rejects). The partial
// buffer holds splits * 4 * d doubles.
HARP_EXPORT int harp_xprod_splits(long n, int d) {
  if (n < 1 || d < 1) return 0;
  return mom_splits(n, d);
}

// partial [splits, 4, d] = s, sum (x - c)^2, min, max per column of each split's rows of X [n, d]
// (as above, any d) shifted by c [d]
HARP_EXPORT int harp_xprod_moments(const void* X, int dt, long ldx, int d, long n, const double* c, double* partial,
                                   hipStream_t s) {
  if (n < 1 || d < 1 || ldx < d || !X || !c || !partial) return HARP_EBADARG;
  if (dt < 0 || dt > 2 || mom_tiles(d) > 65535) return HARP_EUNSUPPORTED;
  const int splits = mom_splits(n, d);
  moments_kernel<<<dim3((unsigned)mom_tiles(d), (unsigned)splits), dim3(XM_THREADS), 0, s>>>(
      (const char*)X, dt, ldx, d, n, c, mom_shift(d), splits, partial);
  return harp_launch_status();
}

// out [4, d] = the splits of partial combined in split order
HARP_EXPORT int harp_xprod_moments_reduce(const double* partial, int splits, int d, double* out, hipStream_t s) {
  if (!partial || !out || splits < 1 || d < 1) return HARP_EBADARG;
  moments_reduce_kernel<<<dim3((unsigned)((4L * d + 255) / 256)), dim3(256), 0, s>>>(partial, splits, d, out);
  return harp_launch_status();
}
