// Outlier detection for gfx950 (MI355X / CDNA4): one fused Mahalanobis pass and an elementwise
// univariate pass.
//
// Reference: ml/daal daal_outlier {unidensebatch, multidensebatch, bacondensebatch} (DAAL
// univariate_outlier_detection, multivariate_outlier_detection, bacon_outlier_detection).
// harp_amd/ops/outlier.py drives the kernels and holds the fp64 torch mirror of the pass (the
// gloo path and the oracle of tests/test_outlier_gpu.py).
//
// pass_kernel. Per row: dist2 = ||P (x - c)||^2 with P = L^-1 the packed lower triangle of the
// whitening matrix (or the identity), member = dist2 < t2 (or <=). Over the members: their count,
// sum (x - s) and the upper triangle of sum (x - s)(x - s)^T; over all rows: how many mask bytes
// flipped. X (bf16 / fp32 / fp64) is read in place through its row stride and widened in
// registers; nothing of size [n, d] is written.
//
//  * A fixed grid of at most OUTLIER_GRID workgroups of four waves; chunk k (OUTLIER_CHUNK rows)
//    belongs to workgroup k mod grid, a wave owns 64 rows of it, a lane one row. No work counter
//    and no atomics: every sum has one fixed order, so a record is bitwise repeatable.
//  * Load. The wave's 64 rows are read as consecutive elements (lane l takes element 64 i + l of
//    the 64 d, so a wave-instruction reads 64 consecutive elements whatever d, the row stride and
//    the alignment are), go through LDS in the input dtype and come back one row per lane. The
//    loads of the workgroup's next chunk are issued before the current one is computed, where
//    the registers allow (every form but fp64 at width 64).
//  * Distance, the gmm_estep_kernel form: the row in registers, P through scalar loads in groups
//    of sixteen that run one group ahead of the FMAs, all indices compile-time for the padded
//    width D (8, 16, 32, 64). Rows of P past d add nothing.
//  * Statistics. Every lane writes x - s to its row of the wave's fp64 LDS tile before the
//    distance is known and a lane that turns out to be no member zeroes its row after (weights
//    0 / 1: exact, and a NaN or infinite row never reaches a sum). The Gram matrix is then
//    v_mfma_f64_16x16x4_f64 over the tile: for column tiles t1 <= t2 both operands are one
//    ds_read_b64 per lane (A[i = lane & 15][k = lane >> 4], B[k = lane >> 4][j = lane & 15]), 16
//    steps of 4 rows, result (row (lane >> 4) + 4 r, column lane & 15) in register r. The
//    accumulators stay in registers over all of the workgroup's chunks. Column sums are read
//    off the same tile, 64 / TW lanes per column. flags bit 0 selects the other form that was
//    measured, 4 x 4 coordinate blocks on the vector FMAs (gmm_stats_blk_kernel with one
//    component): profiles/outlier has both numbers.
//  * Epilogue. The four waves' accumulators meet in LDS, are added in wave order and stored as
//    the workgroup's row of partial [grid, 2 + d + d (d + 1) / 2]: count and changed as int64
//    bit patterns, then the sums, then the upper triangle row by row.
//
// reduce_kernel: one thread per statistic adds the partial rows in workgroup order.
//
// univariate_kernel: w = |(double)x - loc_j| / max(sc_j, 1e-300) <= thr in X's dtype; IEEE fp64
// subtract, divide and compare, so it equals the torch expression on every element.
//
// All stores are vector stores; no kernel waits on another workgroup.
#include "common.h"

#include <utility>

// Nothing here may fuse a multiply into an add on its own: the univariate weights have to equal
// the torch expression bit for bit. The FMAs of the distance are written as fma().
#pragma clang fp contract(off)

#define OUTLIER_THREADS 256
#define OUTLIER_CHUNK 256  // rows of a chunk: one per thread
#define OUTLIER_GRID 512   // workgroups (two per CU)
#define OUTLIER_MAX_D 64
#define OUTLIER_UNI_SPAN 4096  // elements of one univariate workgroup

namespace {

typedef double doublex4 __attribute__((ext_vector_type(4)));
typedef double doublex2 __attribute__((ext_vector_type(2)));

struct InBf16 {
  typedef uint16_t L;
  static __device__ __forceinline__ double wide(L v) { return (double)__uint_as_float((uint32_t)v << 16); }
  static __device__ __forceinline__ L weight(bool w) { return w ? (L)0x3F80 : (L)0; }
};
struct InFp32 {
  typedef float L;
  static __device__ __forceinline__ double wide(L v) { return (double)v; }
  static __device__ __forceinline__ L weight(bool w) { return w ? 1.0f : 0.0f; }
};
struct InFp64 {
  typedef double L;
  static __device__ __forceinline__ double wide(L v) { return v; }
  static __device__ __forceinline__ L weight(bool w) { return w ? 1.0 : 0.0; }
};

// ---- distance: the packed lower triangle, row i = [P_i0 .. P_ii] at i (i + 1) / 2 -------------
constexpr int tri_start(int i) { return i * (i + 1) / 2; }
constexpr int tri_row(int e) {
  int i = 0;
  while (tri_start(i + 1) <= e) ++i;
  return i;
}
constexpr int kLoad = 16;  // doubles per scalar load group

struct DistAcc {
  double za, zb, d2;
};

// pins the accumulators here and orders later loads after it (gmm.hip: without it all scalar
// loads are issued first and the SGPRs spill through lane moves)
__device__ __forceinline__ void pin(DistAcc& a) { asm volatile("" : "+v"(a.za), "+v"(a.zb), "+v"(a.d2)::"memory"); }

template <int D, int E>
__device__ __forceinline__ void tri_elem(double v, const double (&y)[D], DistAcc& a, int d) {
  if constexpr (E < tri_start(D)) {
    constexpr int i = tri_row(E), j = E - tri_start(i);
    if constexpr (j == 0)
      a.za = v * y[0];
    else if constexpr (j == 1)
      a.zb = v * y[1];
    else if constexpr (j % 2 == 0)
      a.za = fma(v, y[j], a.za);
    else
      a.zb = fma(v, y[j], a.zb);
    if constexpr (j == i) {  // row i is complete; a padding row (zeros times the row) is dropped
      const double z = i == 0 ? a.za : a.za + a.zb;
      const double t = fma(z, z, a.d2);
      a.d2 = i < d ? t : a.d2;
    }
  }
}

template <int D, int C, int... Us>
__device__ __forceinline__ void tri_chunk(const double (&v)[kLoad], const double (&y)[D], DistAcc& a, int d,
                                          std::integer_sequence<int, Us...>) {
  (tri_elem<D, C * kLoad + Us>(v[Us], y, a, d), ...);
}

template <int D, int C>
__device__ __forceinline__ void tri_pipe(const double* __restrict__ P, const double (&cur)[kLoad],
                                         const double (&y)[D], DistAcc& a, int d) {
  constexpr int NC = (tri_start(D) + kLoad - 1) / kLoad;
  if constexpr (C < NC) {
    double nxt[kLoad];
    if constexpr (C + 1 < NC) {
#pragma unroll
      for (int u = 0; u < kLoad; ++u) nxt[u] = P[(C + 1) * kLoad + u];
    }
    tri_chunk<D, C>(cur, y, a, d, std::make_integer_sequence<int, kLoad>{});
    pin(a);
    tri_pipe<D, C + 1>(P, nxt, y, a, d);
  }
}

// ---- the pass ---------------------------------------------------------------------------------
// FORM 0: fp64 MFMA Gram; FORM 1: 4 x 4 coordinate blocks on the vector FMAs.
template <int TW, int FORM>
struct StatsShape;
template <int TW>
struct StatsShape<TW, 0> {
  static constexpr int NT = TW / 16;               // column tiles
  static constexpr int UNITS = NT * (NT + 1) / 2;  // 16 x 16 tiles of the upper triangle
  static constexpr int PER_LANE = UNITS;           // a lane holds 4 results of every tile
  static constexpr int VALS = 4;
};
template <int TW>
struct StatsShape<TW, 1> {
  static constexpr int NB = TW / 4;                // coordinate blocks
  static constexpr int UNITS = NB * (NB + 1) / 2;  // 4 x 4 pair-blocks of the upper triangle
  static constexpr int PER_LANE = (UNITS + 63) / 64;
  static constexpr int VALS = 16;
};

// unit u of the upper triangle of an N x N grid of blocks, row by row -> (bi, bj)
__device__ __forceinline__ void upper_unit(int u, int N, int& bi, int& bj) {
  bi = 0;
  while (u >= N - bi) {
    u -= N - bi;
    ++bi;
  }
  bj = bi + u;
}

// A zero and a lane id the compiler cannot see through. P, c, s and the element-to-row maps do
// not change from chunk to chunk, and hoisted out of the chunk loop they would take thousands of
// registers: the zero is added to the pointers and the lane id re-read inside the loop.
__device__ __forceinline__ long opaque_zero() {
  long z = 0;
  asm volatile("" : "+s"(z));
  return z;
}
__device__ __forceinline__ int opaque(int v) {
  asm volatile("" : "+v"(v));
  return v;
}

// Element it * 64 + lane of the wave's 64 rows (r0 ..), read as one run of 64 d elements. The
// loads are unconditional: an element past the wave's last row inside the block reads the
// wave's first element instead (a wave wholly past the end, X's), and the row it lands in is
// never a member.
template <typename F, int D>
__device__ __forceinline__ void load_rows(typename F::L (&v)[D], const typename F::L* __restrict__ X, long n,
                                          long ldx, int d, unsigned magic, long r0, int lane) {
  const long left = n - r0;
  const int rows = left <= 0 ? 0 : left >= 64 ? 64 : (int)left;
  const typename F::L* base = rows ? X + r0 * ldx : X;
  const int limit = rows * d, skip = (int)(ldx - d);
  const int l = opaque(lane);
#pragma unroll
  for (int it = 0; it < D; ++it) {
    if (it < d) {  // uniform
      const int e = it * 64 + l;
      const int row = (int)(((unsigned)e * magic) >> 20);  // e / d for e < 4096, d <= 64
      const int off = e + row * skip;
      v[it] = base[e < limit ? off : 0];
    }
  }
}

template <typename F, int D, int FORM>
__global__ __launch_bounds__(OUTLIER_THREADS) void pass_kernel(
    const typename F::L* __restrict__ X, long n, long ldx, int d, const double* __restrict__ cs,
    const double* __restrict__ P, int identity, double t2, int strict, unsigned char* __restrict__ mask,
    double* __restrict__ dist2, int stats, double* __restrict__ partial) {
  typedef typename F::L L;
  typedef StatsShape<(D < 16 ? 16 : D), FORM> SH;
  constexpr int TW = D < 16 ? 16 : D;  // columns of the fp64 tile
  constexpr int TS = TW + 2;           // its row stride in doubles (16-byte rows, banks spread)
  constexpr int SS = sizeof(L) == 2 ? TW + 2 : TW + 1;  // row stride of the staged input, elements
  constexpr int REGION = 64 * TS;      // doubles of one wave
  constexpr bool PREFETCH = sizeof(L) * D <= 256;
  static_assert(64 * SS * sizeof(L) <= REGION * sizeof(double), "staging fits the tile");
  static_assert(SH::PER_LANE * SH::VALS * 64 + 64 <= REGION, "the epilogue fits the tile");
  __shared__ __attribute__((aligned(16))) double lds[4 * REGION];
  __shared__ long long cnt_lds[2][4];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  double* tile = lds + wv * REGION;
  L* stage = reinterpret_cast<L*>(tile);
  const long nchunks = (n + OUTLIER_CHUNK - 1) / OUTLIER_CHUNK;
  const unsigned magic = ((1u << 20) + (unsigned)d - 1) / (unsigned)d;

  double acc[SH::PER_LANE][SH::VALS];
#pragma unroll
  for (int g = 0; g < SH::PER_LANE; ++g)
#pragma unroll
    for (int r = 0; r < SH::VALS; ++r) acc[g][r] = 0.0;
  double sacc = 0.0;
  int cnt = 0, chg = 0;

  L v[D];
  long k = blockIdx.x;
  if (k < nchunks) load_rows<F, D>(v, X, n, ldx, d, magic, k * OUTLIER_CHUNK + wv * 64, lane);
  for (; k < nchunks; k += gridDim.x) {
    const long r0 = k * OUTLIER_CHUNK + wv * 64;  // the wave's first row
    const long kn = k + gridDim.x;
    // the wave's rows, as loaded, to LDS; back one row per lane
    {
      const int l = opaque(lane);
#pragma unroll
      for (int it = 0; it < D; ++it) {
        if (it < d) {
          const int e = it * 64 + l;
          const int row = (int)(((unsigned)e * magic) >> 20);
          stage[e + row * (SS - d)] = v[it];  // row * SS + column
        }
      }
    }
    lds_sync_wave();
    double x[D];
#pragma unroll
    for (int j = 0; j < D; ++j) {
      const L raw = stage[lane * SS + (j < d ? j : 0)];
      x[j] = j < d ? F::wide(raw) : 0.0;
    }
    lds_sync_wave();
    if (PREFETCH && kn < nchunks) load_rows<F, D>(v, X, n, ldx, d, magic, kn * OUTLIER_CHUNK + wv * 64, lane);

    // x - s to the tile (every lane; non-members are zeroed below), then x - c in place; c and s
    // through scalar loads, a group at a time
    const long zero = opaque_zero();
    const double* __restrict__ cz = cs + zero;
    const double* __restrict__ Pz = P + zero;
    if (stats) {
#pragma unroll
      for (int j = 0; j < TW; j += 2) {
        doublex2 u;
        u[0] = j < D ? x[j < D ? j : 0] - cz[OUTLIER_MAX_D + (j < D ? j : 0)] : 0.0;
        u[1] = j + 1 < D ? x[j + 1 < D ? j + 1 : 0] - cz[OUTLIER_MAX_D + (j + 1 < D ? j + 1 : 0)] : 0.0;
        *reinterpret_cast<doublex2*>(tile + lane * TS + j) = u;
        if (j % kLoad == kLoad - 2) asm volatile("" ::: "memory");
      }
    }
#pragma unroll
    for (int j = 0; j < D; ++j) {
      x[j] = x[j] - cz[j];
      if (j % kLoad == kLoad - 1) asm volatile("" ::: "memory");
    }

    double d2;
    if (identity) {
      double qa = 0.0, qb = 0.0;
#pragma unroll
      for (int j = 0; j < D; j += 2) {
        qa = fma(x[j], x[j], qa);
        qb = fma(x[j + 1], x[j + 1], qb);
      }
      d2 = qa + qb;
    } else {
      DistAcc a;
      a.za = a.zb = a.d2 = 0.0;
      double first[kLoad];
#pragma unroll
      for (int u = 0; u < kLoad; ++u) first[u] = Pz[u];
      tri_pipe<D, 0>(Pz, first, x, a, d);
      d2 = a.d2;
    }
    const long row = r0 + lane;
    const bool valid = row < n;
    const bool member = valid && (strict ? d2 < t2 : d2 <= t2);
    if (valid) {
      if (dist2) dist2[row] = d2;
      if (mask) {
        chg += ((mask[row] != 0) != member) ? 1 : 0;
        mask[row] = member ? 1 : 0;
      }
    }
    cnt += member ? 1 : 0;

    if (stats) {
      if (!member) {
#pragma unroll
        for (int j = 0; j < TW; j += 2) {
          doublex2 z;
          z[0] = 0.0;
          z[1] = 0.0;
          *reinterpret_cast<doublex2*>(tile + lane * TS + j) = z;
        }
      }
      lds_sync_wave();
      if constexpr (FORM == 0) {
        const double* rp = tile + (lane >> 4) * TS + (lane & 15);
#pragma unroll 2
        for (int kk = 0; kk < 16; ++kk) {
          double a[SH::NT];
#pragma unroll
          for (int t = 0; t < SH::NT; ++t) a[t] = rp[kk * 4 * TS + 16 * t];
          int g = 0;
#pragma unroll
          for (int t1 = 0; t1 < SH::NT; ++t1)
#pragma unroll
            for (int t2 = t1; t2 < SH::NT; ++t2) {
              doublex4 c;
#pragma unroll
              for (int r = 0; r < 4; ++r) c[r] = acc[g][r];
              c = __builtin_amdgcn_mfma_f64_16x16x4f64(a[t1], a[t2], c, 0, 0, 0);
#pragma unroll
              for (int r = 0; r < 4; ++r) acc[g][r] = c[r];
              ++g;
            }
        }
      } else {
        // lane's pair-blocks lane, lane + 64, ..: 4 coordinates of each side per row, 16 FMAs
#pragma unroll
        for (int g = 0; g < SH::PER_LANE; ++g) {
          const int u = lane + 64 * g;
          if (u < SH::UNITS) {
            int bi, bj;
            upper_unit(u, SH::NB, bi, bj);
            const double* pi = tile + 4 * bi;
            const double* pj = tile + 4 * bj;
#pragma unroll 4
            for (int r = 0; r < 64; ++r) {
              const doublex2 i0 = *reinterpret_cast<const doublex2*>(pi + r * TS);
              const doublex2 i1 = *reinterpret_cast<const doublex2*>(pi + r * TS + 2);
              const doublex2 j0 = *reinterpret_cast<const doublex2*>(pj + r * TS);
              const doublex2 j1 = *reinterpret_cast<const doublex2*>(pj + r * TS + 2);
              const double xi[4] = {i0[0], i0[1], i1[0], i1[1]};
              const double xj[4] = {j0[0], j0[1], j1[0], j1[1]};
#pragma unroll
              for (int a = 0; a < 4; ++a)
#pragma unroll
                for (int b = 0; b < 4; ++b) acc[g][a * 4 + b] = fma(xi[a], xj[b], acc[g][a * 4 + b]);
            }
          }
        }
      }
      {  // column sums: lane's column lane % TW over rows (lane / TW) TW .. + TW
        const double* cp = tile + (lane / TW) * TW * TS + (lane % TW);
        double s0 = 0.0, s1 = 0.0;
#pragma unroll 8
        for (int r = 0; r < TW; r += 2) {
          s0 += cp[r * TS];
          s1 += cp[(r + 1) * TS];
        }
        sacc += s0 + s1;
      }
      lds_sync_wave();
    }
    if (!PREFETCH && kn < nchunks) load_rows<F, D>(v, X, n, ldx, d, magic, kn * OUTLIER_CHUNK + wv * 64, lane);
  }

  // ---- the workgroup's partial row: the four waves' accumulators added in wave order ----------
  cnt = wave_sum_i(cnt);
  chg = wave_sum_i(chg);
  __syncthreads();
#pragma unroll
  for (int g = 0; g < SH::PER_LANE; ++g)
#pragma unroll
    for (int r = 0; r < SH::VALS; ++r) tile[(g * SH::VALS + r) * 64 + lane] = acc[g][r];
  tile[SH::PER_LANE * SH::VALS * 64 + lane] = sacc;
  if (lane == 0) {
    cnt_lds[0][wv] = cnt;
    cnt_lds[1][wv] = chg;
  }
  __syncthreads();
  double* out = partial + (long)blockIdx.x * (2 + d + tri_start(d));
  if (tid < 2) out[tid] = __longlong_as_double(cnt_lds[tid][0] + cnt_lds[tid][1] + cnt_lds[tid][2] + cnt_lds[tid][3]);
  if (tid < d) {
    double s = 0.0;
    for (int w = 0; w < 4; ++w)
      for (int q = 0; q < 64 / TW; ++q) s += lds[w * REGION + SH::PER_LANE * SH::VALS * 64 + q * TW + tid];
    out[2 + tid] = s;
  }
  double* gram = out + 2 + d;
  for (int e = tid; e < SH::PER_LANE * SH::VALS * 64; e += OUTLIER_THREADS) {
    const double s = ((lds[e] + lds[REGION + e]) + lds[2 * REGION + e]) + lds[3 * REGION + e];
    const int l = e & 63, r = (e >> 6) % SH::VALS, g = (e >> 6) / SH::VALS;
    int i, j;
    if constexpr (FORM == 0) {
      int t1, t2;
      upper_unit(g, SH::NT, t1, t2);
      i = 16 * t1 + (l >> 4) + 4 * r;
      j = 16 * t2 + (l & 15);
    } else {
      const int u = l + 64 * g;
      if (u >= SH::UNITS) continue;
      int bi, bj;
      upper_unit(u, SH::NB, bi, bj);
      i = 4 * bi + (r >> 2);
      j = 4 * bj + (r & 3);
    }
    if (i <= j && j < d) gram[i * d - i * (i - 1) / 2 + (j - i)] = s;
  }
}

// record[t] = sum over the nb partial rows, in row order; the two counters as int64
__global__ __launch_bounds__(256) void reduce_kernel(const double* __restrict__ partial, int nb, int len,
                                                     double* __restrict__ record) {
  const int t = blockIdx.x * 256 + threadIdx.x;
  if (t >= len) return;
  if (t < 2) {
    long long s = 0;
    for (int b = 0; b < nb; ++b) s += __double_as_longlong(partial[(long)b * len + t]);
    record[t] = __longlong_as_double(s);
  } else {
    double s = 0.0;
    for (int b = 0; b < nb; ++b) s += partial[(long)b * len + t];
    record[t] = s;
  }
}

template <typename F>
__global__ __launch_bounds__(256) void univariate_kernel(const typename F::L* __restrict__ X, long n, long ldx, int d,
                                                         const double* __restrict__ loc,
                                                         const double* __restrict__ sc, double thr,
                                                         typename F::L* __restrict__ W) {
  const long e0 = (long)blockIdx.x * OUTLIER_UNI_SPAN;
  const long total = n * d;
  const long row0 = e0 / d;
  const int col0 = (int)(e0 - row0 * d);
#pragma unroll 4
  for (int it = 0; it < OUTLIER_UNI_SPAN / 256; ++it) {
    const int off = it * 256 + (int)threadIdx.x;
    if (e0 + off >= total) break;
    const int t = col0 + off;
    const int dr = t / d, col = t - dr * d;
    const double x = F::wide(X[(row0 + dr) * ldx + col]);
    const double s = sc[col];
    const double w = fabs(x - loc[col]) / (s < 1e-300 ? 1e-300 : s);
    W[e0 + off] = F::weight(w <= thr);
  }
}

template <typename F, int D>
int launch_pass_d(const void* X, long n, long ldx, int d, const double* cs, const double* P, int identity, double t2,
                  int strict, unsigned char* mask, double* dist2, int stats, double* partial, int flags,
                  hipStream_t s) {
  const long nchunks = (n + OUTLIER_CHUNK - 1) / OUTLIER_CHUNK;
  const dim3 g((unsigned)(nchunks < OUTLIER_GRID ? nchunks : OUTLIER_GRID)), b(OUTLIER_THREADS);
  if (flags & 1)
    pass_kernel<F, D, 1><<<g, b, 0, s>>>((const typename F::L*)X, n, ldx, d, cs, P, identity, t2, strict, mask, dist2,
                                         stats, partial);
  else
    pass_kernel<F, D, 0><<<g, b, 0, s>>>((const typename F::L*)X, n, ldx, d, cs, P, identity, t2, strict, mask, dist2,
                                         stats, partial);
  return harp_launch_status();
}

template <typename F>
int launch_pass(const void* X, long n, long ldx, int d, const double* cs, const double* P, int identity, double t2,
                int strict, unsigned char* mask, double* dist2, int stats, double* partial, int flags, hipStream_t s) {
  if (d <= 8) return launch_pass_d<F, 8>(X, n, ldx, d, cs, P, identity, t2, strict, mask, dist2, stats, partial, flags, s);
  if (d <= 16)
    return launch_pass_d<F, 16>(X, n, ldx, d, cs, P, identity, t2, strict, mask, dist2, stats, partial, flags, s);
  if (d <= 32)
    return launch_pass_d<F, 32>(X, n, ldx, d, cs, P, identity, t2, strict, mask, dist2, stats, partial, flags, s);
  return launch_pass_d<F, 64>(X, n, ldx, d, cs, P, identity, t2, strict, mask, dist2, stats, partial, flags, s);
}

template <typename F>
int launch_univariate(const void* X, long n, long ldx, int d, const double* loc, const double* sc, double thr, void* W,
                      hipStream_t s) {
  const long blocks = (n * d + OUTLIER_UNI_SPAN - 1) / OUTLIER_UNI_SPAN;
  if (blocks > 0x7fffffffL) return HARP_EUNSUPPORTED;
  univariate_kernel<F><<<dim3((unsigned)blocks), dim3(256), 0, s>>>((const typename F::L*)X, n, ldx, d, loc, sc, thr,
                                                                    (typename F::L*)W);
  return harp_launch_status();
}

}  // namespace

// The constants the Python side mirrors (ops/outlier.py checks them on first use): 0 rows of a
// chunk, 1 workgroups of the grid, 2 the widest row, 3 doubles of padding after the packed P.
// -1 for any other index.
HARP_EXPORT int harp_outlier_param(int which) {
  switch (which) {
    case 0: return OUTLIER_CHUNK;
    case 1: return OUTLIER_GRID;
    case 2: return OUTLIER_MAX_D;
    case 3: return kLoad;
    default: return -1;
  }
}

// One pass over X [n, d] (dtype 0 bf16 / 1 fp32 / 2 fp64, row stride ldx >= d elements, n > 0).
// cs: fp64 [2 * 64], the centre c in [0, 64) and the shift s in [64, 128), zero past d. P: fp64,
// the packed lower triangle of L^-1 at [0, d (d + 1) / 2), zeros up to 64 * 65 / 2 + 16 doubles
// (read only when identity == 0). member = dist2 < t2 (strict != 0) or <= t2. mask [n] uint8 or
// null: read and rewritten by each row's owner; dist2 [n] fp64 or null. stats == 0 skips the
// sums and the Gram matrix (their partials are zero). partial: fp64 [min(grid, chunks), 2 + d +
// d (d + 1) / 2], every element written. flags bit 0: the vector-FMA statistics form.
HARP_EXPORT int harp_outlier_pass(const void* X, int dtype, long n, long ldx, int d, const double* cs, const double* P,
                                  int identity, double t2, int strict, unsigned char* mask, double* dist2, int stats,
                                  double* partial, int flags, hipStream_t s) {
  if (n < 1 || d < 1 || ldx < d || !X || !cs || !partial || (!identity && !P)) return HARP_EBADARG;
  // 64 rows of the stride have to fit a 32-bit element offset
  if (d > OUTLIER_MAX_D || dtype < 0 || dtype > 2 || ldx >= (1L << 24)) return HARP_EUNSUPPORTED;
  if (dtype == 0)
    return launch_pass<InBf16>(X, n, ldx, d, cs, P, identity, t2, strict, mask, dist2, stats, partial, flags, s);
  if (dtype == 1)
    return launch_pass<InFp32>(X, n, ldx, d, cs, P, identity, t2, strict, mask, dist2, stats, partial, flags, s);
  return launch_pass<InFp64>(X, n, ldx, d, cs, P, identity, t2, strict, mask, dist2, stats, partial, flags, s);
}

// record [2 + d + d (d + 1) / 2] = the nb partial rows added in row order
HARP_EXPORT int harp_outlier_reduce(const double* partial, int nb, int d, double* record, hipStream_t s) {
  if (!partial || !record || nb < 1 || d < 1 || d > OUTLIER_MAX_D) return HARP_EBADARG;
  const int len = 2 + d + d * (d + 1) / 2;
  reduce_kernel<<<dim3((unsigned)((len + 255) / 256)), dim3(256), 0, s>>>(partial, nb, len, record);
  return harp_launch_status();
}

// W [n, d] (contiguous, X's dtype) = |x - loc_j| / max(sc_j, 1e-300) <= thr; loc, sc fp64 [d]
HARP_EXPORT int harp_outlier_univariate(const void* X, int dtype, long n, long ldx, int d, const double* loc,
                                        const double* sc, double thr, void* W, hipStream_t s) {
  if (n < 0 || d < 1 || ldx < d || !loc || !sc || (n > 0 && (!X || !W))) return HARP_EBADARG;
  if (dtype < 0 || dtype > 2) return HARP_EUNSUPPORTED;
  if (n == 0) return HARP_OK;
  if (dtype == 0) return launch_univariate<InBf16>(X, n, ldx, d, loc, sc, thr, W, s);
  if (dtype == 1) return launch_univariate<InFp32>(X, n, ldx, d, loc, sc, thr, W, s);
  return launch_univariate<InFp64>(X, n, ldx, d, loc, sc, thr, W, s);
}
