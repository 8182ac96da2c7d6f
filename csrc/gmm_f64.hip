// EM for Gaussian mixtures in fp64 for gfx950 (MI355X / CDNA4): the E-step and the sufficient
// statistics on the fp64 matrix cores, without a responsibility matrix. No buffer proportional
// to n x K exists; the only per-row buffers are lse [n] (fp64) and, for prediction, the labels.
// The rows X [n, d] (bf16 / fp32 / fp64, unit column stride, any row stride) are read in place
// and widened in registers; no fp64 copy of X is built. Every sum has one fixed order and every
// store is plain: results are bitwise repeatable.
//
// Reference: ml/daal daal_em/BatchDense (DAAL em_gmm, Double throughout). The math is that of
// csrc/gmm.hip: with Sigma_k = L_k L_k^T and P_k = L_k^-1 (lower triangular),
//   c_k = P_k mu_k,  b_k = log w_k - 0.5 (log|Sigma_k| + d log 2 pi),
//   log p(x, k) = b_k - 0.5 |P_k x - c_k|^2.
// The K Cholesky factorisations stay in torch; harp_amd/ops/gmm_f64.py drives the kernels.
//
// Why two kernels evaluate the E-step. The statistics of all components are K (d + 1)(d + 2) / 2
// doubles, far more than a workgroup can keep over its rows, and flushing them per chunk means
// atomics. So the accumulators are owned BY COMPONENT (a wave of stats_kernel keeps one
// component's whole upper Gram in registers over all of its rows) and the price is that log p
// is computed twice: once by lse_kernel for the row's log-sum-exp, once by stats_kernel, which
// turns it into r = exp(log p - lse) and uses it at once. Both call logp_tile on the same
// operand and the same staged tile, so the two values agree bit for bit and the r of a row sum
// to 1 to rounding.
//
// The width is padded to WP = 16 NT (NT = 1 .. 4); NB = NT (NT + 1) / 2 is the number of
// triangular 16 x 16 blocks. A chunk is 64 rows, staged into LDS as fp64 with a row stride of
// WP + 1 doubles (the E-step reads a column of 16 rows per lane group: the odd stride spreads it
// over the banks), zero in padded columns and in rows past n. Two buffers, one barrier per
// chunk; the global loads of chunk i + 1 are issued before the MFMAs of chunk i and land in LDS
// after them (the staging of xprod.hip: thread t owns column t % WP, so a wave-instruction reads
// runs of WP consecutive elements in the input dtype).
//
// prepare_kernel: the operand of a component, OP = NB * 256 + WP + 16 doubles, in the lane
// order logp_tile reads: for coordinate block j, feature block f <= j and k-step s the 64
// values B[(j (j + 1) / 2 + f) * 4 + s][lane] = P[16 j + (lane & 15)][16 f + 4 s + (lane >> 4)]
// (zero above the diagonal and in padding), then -c [WP] (zero in padding, so a padded
// coordinate is exactly 0), then b.
//
// logp_tile<NT> (v_mfma_f64_16x16x4_f64): z = X_tile P^T for one 16-row tile and one component.
// Operand A is the tile (lane l: row l & 15, feature 16 f + 4 s + (l >> 4)), operand B the
// prepared P. Register r of lane l of accumulator j holds z[row (l >> 4) + 4 r][coordinate 16 j
// + (l & 15)]; the accumulators start at -c. Coordinate block j multiplies the feature blocks
// f <= j only: 4 NB MFMAs, half the square. The squares are summed over j in the lane and over
// the 16 coordinate lanes by a DPP butterfly, which leaves the same bits in all 16 lanes.
// WHERE THE OPERAND LIVES. At d = 64 a component's operand is 20 KB; eight of them do not fit
// beside two 33 KB chunk buffers. The operand is therefore held in REGISTERS (4 NB doubles per
// lane, 80 VGPRs at NT = 4), loaded with lane-ordered coalesced reads that hit in L2: a wave
// loads it once per (chunk, component) in lse_kernel and once for its whole life in
// stats_kernel. At NT = 4 stats_kernel holds it beside 80 registers of Gram accumulators, so
// that form runs 4 waves (= components) per workgroup with up to 512 registers each; all other
// forms run 8 waves.
//
// lse_kernel<NT, ARG>: at most 512 workgroups of 8 waves, chunks dealt statically (b, b + G, ..).
// The components are dealt to the waves (k = wave, wave + 8, ..). For its components a wave
// keeps an online (max, sum-exp) pair per row of the chunk (lane group g of tile t computes rows
// 16 t + g + 4 r), with ARG also the best (log p, k), strict compare in ascending k, so a tie
// goes to the lowest component and a NaN never wins. The pairs live in the wave's slice of an
// LDS exchange buffer (in registers, 64 rows of state beside the operand spilled at NT >= 2).
// After the chunk's barrier thread `row` combines the eight waves' pairs in wave order into
// lse[row] (the exchange buffer is doubled, so there is no second barrier); each of these 64 threads adds its rows' lse, and the workgroup's sum (one fixed DPP
// order) is its log-likelihood partial.
//
// stats_kernel<NT>: grid (row splits, component groups), split s takes the chunks s, s + splits,
// .. A wave owns one component: per 16-row tile it recomputes log p, forms r (+inf is staged
// as the lse of a row past n, so its r is exactly 0) and accumulates sum r x x^T as
// (r x)^T x on the MFMA: k-step s of a tile takes rows 4 s + (l >> 4), exactly the rows whose r
// the lane already holds in register s, so r never moves between lanes. Operand A is r x, B is
// x; only the NB upper blocks are kept. sum r x is the running sum of the A values in the lane,
// sum r the running sum of r. One record per (split, component), plain stores: the accumulator
// fragments [NB][4][64], then sum r x [WP], then sum r.
//
// reduce_kernel: one thread per cell adds the records in split order; an off-diagonal block is
// mirrored, a diagonal block contributes its upper triangle and its mirror (its (i, j) and
// (j, i) round r x_i x_j differently). Thread 0 adds the log-likelihood partials in workgroup
// order.
//
// Compiler report (hipcc -O3 --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage): VGPRs +
// AGPRs per lane / LDS bytes; NO instantiation uses scratch (ScratchSize 0, no VGPR spill).
//   NT (d)        lse           lse + argmax     stats
//   1 (<= 16)   106 / 50176    111 / 50176      116 / 18432   (8 waves)
//   2 (<= 32)   139 / 66560    146 / 66560      158 / 34816   (8 waves)
//   3 (<= 48)   190 / 82944    208 / 82944      240 / 51200   (8 waves)
//   4 (<= 64)   238 / 99328    247 / 99328      238 + 144 / 67584   (4 waves)
// prepare_kernel and reduce_kernel use fewer than 32 VGPRs and no LDS.
#include "common.h"

#define GF_MAX_D 64
#define GF_MAX_K 1024
#define GF_CH 64           // rows of a chunk
#define GF_LSE_GRID 512    // workgroups of lse_kernel, at most
#define GF_LSE_WAVES 8
#define GF_MAX_SPLITS 1024
#define GF_STATS_WGS 512   // workgroups harp_gmm_f64_splits aims at

namespace {

typedef double doublex4 __attribute__((ext_vector_type(4)));

// ---- elements: raw bits in, fp64 out (as in xprod.hip) -----------------------------------------
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

// fp64 sum over the 16 lanes of a DPP row: a butterfly, so all 16 lanes end with the same bits
__device__ __forceinline__ double row_sum_d(double v) {
  v += dpp_mov_d<0x128>(v);  // row_ror:8
  v += dpp_mov_d<0x124>(v);  // row_ror:4
  v += dpp_mov_d<0x4E>(v);   // quad_perm [2,3,0,1]
  v += dpp_mov_d<0xB1>(v);   // quad_perm [1,0,3,2]
  return v;
}

__host__ __device__ constexpr int gf_tiles(int d) { return (d + 15) / 16; }
__host__ __device__ constexpr int gf_blocks(int nt) { return nt * (nt + 1) / 2; }
__host__ __device__ constexpr int gf_record(int nt) { return gf_blocks(nt) * 256 + 16 * nt + 16; }
__host__ __device__ constexpr int gf_stats_waves(int nt) { return nt == 4 ? 4 : 8; }
// row-major upper triangle of nt x nt: block g -> (t1, t2), t1 <= t2
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
  static constexpr int NB = gf_blocks(NT);
  static constexpr int LD = WP + 1;            // doubles between the rows of a staged chunk
  static constexpr int TILE = GF_CH * LD;      // doubles of one chunk buffer
  static constexpr int OP = gf_record(NT);     // doubles of a component's operand
  static constexpr int REC = gf_record(NT);    // doubles of a (split, component) record
  static constexpr int SW = gf_stats_waves(NT);
  static constexpr int COMB = GF_LSE_WAVES * GF_CH;  // entries of one exchange array of lse_kernel
  static constexpr int LSE_LDS = (2 * TILE + 2 * 4 * COMB) * 8;
  static constexpr int STATS_LDS = (2 * TILE + 2 * GF_CH) * 8;
  static_assert(LSE_LDS <= 160 * 1024 && STATS_LDS <= 160 * 1024, "chunks fit the LDS");
};

// ---- staging of a chunk: T threads, thread t owns column t % WP -------------------------------
template <int NT, int T>
struct Stage {
  static constexpr int WP = 16 * NT, LD = WP + 1, TR = T / WP, RPT = (GF_CH + TR - 1) / TR;
  uint64_t raw[RPT];
  __device__ __forceinline__ void fetch(const char* X, int dt, long ldx, int d, long n, long chunk, int tid) {
    const int tc = tid % WP, tr = tid / WP;
    const int eb = elem_bytes(dt);
    long off[RPT];
#pragma unroll
    for (int i = 0; i < RPT; ++i) {
      const int row = tr + i * TR;
      const bool ok = tr < TR && tc < d && row < GF_CH && chunk * GF_CH + row < n;
      off[i] = ok ? ((chunk * GF_CH + row) * ldx + tc) * eb : 0;  // out of range: element 0, dropped
    }
    load_raw(raw, X, off, dt);
  }
  __device__ __forceinline__ void stash(double* tile, int dt, int d, long n, long chunk, int tid) const {
    const int tc = tid % WP, tr = tid / WP;
#pragma unroll
    for (int i = 0; i < RPT; ++i) {
      const int row = tr + i * TR;
      const bool ok = tc < d && chunk * GF_CH + row < n;
      if (tr < TR && row < GF_CH) tile[row * LD + tc] = ok ? wide(raw[i], dt) : 0.0;
    }
  }
};

// ---- the operand -----------------------------------------------------------------------------
__global__ __launch_bounds__(256) void prepare_kernel(const double* __restrict__ P, const double* __restrict__ c,
                                                      const double* __restrict__ b, int d, int nt,
                                                      double* __restrict__ op, long total) {
  const int nb = gf_blocks(nt), wp = 16 * nt, len = gf_record(nt);
  const long e = (long)blockIdx.x * 256 + threadIdx.x;
  if (e >= total) return;
  const long k = e / len;
  const int o = (int)(e - k * len);
  double v = 0.0;
  if (o < nb * 256) {
    const int blk = o >> 8, s = (o >> 6) & 3, l = o & 63;
    int j = 0;
    while ((j + 1) * (j + 2) / 2 <= blk) ++j;
    const int f = blk - j * (j + 1) / 2;
    const int coord = 16 * j + (l & 15), feat = 16 * f + 4 * s + (l >> 4);
    if (coord < d && feat <= coord) v = P[(k * d + coord) * d + feat];
  } else if (o < nb * 256 + wp) {
    const int col = o - nb * 256;
    if (col < d) v = -c[k * d + col];
  } else if (o == nb * 256 + wp) {
    v = b[k];
  }
  op[e] = v;
}

template <int NT>
__device__ __forceinline__ void load_operand(const double* __restrict__ op, int lane, double (&P)[4 * gf_blocks(NT)],
                                             double (&nc)[NT], double& b) {
  constexpr int NB = gf_blocks(NT);
#pragma unroll
  for (int i = 0; i < 4 * NB; ++i) P[i] = op[i * 64 + lane];
#pragma unroll
  for (int j = 0; j < NT; ++j) nc[j] = op[NB * 256 + 16 * j + (lane & 15)];
  b = op[NB * 256 + 16 * NT];
}

// log p of the rows (lane >> 4) + 4 r of one staged tile for one component, the same bits in
// the 16 lanes of a row group. xt = the tile's row (lane & 15), plus (lane >> 4).
template <int NT>
__device__ __forceinline__ void logp_tile(const double* xt, const double (&P)[4 * gf_blocks(NT)],
                                          const double (&nc)[NT], double b, double (&lp)[4]) {
  doublex4 acc[NT];
#pragma unroll
  for (int j = 0; j < NT; ++j) acc[j] = doublex4{nc[j], nc[j], nc[j], nc[j]};
#pragma unroll
  for (int f = 0; f < NT; ++f) {
    double a[4];
#pragma unroll
    for (int s = 0; s < 4; ++s) a[s] = xt[16 * f + 4 * s];
#pragma unroll
    for (int j = f; j < NT; ++j)
#pragma unroll
      for (int s = 0; s < 4; ++s)
        acc[j] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[s], P[(j * (j + 1) / 2 + f) * 4 + s], acc[j], 0, 0, 0);
  }
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    double q = acc[0][r] * acc[0][r];
#pragma unroll
    for (int j = 1; j < NT; ++j) q = fma(acc[j][r], acc[j][r], q);
    lp[r] = fma(-0.5, row_sum_d(q), b);
  }
}

// ---- log-sum-exp of every row ------------------------------------------------------------------
template <int NT, bool ARG>
__global__ __launch_bounds__(64 * GF_LSE_WAVES) void lse_kernel(const char* __restrict__ X, int dt, long ldx, int d,
                                                                long n, const double* __restrict__ op, int K,
                                                                double* __restrict__ lse, double* __restrict__ llpart,
                                                                int* __restrict__ label) {
  typedef Shape<NT> SH;
  constexpr int T = 64 * GF_LSE_WAVES, NTL = GF_CH / 16;
  extern __shared__ __attribute__((aligned(16))) double lds[];
  double* comb = lds + 2 * SH::TILE;  // per buffer: max, sum, best value, best index
  const int tid = threadIdx.x, lane = tid & 63;
  const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int p = lane & 15, g = lane >> 4;
  const long nchunks = (n + GF_CH - 1) / GF_CH;

  Stage<NT, T> st;
  long k = blockIdx.x;  // the grid never exceeds nchunks
  int buf = 0;
  st.fetch(X, dt, ldx, d, n, k, tid);
  st.stash(lds, dt, d, n, k, tid);
  __syncthreads();
  double llacc = 0.0;
  for (; k < nchunks; k += gridDim.x) {
    const long kn = k + gridDim.x;
    const bool more = kn < nchunks;
    if (more) st.fetch(X, dt, ldx, d, n, kn, tid);
    const double* tile = lds + buf * SH::TILE;

    // The wave's online (max, sum-exp[, best value, best index]) of the chunk's rows lives in its
    // slice of the exchange buffer: the 16 lanes of a row group hold the same bits, all of them
    // store, and each reads back what it stored itself.
    double* cm = comb + buf * 4 * SH::COMB;
    double* wm = cm + wv * GF_CH + g;
    int* wi = reinterpret_cast<int*>(cm + 3 * SH::COMB) + wv * GF_CH + g;
#pragma unroll
    for (int e = 0; e < GF_CH; e += 4) {
      wm[e] = -__builtin_inf();
      wm[SH::COMB + e] = 0.0;
      if constexpr (ARG) {
        wm[2 * SH::COMB + e] = -__builtin_inf();
        wi[e] = 0x7fffffff;
      }
    }
    for (int c = wv; c < K; c += GF_LSE_WAVES) {
      double P[4 * SH::NB], nc[NT], b;
      load_operand<NT>(op + (long)c * SH::OP, lane, P, nc, b);
#pragma unroll 1
      for (int t = 0; t < NTL; ++t) {
        double lp[4];
        logp_tile<NT>(tile + (16 * t + p) * SH::LD + g, P, nc, b, lp);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int e = 16 * t + 4 * r;  // row 16 t + g + 4 r
          // one exp per entry: the smaller of (old max, new value) is rescaled to the larger
          const double mo = wm[e], so = wm[SH::COMB + e];
          const double df = lp[r] - mo;
          const double ex = exp(-fabs(df));
          wm[SH::COMB + e] = df > 0.0 ? fma(so, ex, 1.0) : so + ex;
          wm[e] = fmax(mo, lp[r]);
          if constexpr (ARG) {
            if (lp[r] > wm[2 * SH::COMB + e]) {  // ascending c: a tie keeps the lower component, a NaN fails
              wm[2 * SH::COMB + e] = lp[r];
              wi[e] = c;
            }
          }
        }
      }
    }
    if (more) st.stash(lds + (buf ^ 1) * SH::TILE, dt, d, n, kn, tid);
    __syncthreads();
    // the waves' pairs of a row in wave order (a wave without components left (-inf, 0))
    if (tid < GF_CH) {
      const long row = k * GF_CH + tid;
      double M = cm[tid];
#pragma unroll
      for (int w = 1; w < GF_LSE_WAVES; ++w) M = fmax(M, cm[w * GF_CH + tid]);
      double S = 0.0;
#pragma unroll
      for (int w = 0; w < GF_LSE_WAVES; ++w) {
        const double sw = cm[SH::COMB + w * GF_CH + tid];
        S += sw == 0.0 ? 0.0 : sw * exp(cm[w * GF_CH + tid] - M);
      }
      const double v = M + log(S);
      if (row < n) {
        lse[row] = v;
        llacc += v;
        if constexpr (ARG) {
          double best = -__builtin_inf();
          int bk = 0x7fffffff;
#pragma unroll
          for (int w = 0; w < GF_LSE_WAVES; ++w)
            arg_take<true>(best, bk, cm[2 * SH::COMB + w * GF_CH + tid],
                           reinterpret_cast<const int*>(cm + 3 * SH::COMB)[w * GF_CH + tid]);
          label[row] = bk == 0x7fffffff ? 0 : bk;
        }
      }
    }
    buf ^= 1;
  }
  if (wv == 0) {
    const double v = wave_sum_d_dpp(llacc);
    if (lane == 0) llpart[blockIdx.x] = v;
  }
}

// ---- the statistics ----------------------------------------------------------------------------
template <int NT>
__global__ __launch_bounds__(64 * gf_stats_waves(NT)) void stats_kernel(const char* __restrict__ X, int dt, long ldx,
                                                                        int d, long n, const double* __restrict__ op,
                                                                        int K, const double* __restrict__ lse,
                                                                        double* __restrict__ rec) {
  typedef Shape<NT> SH;
  constexpr int T = 64 * SH::SW, NTL = GF_CH / 16, NB = SH::NB;
  extern __shared__ __attribute__((aligned(16))) double lds[];
  double* lrow = lds + 2 * SH::TILE;  // lse of the chunk's rows, +inf past n
  const int tid = threadIdx.x, lane = tid & 63;
  const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int p = lane & 15, g = lane >> 4;
  const long nchunks = (n + GF_CH - 1) / GF_CH;
  const int comp = blockIdx.y * SH::SW + wv;
  const bool active = comp < K;  // a wave past K runs component K - 1 and stores nothing

  double P[4 * NB], nc[NT], b;
  load_operand<NT>(op + (long)(active ? comp : K - 1) * SH::OP, lane, P, nc, b);
  doublex4 G[NB];
  double s1[NT], rs = 0.0;
#pragma unroll
  for (int i = 0; i < NB; ++i) G[i] = doublex4{0.0, 0.0, 0.0, 0.0};
#pragma unroll
  for (int t = 0; t < NT; ++t) s1[t] = 0.0;

  Stage<NT, T> st;
  double lnext = 0.0;
  auto fetch = [&](long c) {
    st.fetch(X, dt, ldx, d, n, c, tid);
    if (tid < GF_CH) {
      const long row = c * GF_CH + tid;
      lnext = lse[row < n ? row : 0];
    }
  };
  auto stash = [&](int bf, long c) {
    st.stash(lds + bf * SH::TILE, dt, d, n, c, tid);
    if (tid < GF_CH) lrow[bf * GF_CH + tid] = c * GF_CH + tid < n ? lnext : __builtin_inf();
  };

  long k = blockIdx.x;  // a split past the last chunk writes a record of zeros
  int buf = 0;
  if (k < nchunks) {
    fetch(k);
    stash(0, k);
  }
  __syncthreads();
  for (; k < nchunks; k += gridDim.x) {
    const long kn = k + gridDim.x;
    const bool more = kn < nchunks;
    if (more) fetch(kn);
    const double* tile = lds + buf * SH::TILE;
    const double* lr = lrow + buf * GF_CH;
#pragma unroll 1
    for (int t = 0; t < NTL; ++t) {
      double lp[4];
      logp_tile<NT>(tile + (16 * t + p) * SH::LD + g, P, nc, b, lp);
#pragma unroll
      for (int ks = 0; ks < 4; ++ks) {
        // k-step ks multiplies the rows 4 ks + g: the rows of lp[ks] (register ks of the E-step)
        const int row = 16 * t + 4 * ks + g;
        const double r = exp(lp[ks] - lr[row]);
        rs += r;
        const double* xr = tile + row * SH::LD + p;
        double xv[NT], av[NT];
#pragma unroll
        for (int u = 0; u < NT; ++u) {
          xv[u] = xr[16 * u];
          av[u] = r * xv[u];
          s1[u] += av[u];
        }
#pragma unroll
        for (int i = 0; i < NB; ++i)
          G[i] = __builtin_amdgcn_mfma_f64_16x16x4f64(av[unit_row(i, NT)], xv[unit_col(i, NT)], G[i], 0, 0, 0);
      }
    }
    if (more) stash(buf ^ 1, kn);
    __syncthreads();
    buf ^= 1;
  }

  if (active) {
    double* out = rec + ((long)blockIdx.x * K + comp) * SH::REC;
#pragma unroll
    for (int i = 0; i < NB; ++i)
#pragma unroll
      for (int q = 0; q < 4; ++q) out[(i * 4 + q) * 64 + lane] = G[i][q];
    // the four row groups of a column in one fixed order
#pragma unroll
    for (int u = 0; u < NT; ++u) {
      const double v = (__shfl(s1[u], p, 64) + __shfl(s1[u], p + 16, 64)) +
                       (__shfl(s1[u], p + 32, 64) + __shfl(s1[u], p + 48, 64));
      if (g == 0) out[NB * 256 + 16 * u + p] = v;
    }
    const double tot = (__shfl(rs, 0, 64) + __shfl(rs, 16, 64)) + (__shfl(rs, 32, 64) + __shfl(rs, 48, 64));
    if (lane < 16) out[NB * 256 + SH::WP + lane] = lane == 0 ? tot : 0.0;
  }
}

// N [K], S1 [K, d], S2 [K, d, d] = the records [splits, K, REC] in split order; ll[0] = the nll
// partials of lse_kernel in workgroup order (llpart may be null)
__global__ __launch_bounds__(256) void reduce_kernel(const double* __restrict__ rec, int splits, int K, int d, int nt,
                                                     const double* __restrict__ llpart, int nll,
                                                     double* __restrict__ N, double* __restrict__ S1,
                                                     double* __restrict__ S2, double* __restrict__ ll) {
  const int nb = gf_blocks(nt), wp = 16 * nt, len = gf_record(nt);
  const int e = blockIdx.x * 256 + threadIdx.x, k = blockIdx.y;
  if (e == 0 && k == 0 && llpart) {
    double a = 0.0;
    for (int i = 0; i < nll; ++i) a += llpart[i];
    ll[0] = a;
  }
  if (e > nb * 256 + wp) return;
  double a = 0.0;
  for (int sp = 0; sp < splits; ++sp) a += rec[((long)sp * K + k) * len + e];
  if (e < nb * 256) {
    const int gb = e >> 8, q = (e >> 6) & 3, l = e & 63;
    const int t1 = unit_row(gb, nt), t2 = unit_col(gb, nt);
    const int i = 16 * t1 + (l >> 4) + 4 * q, j = 16 * t2 + (l & 15);
    if (i < d && j < d && (t1 != t2 || i <= j)) {
      S2[((long)k * d + i) * d + j] = a;
      if (i != j) S2[((long)k * d + j) * d + i] = a;
    }
  } else if (e < nb * 256 + wp) {
    const int col = e - nb * 256;
    if (col < d) S1[(long)k * d + col] = a;
  } else {
    N[k] = a;
  }
}

// ---- launchers -------------------------------------------------------------------------------
inline long chunk_count(long n) { return (n + GF_CH - 1) / GF_CH; }
inline int lse_grid(long n) { return (int)(chunk_count(n) < GF_LSE_GRID ? chunk_count(n) : GF_LSE_GRID); }

template <int NT, bool ARG>
int launch_lse(const void* X, int dt, long n, long ldx, int d, const double* op, int K, double* lse, double* llpart,
               int* label, hipStream_t s) {
  typedef Shape<NT> SH;
  if (SH::LSE_LDS > 65536 && hipFuncSetAttribute((const void*)lse_kernel<NT, ARG>,
                                                 hipFuncAttributeMaxDynamicSharedMemorySize, SH::LSE_LDS) != hipSuccess)
    return HARP_ELAUNCH;
  lse_kernel<NT, ARG><<<dim3((unsigned)lse_grid(n)), dim3(64 * GF_LSE_WAVES), SH::LSE_LDS, s>>>(
      (const char*)X, dt, ldx, d, n, op, K, lse, llpart, label);
  return harp_launch_status();
}

template <int NT>
int launch_stats(const void* X, int dt, long n, long ldx, int d, const double* op, int K, const double* lse, int splits,
                 double* rec, hipStream_t s) {
  typedef Shape<NT> SH;
  if (SH::STATS_LDS > 65536 && hipFuncSetAttribute((const void*)stats_kernel<NT>,
                                                   hipFuncAttributeMaxDynamicSharedMemorySize, SH::STATS_LDS) != hipSuccess)
    return HARP_ELAUNCH;
  const int groups = (K + SH::SW - 1) / SH::SW;
  stats_kernel<NT><<<dim3((unsigned)splits, (unsigned)groups), dim3(64 * SH::SW), SH::STATS_LDS, s>>>(
      (const char*)X, dt, ldx, d, n, op, K, lse, rec);
  return harp_launch_status();
}

inline bool bad_shape(long n, int d, int K) { return n > 0x7fffffffL || d > GF_MAX_D || K > GF_MAX_K; }

}  // namespace

#define GF_DISPATCH(d, CALL)        \
  switch (gf_tiles(d)) {            \
    case 1: return CALL(1);         \
    case 2: return CALL(2);         \
    case 3: return CALL(3);         \
    default: return CALL(4);        \
  }

HARP_EXPORT int harp_gmm_f64_max_d() { return GF_MAX_D; }
HARP_EXPORT int harp_gmm_f64_max_k() { return GF_MAX_K; }

// Figures of width d: 0 doubles of a component's operand, 1 doubles of a (split, component)
// record, 2 rows of a chunk, 3 components of a statistics workgroup; -1 for anything else.
HARP_EXPORT int harp_gmm_f64_param(int which, int d) {
  if (d < 1 || d > GF_MAX_D || which < 0 || which > 3) return -1;
  const int nt = gf_tiles(d);
  return which <= 1 ? gf_record(nt) : which == 2 ? GF_CH : gf_stats_waves(nt);
}

// op [K, operand doubles] (every element written) from P [K, d, d] (its lower triangle is
// read), c [K, d] and b [K], all fp64 and contiguous
HARP_EXPORT int harp_gmm_f64_prepare(const double* P, const double* c, const double* b, int K, int d, double* op,
                                     hipStream_t s) {
  if (!P || !c || !b || !op || K < 1 || d < 1) return HARP_EBADARG;
  if (bad_shape(1, d, K)) return HARP_EUNSUPPORTED;
  const int nt = gf_tiles(d);
  const long total = (long)K * gf_record(nt);
  prepare_kernel<<<dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s>>>(P, c, b, d, nt, op, total);
  return harp_launch_status();
}

// workgroups of harp_gmm_f64_lse for n rows = log-likelihood partials it writes (0: rejected)
HARP_EXPORT int harp_gmm_f64_lse_grid(long n) { return n < 1 || n > 0x7fffffffL ? 0 : lse_grid(n); }

// lse [n] = log sum_k exp log p(x, k) of the rows X [n, d] (dtype 0 bf16 / 1 fp32 / 2 fp64, unit
// column stride, row stride ldx >= d elements) under the K components behind op; llpart
// [harp_gmm_f64_lse_grid(n)] = each workgroup's sum of lse; label [n] (int32, may be null) = the
// arg-max component, ties to the lowest
HARP_EXPORT int harp_gmm_f64_lse(const void* X, int dt, long n, long ldx, int d, const double* op, int K, double* lse,
                                 double* llpart, int* label, hipStream_t s) {
  if (!X || !op || !lse || !llpart || n < 1 || d < 1 || K < 1 || ldx < d) return HARP_EBADARG;
  if (bad_shape(n, d, K) || dt < 0 || dt > 2) return HARP_EUNSUPPORTED;
#define GF_LSE(NT)                                                                            \
  (label ? launch_lse<NT, true>(X, dt, n, ldx, d, op, K, lse, llpart, label, s)               \
         : launch_lse<NT, false>(X, dt, n, ldx, d, op, K, lse, llpart, label, s))
  GF_DISPATCH(d, GF_LSE)
#undef GF_LSE
}

// the row splits harp_gmm_f64_stats's caller should use: enough workgroups to fill the chip
// when the component groups alone do not, never more than there are chunks
HARP_EXPORT int harp_gmm_f64_splits(long n, int d, int K) {
  if (n < 1 || d < 1 || K < 1 || bad_shape(n, d, K)) return 1;
  const int sw = gf_stats_waves(gf_tiles(d));
  const long groups = (K + sw - 1) / sw;
  long sp = (GF_STATS_WGS + groups - 1) / groups;
  if (sp > chunk_count(n)) sp = chunk_count(n);
  if (sp > GF_MAX_SPLITS) sp = GF_MAX_SPLITS;
  return sp < 1 ? 1 : (int)sp;
}

// rec [splits, K, record doubles] = per (split, component) the upper blocks of sum r x x^T, then
// sum r x, then sum r, with r = exp(log p(x, k) - lse[row]); X, op as for harp_gmm_f64_lse
HARP_EXPORT int harp_gmm_f64_stats(const void* X, int dt, long n, long ldx, int d, const double* op, int K,
                                   const double* lse, int splits, double* rec, hipStream_t s) {
  if (!X || !op || !lse || !rec || n < 1 || d < 1 || K < 1 || ldx < d || splits < 1) return HARP_EBADARG;
  if (bad_shape(n, d, K) || dt < 0 || dt > 2 || splits > GF_MAX_SPLITS) return HARP_EUNSUPPORTED;
#define GF_STATS(NT) launch_stats<NT>(X, dt, n, ldx, d, op, K, lse, splits, rec, s)
  GF_DISPATCH(d, GF_STATS)
#undef GF_STATS
}

// N [K], S1 [K, d], S2 [K, d, d] (both triangles) = the records added in split order; ll [1] =
// the nll partials of harp_gmm_f64_lse added in workgroup order
HARP_EXPORT int harp_gmm_f64_reduce(const double* rec, int splits, int K, int d, const double* llpart, int nll,
                                    double* N, double* S1, double* S2, double* ll, hipStream_t s) {
  if (!rec || !N || !S1 || !S2 || splits < 1 || K < 1 || d < 1 || (llpart && (!ll || nll < 1))) return HARP_EBADARG;
  if (bad_shape(1, d, K)) return HARP_EUNSUPPORTED;
  const int nt = gf_tiles(d);
  reduce_kernel<<<dim3((unsigned)((gf_record(nt) + 255) / 256), (unsigned)K), dim3(256), 0, s>>>(
      rec, splits, K, d, nt, llpart, nll, N, S1, S2, ll);
  return harp_launch_status();
}
