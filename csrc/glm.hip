// Sum-of-functions objectives and their solvers for gfx950 (MI355X / CDNA4): one fused value +
// gradient pass over a row block, and whole SGD / AdaGrad trajectories in one launch.
//
// Reference: ml/daal daal_optimization_solvers {MSEDenseBatch, SGDDenseBatch, SGDMiniDenseBatch,
// SGDMomentDenseBatch, AdaGradient, LBFGSDenseBatch and the Opt variants} (DAAL optimization_solver
// mse / logistic_loss / cross_entropy_loss, sgd, adagrad, lbfgs). harp_amd/ops/glm.py drives the
// kernels; the oracle of tests/test_optim_gpu.py is the torch Objective of models/optim.py in
// fp64 on the CPU.
//
// X [n, d] (bf16 / fp32 / fp64) is read in place through its row stride and widened in registers;
// the argument, the targets and every sum are fp64. With an index list the rows are gathered by
// index straight from X (repeats, any order, negative indices counted from the end; an index
// outside the block adds nothing). Nothing of size [n, .] is written.
//
// pass_kernel (MSE, logistic loss: one output per row). z = b0 + w . X_i, r = z - y or
// sigmoid(z) - y, value += loss(z, y), g += r X_i.
//  * A fixed grid of at most GLM_GRID workgroups of four waves; chunk k (GLM_CHUNK rows) belongs to
//    workgroup k mod grid, a wave owns 64 rows of it. No work counter and no atomics.
//  * A group of GW lanes owns a row, GW the power of two that covers the row's d / VEC lane slots
//    (1 .. 64); lane l of the group holds columns (a GW + l) VEC .. + VEC for a < NA, so its
//    coefficients and its gradient partials are NA VEC fp64 registers for the whole kernel. VEC = 4
//    (one 8 / 16 / 32-byte load per lane) when d, the row stride and the base allow it, else 1.
//    The 64 / GW groups of a wave read consecutive rows, so a wave-instruction still reads one
//    contiguous run of the block when the rows are dense; up to eight row sets are in flight.
//  * The row's dot product is an xor butterfly over the group (DPP inside a 16-lane row, two
//    shuffles above it): both partners of a step add the same two numbers, so every lane of the
//    group holds the same z and the same r. No LDS round trip, no transpose: the lanes that read a
//    row are the lanes that own its gradient columns.
//  * Epilogue: the groups of a wave meet by the same butterfly, the four waves through LDS in wave
//    order, and the workgroup stores one record [value, gradient (intercept first)] to its row of
//    partial with plain stores.
//
// ce_kernel (cross-entropy, K classes). One workgroup takes GLM_CE_ROWS rows at a time into an fp64
// LDS tile (zero-padded to 16 columns), with the coefficient matrix resident in LDS:
//  * Z = X_tile B^T + b0 on v_mfma_f64_16x16x4_f64 (A[i = lane & 15][k = lane >> 4], B[k = lane >> 4]
//    [j = lane & 15], one ds_read_b64 each), a 16 x 16 tile of Z per wave and step;
//  * eight lanes per row: max, sum of exponentials (butterfly, so all eight agree), the row's loss,
//    and R = softmax - onehot written over Z in LDS;
//  * G [K, d] += R^T X_tile on the same instruction, tile t of G owned by wave t mod 4 with its
//    accumulators in registers over all chunks of the workgroup; R 1 feeds the intercept column.
//
// reduce_kernel adds the partial records in workgroup order: a pass is bitwise repeatable.
//
// solver_kernel: one workgroup runs every iteration of sgd (plain, mini-batch with a conservative
// sequence and inner iterations, momentum) or adagrad on MSE / logistic loss. The argument and the
// solver state live in LDS; a wave owns a batch row at a time (lane l holds columns l + 64 a), the
// waves' register partials of g meet in LDS in wave order, then one thread per coordinate adds
// l2 and the proximal term and applies the update with the roundings of the torch expressions
// (no contraction). The stopping rules are evaluated on the device; the kernel writes x and the
// number of iterations performed.
//
// All stores are vector stores; no kernel waits on another workgroup.
#include "common.h"

// The update formulas have to round like the torch expressions they replace; the FMAs of the
// dot products and gradient sums are written as fma().
#pragma clang fp contract(off)

#define GLM_THREADS 256
#define GLM_CHUNK 256       // rows of a chunk of the one-output pass
#define GLM_GRID 512        // its workgroups (two per CU)
#define GLM_MAX_D 256       // widest row of the one-output pass and of the solver
#define GLM_CE_ROWS 32      // rows of a cross-entropy chunk
#define GLM_CE_GRID 512
#define GLM_CE_MAX_K 64
#define GLM_CE_MAX_D 128
#define GLM_SOLVER_MAX_BATCH 64
#define GLM_SOLVER_MAX_DIM (GLM_MAX_D + 1)

#define GLM_MSE 0
#define GLM_LOGISTIC 1
#define GLM_CE 2

namespace {

typedef double doublex4 __attribute__((ext_vector_type(4)));

struct InBf16 {
  typedef uint16_t L;
  static __device__ __forceinline__ double wide(L v) { return (double)__uint_as_float((uint32_t)v << 16); }
};
struct InFp32 {
  typedef float L;
  static __device__ __forceinline__ double wide(L v) { return (double)v; }
};
struct InFp64 {
  typedef double L;
  static __device__ __forceinline__ double wide(L v) { return v; }
};

// ---- per-row pieces shared by the pass and the solver -----------------------------------------
// residual and loss of one row from its linear response z (kind: GLM_MSE or GLM_LOGISTIC)
__device__ __forceinline__ double row_residual(int kind, double z, double y, double& loss) {
  if (kind == GLM_MSE) {
    const double r = z - y;
    loss = 0.5 * (r * r);
    return r;
  }
  // binary_cross_entropy_with_logits: max(z, 0) - z y + log1p(exp(-|z|))
  loss = (fmax(z, 0.0) - z * y) + log1p(exp(-fabs(z)));
  return 1.0 / (1.0 + exp(-z)) - y;
}

// the local row of an index (negative: from the end), or -1 when it is outside the block
__device__ __forceinline__ long list_row(const int* __restrict__ idx, long p, long n) {
  long row = idx ? (long)idx[p] : p;
  if (row < 0) row += n;
  return row >= 0 && row < n ? row : -1;
}

// sum over the GW lanes of a group (GW consecutive lanes, a power of two), the same bits in all
template <int GW>
__device__ __forceinline__ double group_sum(double v) {
  if constexpr (GW >= 2) v += dpp_mov_d<0xB1>(v);    // quad_perm [1,0,3,2]
  if constexpr (GW >= 4) v += dpp_mov_d<0x4E>(v);    // quad_perm [2,3,0,1]
  if constexpr (GW >= 8) v += dpp_mov_d<0x141>(v);   // row_half_mirror: the other quad of the eight
  if constexpr (GW >= 16) v += dpp_mov_d<0x140>(v);  // row_mirror: the other half of the row
  if constexpr (GW >= 32) v += __shfl_xor(v, 16, 64);
  if constexpr (GW >= 64) v += __shfl_xor(v, 32, 64);
  return v;
}
template <int GW>
__device__ __forceinline__ double group_max(double v) {
  if constexpr (GW >= 2) v = fmax(v, dpp_mov_d<0xB1>(v));
  if constexpr (GW >= 4) v = fmax(v, dpp_mov_d<0x4E>(v));
  if constexpr (GW >= 8) v = fmax(v, dpp_mov_d<0x141>(v));
  return v;
}
// sum over the 64 / GW groups of a wave, lane by lane of the group
template <int GW>
__device__ __forceinline__ double across_groups(double v) {
#pragma unroll
  for (int o = GW; o < 64; o <<= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// ---- the one-output pass ------------------------------------------------------------------------
template <typename L, int VEC>
struct VecOf {
  typedef L T __attribute__((ext_vector_type(VEC)));
};
template <typename L>
struct VecOf<L, 1> {
  typedef L T;
};

template <typename F, int GW, int NA, int VEC>
__global__ __launch_bounds__(GLM_THREADS) void pass_kernel(const typename F::L* __restrict__ X, long n, long ldx, int d,
                                                           const double* __restrict__ y,
                                                           const double* __restrict__ w, int icpt, int kind,
                                                           const int* __restrict__ idx, long m,
                                                           double* __restrict__ partial) {
  typedef typename F::L L;
  typedef typename VecOf<L, VEC>::T LV;
  constexpr int RPW = 64 / GW;         // rows of a wave-instruction
  constexpr int U = GW < 8 ? GW : 8;   // row sets in flight
  __shared__ double red[4][GLM_MAX_D + 2];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int gl = lane & (GW - 1), gi = lane / GW;
  const long nchunks = (m + GLM_CHUNK - 1) / GLM_CHUNK;

  bool live[NA];  // the lane's slot a holds columns of the row
  double wc[NA][VEC], g[NA][VEC];
#pragma unroll
  for (int a = 0; a < NA; ++a) {
    const int c0 = (a * GW + gl) * VEC;
    live[a] = c0 < d;  // d is a multiple of VEC when VEC > 1
#pragma unroll
    for (int v = 0; v < VEC; ++v) {
      wc[a][v] = live[a] ? w[icpt + c0 + v] : 0.0;
      g[a][v] = 0.0;
    }
  }
  const double b0 = icpt ? w[0] : 0.0;
  double val = 0.0, g0 = 0.0;

  for (long k = blockIdx.x; k < nchunks; k += gridDim.x) {
    const long p0 = k * GLM_CHUNK + wv * 64;
    for (int s0 = 0; s0 < GW; s0 += U) {
      LV xv[U][NA];
      double yv[U];
      bool ok[U];
      // loads are unconditional: a slot without a row or without columns reads the block's start
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const long p = p0 + (long)(s0 + u) * RPW + gi;
        const long row = p < m ? list_row(idx, p, n) : -1;
        ok[u] = row >= 0;
        const L* base = X + (ok[u] ? row * ldx : 0);
#pragma unroll
        for (int a = 0; a < NA; ++a)
          xv[u][a] = *reinterpret_cast<const LV*>(base + (live[a] ? (a * GW + gl) * VEC : 0));
        yv[u] = y[ok[u] ? row : 0];
      }
#pragma unroll
      for (int u = 0; u < U; ++u) {
        double x[NA][VEC], dot = 0.0;
#pragma unroll
        for (int a = 0; a < NA; ++a)
#pragma unroll
          for (int v = 0; v < VEC; ++v) {
            L e;
            if constexpr (VEC == 1)
              e = xv[u][a];
            else
              e = xv[u][a][v];
            x[a][v] = ok[u] && live[a] ? F::wide(e) : 0.0;
            dot = fma(x[a][v], wc[a][v], dot);
          }
        const double z = group_sum<GW>(dot) + b0;
        double loss;
        double r = row_residual(kind, z, yv[u], loss);
        r = ok[u] ? r : 0.0;
        if (gl == 0) {
          val += ok[u] ? loss : 0.0;
          g0 += r;
        }
#pragma unroll
        for (int a = 0; a < NA; ++a)
#pragma unroll
          for (int v = 0; v < VEC; ++v) g[a][v] = fma(r, x[a][v], g[a][v]);
      }
    }
  }

  // ---- the workgroup's record: groups by butterfly, waves through LDS in wave order -------------
  val = across_groups<GW>(val);
  g0 = across_groups<GW>(g0);
#pragma unroll
  for (int a = 0; a < NA; ++a)
#pragma unroll
    for (int v = 0; v < VEC; ++v) {
      g[a][v] = across_groups<GW>(g[a][v]);
      if (gi == 0 && live[a]) red[wv][1 + icpt + (a * GW + gl) * VEC + v] = g[a][v];
    }
  if (lane == 0) {
    red[wv][0] = val;
    if (icpt) red[wv][1] = g0;
  }
  __syncthreads();
  const int len = 1 + icpt + d;
  double* out = partial + (long)blockIdx.x * len;
  for (int t = tid; t < len; t += GLM_THREADS) out[t] = ((red[0][t] + red[1][t]) + red[2][t]) + red[3][t];
}

// ---- cross-entropy ----------------------------------------------------------------------------
__host__ __device__ inline int ce_pad(int v) { return (v + 15) & ~15; }
// doubles of LDS: B [KP][DP + 2], X tile [ROWS][DP + 2], Z tile [ROWS][KP + 2], b0 [KP], class ids
// (ROWS ints), the block sum's scratch
__host__ __device__ inline int ce_lds_doubles(int d, int K) {
  const int DP = ce_pad(d), KP = ce_pad(K);
  return KP * (DP + 2) + GLM_CE_ROWS * (DP + 2) + GLM_CE_ROWS * (KP + 2) + KP + GLM_CE_ROWS / 2 + 4;
}

template <typename F>
__global__ __launch_bounds__(GLM_THREADS) void ce_kernel(const typename F::L* __restrict__ X, long n, long ldx, int d,
                                                         int K, const double* __restrict__ y,
                                                         const double* __restrict__ w, int icpt,
                                                         const int* __restrict__ idx, long m,
                                                         double* __restrict__ partial) {
  extern __shared__ __attribute__((aligned(16))) double ce_lds[];
  const int DP = ce_pad(d), KP = ce_pad(K), XS = DP + 2, ZS = KP + 2;
  const int KT = KP / 16, DT = DP / 16;
  double* Bs = ce_lds;
  double* Xs = Bs + KP * XS;
  double* Zs = Xs + GLM_CE_ROWS * XS;
  double* b0s = Zs + GLM_CE_ROWS * ZS;
  int* ys = reinterpret_cast<int*>(b0s + KP);
  double* red = b0s + KP + GLM_CE_ROWS / 2;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int lo = lane & 15, hi = lane >> 4;
  const int wd = d + icpt;  // row length of the coefficient matrix
  const long nchunks = (m + GLM_CE_ROWS - 1) / GLM_CE_ROWS;

  // coefficients to LDS, zero in the padding; the X tile's padding columns are zeroed once
  for (int e = tid; e < KP * XS; e += GLM_THREADS) {
    const int c = e / XS, j = e - c * XS;
    Bs[e] = c < K && j < d ? w[c * wd + icpt + j] : 0.0;
  }
  for (int e = tid; e < GLM_CE_ROWS * XS; e += GLM_THREADS) Xs[e] = 0.0;
  for (int c = tid; c < KP; c += GLM_THREADS) b0s[c] = icpt && c < K ? w[c * wd] : 0.0;

  doublex4 acc[8];  // tile wv + 4 q of G: (class 16 ct + hi + 4 r, column 16 jt + lo) in acc[q][r]
#pragma unroll
  for (int q = 0; q < 8; ++q) acc[q] = doublex4{0.0, 0.0, 0.0, 0.0};
  double val = 0.0, g0 = 0.0;
  __syncthreads();

  for (long k = blockIdx.x; k < nchunks; k += gridDim.x) {
    const long p0 = k * GLM_CE_ROWS;
    // the chunk's rows to the fp64 tile; a slot without a row holds zeros and class -1
    for (int e = tid; e < GLM_CE_ROWS * d; e += GLM_THREADS) {
      const int i = e / d, j = e - i * d;
      const long row = p0 + i < m ? list_row(idx, p0 + i, n) : -1;
      Xs[i * XS + j] = row >= 0 ? F::wide(X[row * ldx + j]) : 0.0;
    }
    if (tid < GLM_CE_ROWS) {
      const long row = p0 + tid < m ? list_row(idx, p0 + tid, n) : -1;
      ys[tid] = row >= 0 ? (int)y[row] : -1;
    }
    __syncthreads();

    // Z tile (row tile rt, class tile ct) = X_tile B^T + b0
    for (int t = wv; t < 2 * KT; t += 4) {
      const int rt = t & 1, ct = t >> 1;
      const double* ap = Xs + (rt * 16 + lo) * XS + hi;
      const double* bp = Bs + (ct * 16 + lo) * XS + hi;
      doublex4 c = doublex4{0.0, 0.0, 0.0, 0.0};
      for (int kk = 0; kk < DP / 4; ++kk) c = __builtin_amdgcn_mfma_f64_16x16x4f64(ap[kk * 4], bp[kk * 4], c, 0, 0, 0);
      const double b0 = b0s[ct * 16 + lo];
#pragma unroll
      for (int r = 0; r < 4; ++r) Zs[(rt * 16 + hi + 4 * r) * ZS + ct * 16 + lo] = c[r] + b0;
    }
    __syncthreads();

    // eight lanes per row: lane s of the row holds classes s, s + 8, ..
    {
      const int i = tid >> 3, s = tid & 7;
      const int yi = ys[i];
      double* zr = Zs + i * ZS;
      const double zy = zr[yi < 0 ? 0 : yi < K ? yi : K - 1];
      double e[8], mx = -__builtin_inf();
#pragma unroll
      for (int q = 0; q < 8; ++q) {
        const int c = s + 8 * q;
        e[q] = c < K ? zr[c] : -__builtin_inf();
        mx = fmax(mx, e[q]);
      }
      mx = group_max<8>(mx);
      double se = 0.0;
#pragma unroll
      for (int q = 0; q < 8; ++q) {
        e[q] = s + 8 * q < K ? exp(e[q] - mx) : 0.0;
        se += e[q];
      }
      se = group_sum<8>(se);
      lds_sync_wave();  // every lane of the row has read its logits and z_y
#pragma unroll
      for (int q = 0; q < 8; ++q) {
        const int c = s + 8 * q;
        if (c < KP) zr[c] = yi >= 0 && c < K ? e[q] / se - (c == yi ? 1.0 : 0.0) : 0.0;
      }
      if (s == 0 && yi >= 0) val += (log(se) + mx) - zy;
    }
    __syncthreads();

    // R 1 for the intercept column, G += R^T X_tile
    if (tid < K) {
      double s = 0.0;
      for (int i = 0; i < GLM_CE_ROWS; ++i) s += Zs[i * ZS + tid];
      g0 += s;
    }
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      const int t = wv + 4 * q;
      if (t < KT * DT) {  // wave-uniform
        const int ct = t / DT, jt = t - ct * DT;
        const double* ap = Zs + hi * ZS + ct * 16 + lo;
        const double* bp = Xs + hi * XS + jt * 16 + lo;
#pragma unroll
        for (int ii = 0; ii < GLM_CE_ROWS / 4; ++ii)
          acc[q] = __builtin_amdgcn_mfma_f64_16x16x4f64(ap[ii * 4 * ZS], bp[ii * 4 * XS], acc[q], 0, 0, 0);
      }
    }
    __syncthreads();
  }

  // ---- the workgroup's record: every tile of G has one owner, plain stores ------------------------
  const int len = 1 + K * wd;
  double* out = partial + (long)blockIdx.x * len;
  val = block_sum_d<GLM_THREADS>(val, red);
  if (tid == 0) out[0] = val;
  if (icpt && tid < K) out[1 + tid * wd] = g0;
#pragma unroll
  for (int q = 0; q < 8; ++q) {
    const int t = wv + 4 * q;
    if (t < KT * DT) {
      const int ct = t / DT, jt = t - ct * DT;
      const int j = jt * 16 + lo;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int c = ct * 16 + hi + 4 * r;
        if (c < K && j < d) out[1 + c * wd + icpt + j] = acc[q][r];
      }
    }
  }
}

// record[t] = sum over the nb partial rows, in row order
__global__ __launch_bounds__(256) void reduce_kernel(const double* __restrict__ partial, int nb, int len,
                                                     double* __restrict__ record) {
  const int t = blockIdx.x * 256 + threadIdx.x;
  if (t >= len) return;
  double s = 0.0;
  for (int b = 0; b < nb; ++b) s += partial[(long)b * len + t];
  record[t] = s;
}

// ---- whole trajectories ---------------------------------------------------------------------------
struct SolverArgs {
  long n, ldx;
  int d, icpt, kind, method;  // method 0: sgd family, 1: adagrad
  int iterations, batch, inner;
  double momentum, l2, threshold, eps;
};

template <typename F>
__global__ __launch_bounds__(GLM_THREADS) void solver_kernel(const typename F::L* __restrict__ X,
                                                             const double* __restrict__ y,
                                                             const int* __restrict__ table,
                                                             const double* __restrict__ lr,
                                                             const double* __restrict__ gamma, SolverArgs p,
                                                             double* __restrict__ x, int* __restrict__ niter) {
  typedef typename F::L L;
  constexpr int NA = GLM_MAX_D / 64;
  __shared__ double xs[GLM_SOLVER_MAX_DIM], state[GLM_SOLVER_MAX_DIM], anchor[GLM_SOLVER_MAX_DIM];
  __shared__ double gs[GLM_SOLVER_MAX_DIM], gp[4][GLM_SOLVER_MAX_DIM], red[4];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int d = p.d, icpt = p.icpt, dim = d + icpt;
  for (int t = tid; t < dim; t += GLM_THREADS) {
    xs[t] = x[t];
    state[t] = 0.0;
  }
  __syncthreads();

  int done = p.iterations;
  for (int k = 0; k < p.iterations; ++k) {
    const double lrk = lr[k], gam = gamma ? gamma[k] : 0.0;
    for (int t = tid; t < dim; t += GLM_THREADS) anchor[t] = xs[t];  // x_k: the proximal anchor and x_prev
    __syncthreads();
    bool stop = false;
    for (int it = 0; it < p.inner; ++it) {
      // the batch's gradient sum: a wave per row, its partials in registers
      double wc[NA], g[NA], g0 = 0.0;
#pragma unroll
      for (int a = 0; a < NA; ++a) {
        wc[a] = lane + 64 * a < d ? xs[icpt + lane + 64 * a] : 0.0;
        g[a] = 0.0;
      }
      const double b0 = icpt ? xs[0] : 0.0;
      for (int j = wv; j < p.batch; j += 4) {
        const long row = list_row(table, (long)k * p.batch + j, p.n);
        const L* base = X + (row >= 0 ? row * p.ldx : 0);
        double xr[NA], dot = 0.0;
#pragma unroll
        for (int a = 0; a < NA; ++a) {
          const int c = lane + 64 * a;
          xr[a] = row >= 0 && c < d ? F::wide(base[c < d ? c : 0]) : 0.0;
          dot = fma(xr[a], wc[a], dot);
        }
        const double z = wave_sum_d_dpp(dot) + b0;
        double loss;
        double r = row_residual(p.kind, z, y[row >= 0 ? row : 0], loss);
        r = row >= 0 ? r : 0.0;
        g0 += r;
#pragma unroll
        for (int a = 0; a < NA; ++a) g[a] = fma(r, xr[a], g[a]);
      }
#pragma unroll
      for (int a = 0; a < NA; ++a)
        if (lane + 64 * a < d) gp[wv][icpt + lane + 64 * a] = g[a];
      if (icpt && lane == 0) gp[wv][0] = g0;
      __syncthreads();

      // one thread per coordinate: normalise, l2, the proximal term, the update
      double sq = 0.0;
      for (int t = tid; t < dim; t += GLM_THREADS) {
        double gt = (((gp[0][t] + gp[1][t]) + gp[2][t]) + gp[3][t]) / (double)p.batch;
        if (p.l2 != 0.0 && t >= icpt) gt = gt + (2 * p.l2) * xs[t];
        if (p.method == 0) {
          if (gam != 0.0) gt = gt + gam * (xs[t] - anchor[t]);
          if (p.momentum != 0.0) {
            const double v = p.momentum * state[t] + lrk * gt;
            state[t] = v;
            xs[t] = xs[t] - v;
          } else {
            xs[t] = xs[t] - lrk * gt;
          }
        } else {
          gs[t] = gt;
          sq += gt * gt;
        }
      }
      if (p.method == 1) {  // adagrad: ||g|| < threshold stops before the update
        if (p.threshold != 0.0) stop = sqrt(block_sum_d<GLM_THREADS>(sq, red)) < p.threshold;
        if (stop) break;
        for (int t = tid; t < dim; t += GLM_THREADS) {
          const double gt = gs[t];
          const double G = state[t] + gt * gt;
          state[t] = G;
          xs[t] = xs[t] - lrk * gt / sqrt(G + p.eps);
        }
      }
      __syncthreads();
    }
    if (p.method == 0 && p.threshold != 0.0) {  // sgd: the relative step
      double dn = 0.0, pn = 0.0;
      for (int t = tid; t < dim; t += GLM_THREADS) {
        const double s = xs[t] - anchor[t];
        dn += s * s;
        pn += anchor[t] * anchor[t];
      }
      dn = block_sum_d<GLM_THREADS>(dn, red);
      pn = block_sum_d<GLM_THREADS>(pn, red);
      stop = sqrt(dn) / fmax(1.0, sqrt(pn)) < p.threshold;
    }
    if (stop) {  // the same bits in every thread: the whole workgroup leaves together
      done = k + 1;
      break;
    }
  }
  __syncthreads();
  for (int t = tid; t < dim; t += GLM_THREADS) x[t] = xs[t];
  if (tid == 0) niter[0] = done;
}

// ---- launchers ------------------------------------------------------------------------------------
template <typename F, int GW, int NA, int VEC>
int launch_pass_g(const void* X, long n, long ldx, int d, const double* y, const double* w, int icpt, int kind,
                  const int* idx, long m, double* partial, hipStream_t s) {
  const long nchunks = (m + GLM_CHUNK - 1) / GLM_CHUNK;
  pass_kernel<F, GW, NA, VEC><<<dim3((unsigned)(nchunks < GLM_GRID ? nchunks : GLM_GRID)), dim3(GLM_THREADS), 0, s>>>(
      (const typename F::L*)X, n, ldx, d, y, w, icpt, kind, idx, m, partial);
  return harp_launch_status();
}

#define GLM_PASS_ARGS X, n, ldx, d, y, w, icpt, kind, idx, m, partial, s
template <typename F>
int launch_pass(const void* X, long n, long ldx, int d, const double* y, const double* w, int icpt, int kind,
                const int* idx, long m, double* partial, hipStream_t s) {
  const size_t vb = 4 * sizeof(typename F::L);
  if (d % 4 == 0 && ldx % 4 == 0 && (uintptr_t)X % vb == 0) {  // four columns per lane
    const int slots = d / 4;
    if (slots <= 1) return launch_pass_g<F, 1, 1, 4>(GLM_PASS_ARGS);
    if (slots <= 2) return launch_pass_g<F, 2, 1, 4>(GLM_PASS_ARGS);
    if (slots <= 4) return launch_pass_g<F, 4, 1, 4>(GLM_PASS_ARGS);
    if (slots <= 8) return launch_pass_g<F, 8, 1, 4>(GLM_PASS_ARGS);
    if (slots <= 16) return launch_pass_g<F, 16, 1, 4>(GLM_PASS_ARGS);
    if (slots <= 32) return launch_pass_g<F, 32, 1, 4>(GLM_PASS_ARGS);
    return launch_pass_g<F, 64, 1, 4>(GLM_PASS_ARGS);
  }
  if (d <= 1) return launch_pass_g<F, 1, 1, 1>(GLM_PASS_ARGS);
  if (d <= 2) return launch_pass_g<F, 2, 1, 1>(GLM_PASS_ARGS);
  if (d <= 4) return launch_pass_g<F, 4, 1, 1>(GLM_PASS_ARGS);
  if (d <= 8) return launch_pass_g<F, 8, 1, 1>(GLM_PASS_ARGS);
  if (d <= 16) return launch_pass_g<F, 16, 1, 1>(GLM_PASS_ARGS);
  if (d <= 32) return launch_pass_g<F, 32, 1, 1>(GLM_PASS_ARGS);
  if (d <= 64) return launch_pass_g<F, 64, 1, 1>(GLM_PASS_ARGS);
  if (d <= 128) return launch_pass_g<F, 64, 2, 1>(GLM_PASS_ARGS);
  return launch_pass_g<F, 64, 4, 1>(GLM_PASS_ARGS);
}

template <typename F>
int launch_ce(const void* X, long n, long ldx, int d, int K, const double* y, const double* w, int icpt,
              const int* idx, long m, double* partial, hipStream_t s) {
  const size_t lds = (size_t)ce_lds_doubles(d, K) * sizeof(double);
  if (lds > 65536 &&
      hipFuncSetAttribute((const void*)ce_kernel<F>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess)
    return HARP_ELAUNCH;
  const long nchunks = (m + GLM_CE_ROWS - 1) / GLM_CE_ROWS;
  ce_kernel<F><<<dim3((unsigned)(nchunks < GLM_CE_GRID ? nchunks : GLM_CE_GRID)), dim3(GLM_THREADS), lds, s>>>(
      (const typename F::L*)X, n, ldx, d, K, y, w, icpt, idx, m, partial);
  return harp_launch_status();
}

}  // namespace

// The constants the Python side mirrors (ops/glm.py checks them on first use): 0 rows of a chunk,
// 1 workgroups of the pass, 2 the widest row of the one-output pass, 3 rows of a cross-entropy
// chunk, 4 its workgroups, 5 its most classes, 6 its widest row, 7 the largest batch of the
// one-launch solver, 8 its longest argument. -1 for any other index.
HARP_EXPORT int harp_glm_param(int which) {
  switch (which) {
    case 0: return GLM_CHUNK;
    case 1: return GLM_GRID;
    case 2: return GLM_MAX_D;
    case 3: return GLM_CE_ROWS;
    case 4: return GLM_CE_GRID;
    case 5: return GLM_CE_MAX_K;
    case 6: return GLM_CE_MAX_D;
    case 7: return GLM_SOLVER_MAX_BATCH;
    case 8: return GLM_SOLVER_MAX_DIM;
    default: return -1;
  }
}

// One pass over m rows of X [n, d] (dtype 0 bf16 / 1 fp32 / 2 fp64, row stride ldx >= d elements):
// all n rows in order (idx null, m == n) or the rows idx[0 .. m) (int32). y: fp64 [n], targets or
// class ids. w: the fp64 argument, [icpt + d] (kind 0 MSE, 1 logistic loss) or [K, icpt + d] (kind 2
// cross-entropy), the intercept first when icpt != 0. partial: fp64 [min(grid, chunks), len] with
// len = 1 + icpt + d or 1 + K (icpt + d), every element written: the value, then the gradient.
HARP_EXPORT int harp_glm_pass(const void* X, int dtype, long n, long ldx, int d, const double* y, const double* w,
                              int icpt, int kind, int K, const int* idx, long m, double* partial, hipStream_t s) {
  if (n < 1 || m < 1 || d < 1 || ldx < d || !X || !y || !w || !partial || (!idx && m != n)) return HARP_EBADARG;
  if (dtype < 0 || dtype > 2 || kind < 0 || kind > 2) return HARP_EUNSUPPORTED;
  icpt = icpt ? 1 : 0;
  if (kind == GLM_CE) {
    if (K < 1 || K > GLM_CE_MAX_K || d > GLM_CE_MAX_D) return HARP_EUNSUPPORTED;
    if (dtype == 0) return launch_ce<InBf16>(X, n, ldx, d, K, y, w, icpt, idx, m, partial, s);
    if (dtype == 1) return launch_ce<InFp32>(X, n, ldx, d, K, y, w, icpt, idx, m, partial, s);
    return launch_ce<InFp64>(X, n, ldx, d, K, y, w, icpt, idx, m, partial, s);
  }
  if (d > GLM_MAX_D) return HARP_EUNSUPPORTED;
  if (dtype == 0) return launch_pass<InBf16>(GLM_PASS_ARGS);
  if (dtype == 1) return launch_pass<InFp32>(GLM_PASS_ARGS);
  return launch_pass<InFp64>(GLM_PASS_ARGS);
}

// record [len] = the nb partial rows added in row order
HARP_EXPORT int harp_glm_reduce(const double* partial, int nb, int len, double* record, hipStream_t s) {
  if (!partial || !record || nb < 1 || len < 1) return HARP_EBADARG;
  reduce_kernel<<<dim3((unsigned)((len + 255) / 256)), dim3(256), 0, s>>>(partial, nb, len, record);
  return harp_launch_status();
}

// A whole run of sgd (method 0) or adagrad (method 1) on MSE (kind 0) or logistic loss (kind 1) over
// X [n, d], y fp64 [n]. table: int32 [iterations, batch], the rows of every step; lr: fp64
// [iterations]; gamma: fp64 [iterations], the conservative sequence, or null. x: fp64 [icpt + d], the
// start on entry and the result on return; niter: int32 [1], the iterations performed. One workgroup.
HARP_EXPORT int harp_solver_run(const void* X, int dtype, long n, long ldx, int d, const double* y, int icpt, int kind,
                                int method, const int* table, int iterations, int batch, const double* lr,
                                const double* gamma, int inner, double momentum, double l2, double threshold,
                                double eps, double* x, int* niter, hipStream_t s) {
  if (n < 1 || d < 1 || ldx < d || !X || !y || !table || !lr || !x || !niter || iterations < 1 || batch < 1 ||
      inner < 1)
    return HARP_EBADARG;
  if (dtype < 0 || dtype > 2 || kind < 0 || kind > 1 || method < 0 || method > 1 || d > GLM_MAX_D ||
      batch > GLM_SOLVER_MAX_BATCH)
    return HARP_EUNSUPPORTED;
  SolverArgs p;
  p.n = n, p.ldx = ldx, p.d = d, p.icpt = icpt ? 1 : 0, p.kind = kind, p.method = method;
  p.iterations = iterations, p.batch = batch, p.inner = inner;
  p.momentum = momentum, p.l2 = l2, p.threshold = threshold, p.eps = eps;
  const dim3 g(1), b(GLM_THREADS);
  if (dtype == 0)
    solver_kernel<InBf16><<<g, b, 0, s>>>((const uint16_t*)X, y, table, lr, gamma, p, x, niter);
  else if (dtype == 1)
    solver_kernel<InFp32><<<g, b, 0, s>>>((const float*)X, y, table, lr, gamma, p, x, niter);
  else
    solver_kernel<InFp64><<<g, b, 0, s>>>((const double*)X, y, table, lr, gamma, p, x, niter);
  return harp_launch_status();
}
