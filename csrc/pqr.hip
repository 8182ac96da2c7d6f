// Column-pivoted Householder QR of one small fp64 matrix (d <= 128) for gfx950: the step
// that turns the R factor of a tall-skinny QR into a rank-revealing one. For X = Q1 R1 every
// pivot decision of X depends on R1 alone (the residual column norms of X and of R1 are the
// same), so X P = Q1 (R1 P) = (Q1 Q2) R2 and only this d x d problem is left: latency-bound,
// one launch, no pass over the rows (harp_amd/ops/pqr.py, stats.pivoted_qr engine="native").
//
// A[:, perm] = Q2 R2, R2 upper triangular with a non-negative diagonal (the convention of
// house_tsqr), Q2 explicit.
//
// Pivot rule: at step k the free column with the largest squared norm over rows k..d-1, the
// norm formed fresh from the current entries (no downdating, so no cancellation safeguard),
// ties to the lowest current slot. Slots are swapped as LAPACK swaps columns k and pivot, but
// only the slot numbers move: a column stays with its owner. Reflector: LAPACK's dlarfg form
// with the unscaled norm of tsqr.hip (the caller pre-scales by a power of two); a zero
// residual gives tau = 0.
//
// Two forms, both plain stores only and bitwise repeatable:
//  * d <= 64, one wave (widths 8 / 16 / 32 / 64 of harp_tsqr_width): lane j holds column j in
//    registers, loops over rows fully unrolled (static register indices), no barrier. The
//    (norm, slot) argmax runs on the DPP network, the pivot column's tail is broadcast by
//    wave-uniform lane reads, dot product and rank-1 update are lane-local. Reflectors and tau
//    are kept in LDS; after R2 is stored the same registers hold the columns of I and the
//    reflectors are applied backwards from LDS broadcast reads.
//  * 64 < d <= 128, one workgroup: the matrix column-major in LDS (leading dimension 129: the
//    64 lanes of a wave hold 64 neighbouring columns at one row, 64 different banks), PQR_G
//    threads per column, each with the rows r = g mod PQR_G. Column sums go through [G][128]
//    partials in LDS and are added in one fixed order by every thread of the column. The
//    reflector stays in place below the diagonal of its column, where every column reads it
//    (a broadcast read); Q2 is then built in the same buffer as LAPACK's dorg2r does. With the
//    partial buffers the workgroup takes 148 KB of the CU's 160 KB of LDS at d = 128.
#include "common.h"

extern "C" int harp_tsqr_width(int d);

namespace {

constexpr int PQR_MAX_D = 128;
constexpr int PQR_T = 1024;             // threads of the workgroup form
constexpr int PQR_G = PQR_T / PQR_MAX_D;  // threads per column
constexpr int PQR_LDC = PQR_MAX_D + 1;  // leading dimension of the LDS matrix

// dlarfg on (alpha, sum of squares below it): H = I - tau v v^T, v = [1; x * sc], H [alpha; x] = [beta; 0]
__device__ __forceinline__ void reflector(double alpha, double sig, double& beta, double& tau, double& sc) {
  beta = alpha;
  tau = 0.0;
  sc = 0.0;
  if (sig > 0.0) {
    beta = -copysign(sqrt(alpha * alpha + sig), alpha);
    tau = (beta - alpha) / beta;
    sc = 1.0 / (alpha - beta);
  }
}

// ---------------------------------------------------------------- one wave, d <= W <= 64
template <int W>
__global__ __launch_bounds__(64) void pqr_wave_kernel(const double* __restrict__ A, long ld, int d,
                                                      double* __restrict__ Q2, double* __restrict__ R2,
                                                      int* __restrict__ perm) {
  __shared__ double vs[W * W];  // reflector k: vs[k * W + r], 0 above row k and 1 on it
  __shared__ double taus[W];
  __shared__ double sgs[W];  // sign that makes R2[k, k] non-negative
  const int lane = threadIdx.x;
  const bool mine = lane < d;
  double a[W];
#pragma unroll
  for (int r = 0; r < W; ++r) a[r] = (mine && r < d) ? A[r * ld + lane] : 0.0;
  int slot = lane;  // where LAPACK's swaps would have put this column by now
  // the step loop is not unrolled (W^2 code): a[k] with a runtime k is a select chain
#pragma unroll 1
  for (int k = 0; k < d; ++k) {
    double alpha = 0.0, sig = 0.0;
#pragma unroll
    for (int r = 0; r < W; ++r) {
      alpha = r == k ? a[r] : alpha;
      sig += r > k ? a[r] * a[r] : 0.0;
    }
    const bool free_col = mine && slot >= k;
    double best = free_col ? alpha * alpha + sig : -__builtin_inf();
    int bslot = free_col ? slot : 0x7fffffff;
    wave_arg_dpp<true>(best, bslot);
    // (a NaN norm can leave no winner: lane 0 then, the caller refuses non-finite input)
    const unsigned long long won = __ballot(slot == bslot);
    const int p = __builtin_amdgcn_readfirstlane(won ? __ffsll(won) - 1 : 0);
    bslot = won ? bslot : k;
    double beta, tau, sc;
    reflector(readlane_d(alpha, p), readlane_d(sig, p), beta, tau, sc);
    if (slot == k) slot = bslot;
    if (lane == p) slot = k;
    double v[W];
    double w = 0.0;
#pragma unroll
    for (int r = 0; r < W; ++r) {
      const double x = readlane_d(a[r], p) * sc;
      v[r] = r < k ? 0.0 : (r == k ? 1.0 : x);
      w += v[r] * a[r];
    }
    const double tw = (mine && slot > k) ? tau * w : 0.0;
#pragma unroll
    for (int r = 0; r < W; ++r) {
      const double mine_r = r == k ? beta : (r > k ? 0.0 : a[r]);  // the pivot column, reduced
      a[r] = lane == p ? mine_r : a[r] - tw * v[r];
    }
    if (lane == 0) {
#pragma unroll
      for (int r = 0; r < W; ++r) vs[k * W + r] = v[r];
      taus[k] = tau;
      sgs[k] = beta < 0.0 ? -1.0 : 1.0;
    }
  }
  lds_sync_wave();
  if (mine) {
    perm[slot] = lane;
#pragma unroll
    for (int r = 0; r < W; ++r)
      if (r < d) R2[r * d + slot] = r <= slot ? a[r] * sgs[r] : 0.0;
  }
  // Q2 = H_0 ... H_{d-1} I, this lane's column
#pragma unroll
  for (int r = 0; r < W; ++r) a[r] = r == lane ? 1.0 : 0.0;
#pragma unroll 1
  for (int k = d - 1; k >= 0; --k) {
    double v[W];
    double w = 0.0;
#pragma unroll
    for (int r = 0; r < W; ++r) {
      v[r] = vs[k * W + r];
      w += v[r] * a[r];
    }
    const double tw = taus[k] * w;
#pragma unroll
    for (int r = 0; r < W; ++r) a[r] -= tw * v[r];
  }
  if (mine) {
    const double sg = sgs[lane];
#pragma unroll
    for (int r = 0; r < W; ++r)
      if (r < d) Q2[r * d + lane] = a[r] * sg;
  }
}

// ---------------------------------------------------------------- one workgroup, d <= 128
__host__ __device__ constexpr size_t pqr_block_lds(int d) {
  // matrix, two [G][128] partial buffers, tau, sign, block_arg's values; then its indices and
  // the column of every step. At d = 128: 132,096 B of matrix + 19,136 B = 151,232 B of the
  // CU's 163,840 B, so 12,608 B are left
  return ((size_t)d * PQR_LDC + 2 * PQR_G * PQR_MAX_D + 2 * PQR_MAX_D + 16) * sizeof(double) +
         (16 + PQR_MAX_D) * sizeof(int);
}

// smallest row above k among this thread's rows (r = g mod PQR_G)
__device__ __forceinline__ int first_row_above(int k, int g) { return g > k ? g : g + ((k - g) / PQR_G + 1) * PQR_G; }

__global__ __launch_bounds__(PQR_T) void pqr_block_kernel(const double* __restrict__ A, long ld, int d,
                                                          double* __restrict__ Q2, double* __restrict__ R2,
                                                          int* __restrict__ perm) {
  extern __shared__ double sm[];
  double* M = sm;  // element (r, c) at c * PQR_LDC + r
  double* partN = M + d * PQR_LDC;
  double* partD = partN + PQR_G * PQR_MAX_D;
  double* taus = partD + PQR_G * PQR_MAX_D;
  double* sgs = taus + PQR_MAX_D;
  double* sv = sgs + PQR_MAX_D;
  int* si = (int*)(sv + 16);
  int* colof = si + 16;  // the column reduced at step k
  const int t = threadIdx.x, c = t & (PQR_MAX_D - 1), g = t / PQR_MAX_D, lane = t & 63, wv = t >> 6;
  const bool mine = c < d;
  for (int i = t; i < d * d; i += PQR_T) {
    const int r = i / d, cc = i - r * d;
    M[cc * PQR_LDC + r] = A[r * ld + cc];
  }
  __syncthreads();
  double* col = M + (mine ? c : 0) * PQR_LDC;  // touched only where mine
  int slot = c;
  for (int k = 0; k < d; ++k) {
    const int r0 = first_row_above(k, g);
    const bool krow = g == (k & (PQR_G - 1));  // this thread has row k
    double s = 0.0;
    if (mine)
      for (int r = r0; r < d; r += PQR_G) s += col[r] * col[r];
    partN[g * PQR_MAX_D + c] = s;
    __syncthreads();
    double sig = 0.0;
#pragma unroll
    for (int q = 0; q < PQR_G; ++q) sig += partN[q * PQR_MAX_D + c];
    const double alpha = mine ? col[k] : 0.0;
    const bool free_col = mine && slot >= k;
    double best = free_col ? alpha * alpha + sig : -__builtin_inf();
    int bi = free_col ? (slot << 8 | c) : 0x7fffffff;  // ordered by slot, and names the column
    block_arg<true, PQR_T>(best, bi, sv, si, lane, wv);
    const bool won = bi != 0x7fffffff;  // false only for NaN norms, which the caller refuses
    const int p = won ? bi & 255 : 0, pslot = won ? bi >> 8 : k;
    double* vp = M + p * PQR_LDC;
    double psig = 0.0;
#pragma unroll
    for (int q = 0; q < PQR_G; ++q) psig += partN[q * PQR_MAX_D + p];
    double beta, tau, sc;
    reflector(vp[k], psig, beta, tau, sc);
    if (slot == k) slot = pslot;
    if (c == p) {
      slot = k;
      for (int r = r0; r < d; r += PQR_G) col[r] *= sc;  // the reflector's tail, in place
    }
    if (t == 0) {
      taus[k] = tau;
      sgs[k] = beta < 0.0 ? -1.0 : 1.0;
      colof[k] = p;
    }
    __syncthreads();  // the tail is published; every thread has read vp[k]
    if (c == p && krow) col[k] = beta;
    const bool upd = mine && slot > k;
    double w = 0.0;
    if (upd) {
      if (krow) w = col[k];
      for (int r = r0; r < d; r += PQR_G) w += vp[r] * col[r];
    }
    partD[g * PQR_MAX_D + c] = w;
    __syncthreads();
    if (upd) {
      double ws = 0.0;
#pragma unroll
      for (int q = 0; q < PQR_G; ++q) ws += partD[q * PQR_MAX_D + c];
      const double tw = tau * ws;
      if (krow) col[k] -= tw;
      for (int r = r0; r < d; r += PQR_G) col[r] -= tw * vp[r];
    }
  }
  __syncthreads();
  if (mine) {
    if (g == 0) perm[slot] = c;
    for (int r = g; r < d; r += PQR_G) R2[r * d + slot] = r <= slot ? col[r] * sgs[r] : 0.0;
  }
  __syncthreads();
  // Q2 in place (dorg2r): the column of step k becomes H_k e_k after H_k went over the
  // columns of the later steps
  for (int k = d - 1; k >= 0; --k) {
    const int r0 = first_row_above(k, g);
    const bool krow = g == (k & (PQR_G - 1));
    const int p = colof[k];
    const double tau = taus[k];
    const double* vp = M + p * PQR_LDC;
    const bool upd = mine && slot > k;
    double w = 0.0;
    if (upd) {
      if (krow) w = col[k];
      for (int r = r0; r < d; r += PQR_G) w += vp[r] * col[r];
    }
    partD[g * PQR_MAX_D + c] = w;
    __syncthreads();
    if (upd) {
      double ws = 0.0;
#pragma unroll
      for (int q = 0; q < PQR_G; ++q) ws += partD[q * PQR_MAX_D + c];
      const double tw = tau * ws;
      if (krow) col[k] -= tw;
      for (int r = r0; r < d; r += PQR_G) col[r] -= tw * vp[r];
    }
    __syncthreads();  // every reader of the reflector is done
    if (c == p)
      for (int r = g; r < d; r += PQR_G) col[r] = r < k ? 0.0 : (r == k ? 1.0 - tau : -tau * col[r]);
  }
  __syncthreads();
  if (mine) {
    const double sg = sgs[slot];
    for (int r = g; r < d; r += PQR_G) Q2[r * d + slot] = col[r] * sg;
  }
}

template <int W>
int launch_wave(const double* A, long ld, int d, double* Q2, double* R2, int* perm, hipStream_t s) {
  pqr_wave_kernel<W><<<dim3(1), dim3(64), 0, s>>>(A, ld, d, Q2, R2, perm);
  return harp_launch_status();
}

}  // namespace

HARP_EXPORT int harp_pqr_max_d() { return PQR_MAX_D; }

// Column-pivoted QR of A [d, d] (row-major, leading dimension ld): Q2 [d, d], R2 [d, d],
// perm [d] (int32), A[:, perm] = Q2 R2.
HARP_EXPORT int harp_pqr_small(const double* A, long ld, int d, double* Q2, double* R2, int* perm, hipStream_t s) {
  if (d < 1 || d > PQR_MAX_D || ld < d || !A || !Q2 || !R2 || !perm) return HARP_EBADARG;
  if (d <= 64) {
    switch (harp_tsqr_width(d)) {
      case 8: return launch_wave<8>(A, ld, d, Q2, R2, perm, s);
      case 16: return launch_wave<16>(A, ld, d, Q2, R2, perm, s);
      case 32: return launch_wave<32>(A, ld, d, Q2, R2, perm, s);
      case 64: return launch_wave<64>(A, ld, d, Q2, R2, perm, s);
      default: return HARP_EUNSUPPORTED;
    }
  }
  const size_t lds = pqr_block_lds(d);
  if (lds > 65536 && hipFuncSetAttribute((const void*)pqr_block_kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                                         (int)lds) != hipSuccess)
    return HARP_ELAUNCH;
  pqr_block_kernel<<<dim3(1), dim3(PQR_T), lds, s>>>(A, ld, d, Q2, R2, perm);
  return harp_launch_status();
}
