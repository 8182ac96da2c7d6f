// One-sided (Hestenes) Jacobi SVD of one small square fp64 matrix (d <= 128) for gfx950: the
// d x d step of the native SVD. For a tall block X = Q R only the factor R is left to
// decompose: latency-bound, one launch, nothing leaves the device (harp_amd/ops/jsvd.py,
// stats.svd / stats.pca(method="svd") with engine="native").
//
// M = Z diag(s) W^T: plane rotations from the right make the columns of M orthogonal, W
// accumulates them (it starts as I), s are the column norms in descending order and Z the
// normalised columns. A column of exactly zero norm gives s = 0 and a ZERO column of Z (Z is
// not completed to a basis); tiny non-zero columns come out orthonormal, because the stopping
// rule is relative.
//
// Rules (the same in the torch mirror of ops/jsvd.py):
//  * pair (p, q), p < q: alpha = |m_p|^2, beta = |m_q|^2, gamma = m_p . m_q, all three formed
//    fresh from the current columns at every visit (no norm downdating);
//  * skipped when |gamma| <= tol sqrt(alpha beta), tol = sqrt(d) 2^-53 (LAPACK dgesvj's
//    threshold); a zero column has gamma = 0 and never rotates;
//  * else zeta = (beta - alpha) / (2 gamma), t = sign(zeta) / (|zeta| + sqrt(1 + zeta^2)), t = 1
//    for zeta = 0, c = 1 / sqrt(1 + t^2), sn = c t, m_p' = c m_p - sn m_q, m_q' = sn m_p + c m_q;
//  * order: the round-robin tournament over Wp = d rounded up to even slots. At step s in
//    0 .. Wp-2 slot i < Wp-1 meets (2 s - i) mod (Wp-1), slot s (which would meet itself) meets
//    slot Wp-1: closed form per lane, every pair once per sweep, Wp/2 disjoint pairs per step.
//    The padding column is zero and never rotates;
//  * a sweep without a rotation ends the iteration; *sweeps is the number of sweeps run (the
//    clean one included), or -1 after JSVD_MAX_SWEEPS;
//  * epilogue: sigma_j = sqrt(|m_j|^2), rank of column j = #{k: sigma_k > sigma_j, or sigma_k ==
//    sigma_j and k < j}; s[rank] = sigma_j, Z[:, rank] = m_j / sigma_j, W[:, rank] = w_j. No
//    host-side sort.
//
// There is no MFMA here and none to look for: a rotation is level-1 work on one column pair
// and has no matrix-instruction shape.
//
// Two forms. Columns never move, only the partner index changes. Plain vector stores only, no
// atomics; both lanes (groups) of a pair form alpha, beta, gamma from the same products in the
// same order, so they hold bit-identical c and sn and each rotates its own side: the kernel is
// bitwise repeatable.
//  * d <= 64, one wave (register widths 8 / 16 / 32 / 64 of harp_tsqr_width): lane j keeps
//    column j of M and of W in registers (2 x 64 doubles at W = 64), row loops fully unrolled,
//    the step loop not. The partner's column is fetched row by row with lane permutes
//    (ds_bpermute: the LDS crossbar, no LDS memory); the dot pass uses each fetched value at
//    once, the update pass fetches again and rewrites a[r] in the same instruction slot on both
//    lanes, so both sides read old values. No cross-lane reduction, no barrier, no LDS; the
//    "any rotation" flag is a ballot, and a step without a rotation skips its update pass.
//    WANT_W is a template parameter: without it the W registers and half the permutes vanish.
//  * 64 < d <= 128, one workgroup of 1024 threads, 8 lanes per column: lane g holds the rows
//    r = g mod 8 of its M and W column (16 + 16 doubles). Per step every group stores its M
//    column into one LDS exchange buffer (128 columns, leading dimension 136: the 8 columns x
//    8 rows that a wave stores at once then cover every pair of banks exactly twice, the
//    two-pass minimum of a 64-lane 8-byte access; 139,264 B of the CU's 160 KB),
//    barrier, each group reads its partner's column, forms the three partial sums over its 16
//    rows and adds them over the 8 lanes in one fixed DPP order (quad_perm xor 1, xor 2,
//    row_half_mirror; each step adds two values that both sides hold, so all 8 lanes and the
//    partner's 8 lanes agree bitwise). The group rotates its M column in registers; after a
//    barrier the same buffer carries the W columns. The sweep flag is an LDS word that every
//    rotating group sets.
#include "common.h"

extern "C" int harp_tsqr_width(int d);

namespace {

constexpr int JSVD_MAX_D = 128;
constexpr int JSVD_MAX_SWEEPS = 60;
constexpr int JSVD_T = 1024;                  // threads of the workgroup form
constexpr int JSVD_G = JSVD_T / JSVD_MAX_D;   // lanes per column
constexpr int JSVD_R = JSVD_MAX_D / JSVD_G;   // rows per lane
constexpr int JSVD_LDC = JSVD_MAX_D + 8;      // leading dimension of the exchange buffer
constexpr size_t JSVD_LDS = (size_t)JSVD_MAX_D * JSVD_LDC * sizeof(double) + 16;

// slot i's partner at step s of the tournament over n + 1 slots (n odd); slots above n idle
__device__ __forceinline__ int partner_of(int i, int s, int n) {
  int p = 2 * s - i;  // in [-(n-1), 2(n-1)] for i, s < n
  p = p < 0 ? p + n : (p >= n ? p - n : p);
  p = i == s ? n : p;
  p = i == n ? s : p;
  return i > n ? i : p;
}

// the rotation of a pair, or false when the pair is skipped
__device__ __forceinline__ bool rotation(double alpha, double beta, double gamma, double tol, double& c, double& sn) {
  c = 1.0;
  sn = 0.0;
  if (!(fabs(gamma) > tol * sqrt(alpha * beta))) return false;
  const double zeta = (beta - alpha) / (2.0 * gamma);
  const double t = zeta == 0.0 ? 1.0 : copysign(1.0, zeta) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
  c = 1.0 / sqrt(1.0 + t * t);
  sn = c * t;
  return true;
}

// lane (addr / 4)'s value of v; every lane of the wave must be active
__device__ __forceinline__ double lane_fetch_d(double v, int addr) {
  const unsigned long long u = __builtin_bit_cast(unsigned long long, v);
  const unsigned lo = (unsigned)__builtin_amdgcn_ds_bpermute(addr, (int)(unsigned)u);
  const unsigned hi = (unsigned)__builtin_amdgcn_ds_bpermute(addr, (int)(unsigned)(u >> 32));
  return __builtin_bit_cast(double, ((unsigned long long)hi << 32) | lo);
}

// ---------------------------------------------------------------- one wave, d <= W <= 64
template <int W, bool WANT_W>
__global__ __launch_bounds__(64) void jsvd_wave_kernel(const double* __restrict__ M, long ld, int d, double tol,
                                                       double* __restrict__ Z, double* __restrict__ S,
                                                       double* __restrict__ Wout, int* __restrict__ sweeps) {
  const int lane = threadIdx.x;
  const bool mine = lane < d;
  const int n = ((d + 1) & ~1) - 1;
  double a[W], w[WANT_W ? W : 1];
#pragma unroll
  for (int r = 0; r < W; ++r) a[r] = (mine && r < d) ? M[r * ld + lane] : 0.0;
  if (WANT_W) {
#pragma unroll
    for (int r = 0; r < W; ++r) w[r] = r == lane ? 1.0 : 0.0;
  }
  int done = -1;
#pragma unroll 1
  for (int sweep = 1; sweep <= JSVD_MAX_SWEEPS; ++sweep) {
    unsigned long long any = 0;
    // the step loop is not unrolled (W^2 code)
#pragma unroll 1
    for (int s = 0; s < n; ++s) {
      const int pr = partner_of(lane, s, n);
      const int addr = pr << 2;
      double own2 = 0.0, oth2 = 0.0, gam = 0.0;
#pragma unroll
      for (int r = 0; r < W; ++r) {
        const double b = lane_fetch_d(a[r], addr);
        own2 = fma(a[r], a[r], own2);
        oth2 = fma(b, b, oth2);
        gam = fma(a[r], b, gam);
      }
      const bool lo = lane < pr;
      double c, sn;
      const bool rot = rotation(lo ? own2 : oth2, lo ? oth2 : own2, gam, tol, c, sn) && pr != lane;
      const unsigned long long m = __ballot(rot);
      if (m == 0) continue;  // wave-uniform
      any |= m;
      const double ssn = lo ? -sn : sn;
#pragma unroll
      for (int r = 0; r < W; ++r) {
        const double b = lane_fetch_d(a[r], addr);
        a[r] = rot ? fma(ssn, b, c * a[r]) : a[r];
      }
      if (WANT_W) {
#pragma unroll
        for (int r = 0; r < W; ++r) {
          const double b = lane_fetch_d(w[r], addr);
          w[r] = rot ? fma(ssn, b, c * w[r]) : w[r];
        }
      }
    }
    if (any == 0) {
      done = sweep;
      break;
    }
  }
  double nrm2 = 0.0;
#pragma unroll
  for (int r = 0; r < W; ++r) nrm2 = fma(a[r], a[r], nrm2);
  const double sig = sqrt(nrm2);
  int rank = 0;
#pragma unroll 1
  for (int k = 0; k < d; ++k) {
    const double sk = readlane_d(sig, k);
    rank += (sk > sig || (sk == sig && k < lane)) ? 1 : 0;
  }
  if (mine) {
    S[rank] = sig;
#pragma unroll
    for (int r = 0; r < W; ++r) {
      if (r < d) {
        Z[r * d + rank] = sig > 0.0 ? a[r] / sig : 0.0;
        if (WANT_W) Wout[r * d + rank] = w[r];
      }
    }
  }
  if (lane == 0) *sweeps = done;
}

// ---------------------------------------------------------------- one workgroup, d <= 128
// sum over the 8 lanes of a column's group, the same bits in all 8 lanes
__device__ __forceinline__ double group_sum(double v) {
  v += dpp_mov_d<0xB1>(v);   // quad_perm [1,0,3,2]
  v += dpp_mov_d<0x4E>(v);   // quad_perm [2,3,0,1]
  v += dpp_mov_d<0x141>(v);  // row_half_mirror: the other quad of the 8 lanes
  return v;
}

template <bool WANT_W>
__global__ __launch_bounds__(JSVD_T) void jsvd_block_kernel(const double* __restrict__ M, long ld, int d, double tol,
                                                            double* __restrict__ Z, double* __restrict__ S,
                                                            double* __restrict__ Wout, int* __restrict__ sweeps) {
  extern __shared__ double ex[];  // column c at ex + c * JSVD_LDC, all 128 columns addressable
  int* flag = (int*)(ex + JSVD_MAX_D * JSVD_LDC);
  const int t = threadIdx.x, col = t / JSVD_G, g = t % JSVD_G;
  const bool mine = col < d;
  const int n = ((d + 1) & ~1) - 1;
  double a[JSVD_R], w[WANT_W ? JSVD_R : 1];
#pragma unroll
  for (int i = 0; i < JSVD_R; ++i) {
    const int r = g + i * JSVD_G;
    a[i] = (mine && r < d) ? M[r * ld + col] : 0.0;
    if (WANT_W) w[i] = r == col ? 1.0 : 0.0;
  }
  double* own = ex + col * JSVD_LDC + g;
  if (t == 0) *flag = 0;  // ordered before the first set by the barrier of step 0
  int done = -1;
#pragma unroll 1
  for (int sweep = 1; sweep <= JSVD_MAX_SWEEPS; ++sweep) {
#pragma unroll 1
    for (int s = 0; s < n; ++s) {
      const int pr = partner_of(col, s, n);
      const double* oth = ex + pr * JSVD_LDC + g;
#pragma unroll
      for (int i = 0; i < JSVD_R; ++i) own[i * JSVD_G] = a[i];
      __syncthreads();
      double own2 = 0.0, oth2 = 0.0, gam = 0.0;
#pragma unroll
      for (int i = 0; i < JSVD_R; ++i) {
        const double b = oth[i * JSVD_G];
        own2 = fma(a[i], a[i], own2);
        oth2 = fma(b, b, oth2);
        gam = fma(a[i], b, gam);
      }
      own2 = group_sum(own2);
      oth2 = group_sum(oth2);
      gam = group_sum(gam);
      const bool lo = col < pr;
      double c, sn;
      const bool rot = rotation(lo ? own2 : oth2, lo ? oth2 : own2, gam, tol, c, sn) && pr != col;
      const double ssn = lo ? -sn : sn;
      if (rot) {  // the partner's column is read again: 16 more doubles alive would spill
#pragma unroll
        for (int i = 0; i < JSVD_R; ++i) a[i] = fma(ssn, oth[i * JSVD_G], c * a[i]);
        if (g == 0) *flag = 1;
      }
      if (WANT_W) {
        __syncthreads();  // every reader of the M columns is done
#pragma unroll
        for (int i = 0; i < JSVD_R; ++i) own[i * JSVD_G] = w[i];
        __syncthreads();
        if (rot) {
#pragma unroll
          for (int i = 0; i < JSVD_R; ++i) w[i] = fma(ssn, oth[i * JSVD_G], c * w[i]);
        }
      }
      __syncthreads();  // every reader of the buffer is done
    }
    const int any = *flag;
    __syncthreads();
    if (any == 0) {
      done = sweep;
      break;
    }
    if (t == 0) *flag = 0;  // ordered before the next set by the barrier of step 0
  }
  double nrm2 = 0.0;
#pragma unroll
  for (int i = 0; i < JSVD_R; ++i) nrm2 = fma(a[i], a[i], nrm2);
  const double sig = sqrt(group_sum(nrm2));
  if (g == 0) ex[col] = sig;
  __syncthreads();
  int rank = 0;
  for (int k = 0; k < d; ++k) {
    const double sk = ex[k];
    rank += (sk > sig || (sk == sig && k < col)) ? 1 : 0;
  }
  if (mine) {
    if (g == 0) S[rank] = sig;
#pragma unroll
    for (int i = 0; i < JSVD_R; ++i) {
      const int r = g + i * JSVD_G;
      if (r < d) {
        Z[r * d + rank] = sig > 0.0 ? a[i] / sig : 0.0;
        if (WANT_W) Wout[r * d + rank] = w[i];
      }
    }
  }
  if (t == 0) *sweeps = done;
}

template <int W>
int launch_wave(const double* M, long ld, int d, int want_w, double tol, double* Z, double* S, double* Wout,
                int* sweeps, hipStream_t st) {
  if (want_w)
    jsvd_wave_kernel<W, true><<<dim3(1), dim3(64), 0, st>>>(M, ld, d, tol, Z, S, Wout, sweeps);
  else
    jsvd_wave_kernel<W, false><<<dim3(1), dim3(64), 0, st>>>(M, ld, d, tol, Z, S, Wout, sweeps);
  return harp_launch_status();
}

template <bool WANT_W>
int launch_block(const double* M, long ld, int d, double tol, double* Z, double* S, double* Wout, int* sweeps,
                 hipStream_t st) {
  if (hipFuncSetAttribute((const void*)jsvd_block_kernel<WANT_W>, hipFuncAttributeMaxDynamicSharedMemorySize,
                          (int)JSVD_LDS) != hipSuccess)
    return HARP_ELAUNCH;
  jsvd_block_kernel<WANT_W><<<dim3(1), dim3(JSVD_T), JSVD_LDS, st>>>(M, ld, d, tol, Z, S, Wout, sweeps);
  return harp_launch_status();
}

}  // namespace

HARP_EXPORT int harp_jsvd_max_d() { return JSVD_MAX_D; }

// SVD of M [d, d] (row-major, leading dimension ld): M = Z diag(s) W^T with Z [d, d], s [d]
// descending, W [d, d] (written only when want_w; may be null otherwise), sweeps [1] (int32).
HARP_EXPORT int harp_jsvd_small(const double* M, long ld, int d, int want_w, double* Z, double* s, double* W,
                                int* sweeps, hipStream_t st) {
  if (d < 1 || d > JSVD_MAX_D || ld < d || !M || !Z || !s || !sweeps || (want_w && !W)) return HARP_EBADARG;
  const double tol = sqrt((double)d) * 0x1p-53;
  if (d <= 64) {
    switch (harp_tsqr_width(d)) {
      case 8: return launch_wave<8>(M, ld, d, want_w, tol, Z, s, W, sweeps, st);
      case 16: return launch_wave<16>(M, ld, d, want_w, tol, Z, s, W, sweeps, st);
      case 32: return launch_wave<32>(M, ld, d, want_w, tol, Z, s, W, sweeps, st);
      case 64: return launch_wave<64>(M, ld, d, want_w, tol, Z, s, W, sweeps, st);
      default: return HARP_EUNSUPPORTED;
    }
  }
  return want_w ? launch_block<true>(M, ld, d, tol, Z, s, W, sweeps, st)
                : launch_block<false>(M, ld, d, tol, Z, s, W, sweeps, st);
}
