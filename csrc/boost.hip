// Boosting rounds on quantile-binned rows for gfx950 (MI355X / CDNA4): decision stump,
// AdaBoost (SAMME), LogitBoost and BrownBoost (ml/daal daal_stump, daal_adaboost,
// daal_logitboost, daal_brownboost).
//
// A boosted stump is the root level of a tree whose sample weights (AdaBoost, BrownBoost) or
// working responses (LogitBoost) changed since the last round. The features are binned once
// per fit (harp_forest_bin, uint8 [n, dpad], dpad = d rounded up to 16); a round is then ONE
// pass over the binned rows that applies the previous round's learner to every row and
// accumulates the root histogram of the new weights. The split search is the forest engine's
// (harp_forest_split_feature / harp_forest_split_node) on that histogram.
// harp_amd/ops/boost.py drives the rounds and holds the CPU torch mirror of every kernel
// here (the oracle of tests/test_boost_gpu.py).
//
// Everything a round needs from the previous split is read from device memory: the stump
// record and the weight multipliers are written by harp_boost_class_finish, the K regression
// stumps of a LogitBoost round by torch element-wise ops on the split kernel's outputs. The
// host reads one small record per AdaBoost round (for the stop tests) and nothing per
// LogitBoost round.
//
// round kernels. One workgroup per (2048-row chunk, feature group); a thread owns a row at a
// time: it recomputes the row's new weight (or the K working responses) from the read-only
// input buffer, then walks the row's 16-byte segments of the feature group and adds into the
// fp64 LDS cells (ds_add_f64); the cells are flushed once per chunk with one global atomic
// per non-zero cell. Every feature group recomputes the row values, only group 0 stores them
// (w_out / F_out are separate buffers: with one buffer group 0's stores would race with the
// other groups' loads). A feature group is as many features as fit 64 KiB of LDS; LogitBoost
// also splits the classes into groups when one feature of all classes does not fit. A row
// whose bin is >= B or whose label is outside [0, C) adds nothing. fp64 sums depend on arrival
// order in the last bits; the per-row outputs are element-wise and reproducible.
//
// BrownBoost line search. harp_boost_brown_sums evaluates up to 64 candidate steps (a, t) in
// one pass over (r, u): candidate per lane, rows strided over the waves, register
// accumulators, per-block partials summed in block order by a second kernel, so the sums are
// reproducible run to run (their signs steer a bisection). harp_boost_brown_step narrows the
// bracket of t to the sub-interval where the (monotone) potential crosses its target and
// writes the next 64 candidates: 10 passes of 64-way section reach the width of 60 bisection
// steps without a host read.
//
// No kernel waits on another workgroup; all stores are vector stores.
#include "common.h"

#pragma clang fp contract(off)

#define BOOST_CHUNK 2048
#define BOOST_LDS_BYTES 65536
#define BOOST_MAX_BINS 256
#define BOOST_MAX_CLASSES 32
#define BOOST_MAX_CAND 64
#define BOOST_SUM_BLOCKS 1024

namespace {

__device__ __forceinline__ int seg_byte(const uint4& v, int j) {
  const unsigned w = j < 4 ? v.x : j < 8 ? v.y : j < 12 ? v.z : v.w;
  return (int)((w >> ((j & 3) * 8)) & 0xffu);
}

// ------------------------------------------------------------------ class round
// rec = (feature, bin, left class, right class) of the previous stump, feature < 0: no update;
// mul = (mul_hit, mul_miss). r != null (BrownBoost): w = exp(-(r + s)^2 / c), scal = (s, c).
__global__ __launch_bounds__(256) void class_round_kernel(const uint8_t* __restrict__ Xb, int dpad, long n,
                                                          const int* __restrict__ y,
                                                          const double* __restrict__ w_in,
                                                          double* __restrict__ w_out, const int* __restrict__ rec,
                                                          const double* __restrict__ mul,
                                                          const double* __restrict__ r,
                                                          const double* __restrict__ scal, int d, int B, int C,
                                                          int dg, double* __restrict__ H) {
  extern __shared__ double boost_smem[];
  double* cell = boost_smem;
  const int f0 = (int)blockIdx.y * dg;
  const int nf = min(dg, d - f0);
  if (nf <= 0) return;  // block-uniform
  const int ncell = nf * B * C;
  for (int i = threadIdx.x; i < ncell; i += blockDim.x) cell[i] = 0.0;
  __syncthreads();
  int pf = -1, pbin = 0, pl = 0, pr = 0;
  double mh = 1.0, mm = 1.0, bs = 0.0, bc = 1.0;
  if (r) {
    bs = scal[0];
    bc = scal[1];
  } else {
    pf = rec[0];
    if (pf >= d) pf = -1;
    if (pf >= 0) {
      pbin = rec[1], pl = rec[2], pr = rec[3];
      mh = mul[0], mm = mul[1];
    }
  }
  const long row0 = (long)blockIdx.x * BOOST_CHUNK;
  const int rows = (int)min((long)BOOST_CHUNK, n - row0);
  const int s0 = f0 >> 4, s1 = (f0 + nf - 1) >> 4;
  for (int i = threadIdx.x; i < rows; i += blockDim.x) {
    const long row = row0 + i;
    const uint8_t* xr = Xb + row * dpad;
    const int cl = y[row];
    double w;
    if (r) {
      const double q = r[row] + bs;
      w = exp((-(q * q)) / bc);
    } else {
      w = w_in[row];
      if (pf >= 0) {
        const int pred = (int)xr[pf] > pbin ? pr : pl;
        w = w * (pred != cl ? mm : mh);
      }
    }
    if (blockIdx.y == 0 && w_out) w_out[row] = w;
    if (cl < 0 || cl >= C || w == 0.0) continue;
    for (int sg = s0; sg <= s1; ++sg) {
      const uint4 v = *reinterpret_cast<const uint4*>(xr + sg * 16);
#pragma unroll
      for (int j = 0; j < 16; ++j) {
        const int f = sg * 16 + j - f0;
        const int bin = seg_byte(v, j);
        if (f >= 0 && f < nf && bin < B) atomicAdd(&cell[(f * B + bin) * C + cl], w);
      }
    }
  }
  __syncthreads();
  double* dst = H + (size_t)f0 * B * C;
  for (int i = threadIdx.x; i < ncell; i += blockDim.x) {
    const double v = cell[i];
    if (v != 0.0) atomicAdd(&dst[i], v);
  }
}

// The unfused A/B of scripts/bench_boost.py: the weight update alone (one thread per row).
__global__ __launch_bounds__(256) void class_update_kernel(const uint8_t* __restrict__ Xb, int dpad, long n,
                                                           const int* __restrict__ y,
                                                           const double* __restrict__ w_in,
                                                           double* __restrict__ w_out, const int* __restrict__ rec,
                                                           const double* __restrict__ mul, int d) {
  const long row = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (row >= n) return;
  int pf = rec[0];
  if (pf >= d) pf = -1;
  double w = w_in[row];
  if (pf >= 0) {
    const int pred = (int)Xb[row * dpad + pf] > rec[1] ? rec[3] : rec[2];
    w = w * (pred != y[row] ? mul[1] : mul[0]);
  }
  w_out[row] = w;
}

// One wave; lane 0 turns the split of the root into the next round's stump record and
// multipliers. info = (split, feature, bin, left class, right class, err, alpha, S, L[C], R[C]).
__global__ __launch_bounds__(64) void class_finish_kernel(const int* __restrict__ bf, const int* __restrict__ bb,
                                                          const int* __restrict__ sp, const double* __restrict__ L,
                                                          const double* __restrict__ R, const double* __restrict__ T,
                                                          int C, double n, int* __restrict__ rec,
                                                          double* __restrict__ mul, double* __restrict__ info) {
  if (threadIdx.x != 0) return;
  double S = 0.0, mL = L[0], mR = R[0];
  int lc = 0, rc = 0;
  for (int c = 0; c < C; ++c) {
    S = S + T[c];
    if (L[c] > mL) mL = L[c], lc = c;
    if (R[c] > mR) mR = R[c], rc = c;
    info[8 + c] = L[c];
    info[8 + C + c] = R[c];
  }
  const double err = 1.0 - (mL + mR) / S;
  const double alpha = log((1.0 - err) / fmax(err, 1e-12)) + log((double)(C - 1));
  const double ea = exp(alpha);
  const double hit = n / (S * ((1.0 - err) + err * ea));
  const int split = sp[0];
  rec[0] = split ? bf[0] : -1;
  rec[1] = bb[0];
  rec[2] = lc;
  rec[3] = rc;
  mul[0] = hit;
  mul[1] = hit * ea;
  info[0] = (double)split;
  info[1] = (double)bf[0];
  info[2] = (double)bb[0];
  info[3] = (double)lc;
  info[4] = (double)rc;
  info[5] = err;
  info[6] = alpha;
  info[7] = S;
}

// ------------------------------------------------------------------ logit round
// rec_i [K, 2] = (feature, bin), rec_v [K, 2] = (v_left, v_right) of the previous round's K
// regression stumps; feature < 0: the constant v_left. Block y = feature group * ncg + class
// group; classes k0 .. k0 + kg - 1 accumulate, every block computes the full softmax.
__global__ __launch_bounds__(256) void logit_round_kernel(const uint8_t* __restrict__ Xb, int dpad, long n,
                                                          const int* __restrict__ y,
                                                          const double* __restrict__ F_in,
                                                          double* __restrict__ F_out,
                                                          const int* __restrict__ rec_i,
                                                          const double* __restrict__ rec_v, double zmax, int d,
                                                          int B, int K, int dg, int kg, int ncg,
                                                          double* __restrict__ H, double* __restrict__ wz) {
  extern __shared__ double boost_smem[];
  double* cell = boost_smem;
  const int fgi = (int)blockIdx.y / ncg, cgi = (int)blockIdx.y % ncg;
  const int f0 = fgi * dg, k0 = cgi * kg;
  const int nf = min(dg, d - f0), nk = min(kg, K - k0);
  if (nf <= 0 || nk <= 0) return;  // block-uniform
  const int ncell = nk * nf * B * 3;
  for (int i = threadIdx.x; i < ncell; i += blockDim.x) cell[i] = 0.0;
  __syncthreads();
  const long row0 = (long)blockIdx.x * BOOST_CHUNK;
  const int rows = (int)min((long)BOOST_CHUNK, n - row0);
  const double shrink = (double)(K - 1) / (double)K;
  const bool store = blockIdx.y == 0;
  for (int i = threadIdx.x; i < rows; i += blockDim.x) {
    const long row = row0 + i;
    const uint8_t* xr = Xb + row * dpad;
    const int cl = y[row];
    double fv[BOOST_MAX_CLASSES];
    double gs = 0.0;
#pragma unroll
    for (int k = 0; k < BOOST_MAX_CLASSES; ++k) {
      fv[k] = 0.0;
      if (k < K) {
        int f = rec_i[2 * k];
        if (f >= d) f = -1;
        const double g = (f >= 0 && (int)xr[f] > rec_i[2 * k + 1]) ? rec_v[2 * k + 1] : rec_v[2 * k];
        fv[k] = g;
        gs = gs + g;
      }
    }
    const double gm = gs / (double)K;
    double mx = -__builtin_inf();
#pragma unroll
    for (int k = 0; k < BOOST_MAX_CLASSES; ++k)
      if (k < K) {
        const double v = F_in[row * K + k] + shrink * (fv[k] - gm);
        fv[k] = v;
        mx = fmax(mx, v);
        if (store) F_out[row * K + k] = v;
      }
    double se = 0.0;
#pragma unroll
    for (int k = 0; k < BOOST_MAX_CLASSES; ++k)
      if (k < K) {
        fv[k] = exp(fv[k] - mx);
        se = se + fv[k];
      }
#pragma unroll
    for (int k = 0; k < BOOST_MAX_CLASSES; ++k) {
      if (k >= K) continue;
      const bool mine = k >= k0 && k < k0 + nk;
      if (!mine && !(store && wz)) continue;
      const double p = fv[k] / se;
      const double w = fmax(p * (1.0 - p), 1e-12);
      const double z = fmin(fmax(((cl == k ? 1.0 : 0.0) - p) / w, -zmax), zmax);
      if (store && wz) {
        wz[(row * K + k) * 2] = w;
        wz[(row * K + k) * 2 + 1] = z;
      }
      if (!mine || cl < 0 || cl >= K) continue;  // a row without a valid label adds nothing
      const double wzv = w * z, wzz = wzv * z;
      double* ck = cell + (size_t)(k - k0) * nf * B * 3;
      for (int f = 0; f < nf; ++f) {
        const int bin = xr[f0 + f];
        if (bin >= B) continue;
        double* c3 = ck + (f * B + bin) * 3;
        atomicAdd(&c3[0], w);
        if (wzv != 0.0) atomicAdd(&c3[1], wzv);
        if (wzz != 0.0) atomicAdd(&c3[2], wzz);
      }
    }
  }
  __syncthreads();
  for (int i = threadIdx.x; i < ncell; i += blockDim.x) {
    const double v = cell[i];
    if (v == 0.0) continue;
    const int kk = i / (nf * B * 3), rest = i - kk * (nf * B * 3);
    atomicAdd(&H[((size_t)(k0 + kk) * d + f0) * B * 3 + rest], v);
  }
}

// ------------------------------------------------------------------ BrownBoost sums
// Candidate j = lane: pot_j = sum_i (1 - erf(z / sqrt(c))), cor_j = sum_i exp(-z^2 / c) * u_i,
// z = r_i + s - t_j + a_j * u_i. Wave w of block b takes rows (b * 4 + w), + 4 * gridDim.x, ..
// part [gridDim.x, J, 2].
// what: bit 0 = pot, bit 1 = cor (a sum that is not asked for is returned as 0). A single
// candidate (J = 1) is summed with a row per thread instead and the block's 256 partials are
// added in thread order.
__global__ __launch_bounds__(256) void brown_sums_kernel(const double* __restrict__ r, const double* __restrict__ u,
                                                         long n, const double* __restrict__ scal,
                                                         const double* __restrict__ cand, int J, int what,
                                                         double* __restrict__ part) {
  __shared__ double acc[4][BOOST_MAX_CAND][2];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const double s = scal[0], c = scal[1], isc = 1.0 / sqrt(c), ic = 1.0 / c;
  const bool one = J == 1;
  const bool act = one || lane < J;
  const int cj = one ? 0 : lane;
  const double a = act ? cand[2 * cj] : 0.0, t = act ? cand[2 * cj + 1] : 0.0;
  const long first = one ? (long)blockIdx.x * 256 + threadIdx.x : (long)blockIdx.x * 4 + wave;
  const long step = (long)gridDim.x * (one ? 256 : 4);
  double pot = 0.0, cor = 0.0;
  if (act)
    for (long i = first; i < n; i += step) {
      const double ui = u[i];
      const double z = ((r[i] + s) - t) + a * ui;
      if (what & 1) pot = pot + (1.0 - erf(z * isc));
      if (what & 2) cor = cor + exp((-(z * z)) * ic) * ui;
    }
  acc[wave][lane][0] = pot;
  acc[wave][lane][1] = cor;
  __syncthreads();
  if (one) {
    if (threadIdx.x < 2) {
      double v = 0.0;
      for (int i = 0; i < 256; ++i) v = v + acc[i >> 6][i & 63][threadIdx.x];
      part[(size_t)blockIdx.x * 2 + threadIdx.x] = v;
    }
  } else if (threadIdx.x < 2 * J) {
    const int j = threadIdx.x >> 1, k = threadIdx.x & 1;
    part[((size_t)blockIdx.x * J + j) * 2 + k] = ((acc[0][j][k] + acc[1][j][k]) + acc[2][j][k]) + acc[3][j][k];
  }
}

// out [J, 2] = the partials summed in block order
__global__ __launch_bounds__(128) void brown_reduce_kernel(const double* __restrict__ part, int nblocks, int J,
                                                           double* __restrict__ out) {
  const int i = threadIdx.x;
  if (i >= 2 * J) return;
  double v = 0.0;
  for (int b = 0; b < nblocks; ++b) v = v + part[(size_t)b * J * 2 + i];
  out[i] = v;
}

// srch = (lo, hi, target, done, t). pass < 0: only write the 64 candidates of [lo, hi];
// pass 0 also tests "time runs out" (pot(hi) <= target: done = 1, t = hi); every pass narrows
// [lo, hi] to the first sub-interval whose upper end has pot >= target.
__device__ __forceinline__ double section_point(double lo, double hi, int j) {
  return j >= BOOST_MAX_CAND - 1 ? hi : (j < 0 ? lo : lo + (hi - lo) * ((double)(j + 1) / (double)BOOST_MAX_CAND));
}

__global__ __launch_bounds__(64) void brown_step_kernel(const double* __restrict__ sums, double* __restrict__ srch,
                                                        double a, double* __restrict__ cand, int pass) {
  const int lane = threadIdx.x;
  double lo = srch[0], hi = srch[1];
  const double target = srch[2];
  int done = srch[3] != 0.0 ? 1 : 0;
  if (pass >= 0 && !done) {
    const double pot = sums[2 * lane];
    const double top = __shfl(pot, BOOST_MAX_CAND - 1, 64);
    if (pass == 0 && top <= target) {
      done = 1;
    } else {
      const unsigned long long m = __ballot(pot >= target);
      const int js = m ? (int)__ffsll((long long)m) - 1 : BOOST_MAX_CAND - 1;
      const double nlo = section_point(lo, hi, js - 1), nhi = section_point(lo, hi, js);
      lo = nlo;
      hi = nhi;
    }
  }
  __syncthreads();  // every lane has read srch
  if (lane == 0) {
    srch[0] = lo;
    srch[1] = hi;
    srch[3] = (double)done;
    srch[4] = done ? hi : 0.5 * (lo + hi);
  }
  cand[2 * lane] = a;
  cand[2 * lane + 1] = section_point(lo, hi, lane);
}

inline int shape_status(int B, int C) {
  if (B < 1 || C < 1) return HARP_EBADARG;
  if (B > BOOST_MAX_BINS || C > BOOST_MAX_CLASSES) return HARP_EUNSUPPORTED;
  return HARP_OK;
}

}  // namespace

// H [1, d, B, C] fp64 (zeroed by the caller) += the root histogram of the updated weights;
// w_out [n] (may be null in BrownBoost mode) = the updated weights. Xb [n, dpad] uint8, 16-byte
// aligned rows; y [n] int32. AdaBoost mode: r = scal = null, w_in / rec / mul given.
// BrownBoost mode: r [n], scal = (s, c) given.
HARP_EXPORT int harp_boost_class_round(const uint8_t* Xb, int dpad, long n, const int* y, const double* w_in,
                                       double* w_out, const int* rec, const double* mul, const double* r,
                                       const double* scal, int d, int B, int C, double* H, hipStream_t s) {
  if (n < 0 || d < 1 || dpad < d || (dpad & 15) || ((uintptr_t)Xb & 15) || !y || !H) return HARP_EBADARG;
  if (r ? !scal : (!w_in || !w_out || !rec || !mul || w_in == w_out)) return HARP_EBADARG;
  const int st = shape_status(B, C);
  if (st) return st;
  if (n == 0) return HARP_OK;
  int dg = BOOST_LDS_BYTES / (B * C * 8);
  if (dg < 1) return HARP_EUNSUPPORTED;
  if (dg > d) dg = d;
  const int groups = (d + dg - 1) / dg;
  const long chunks = (n + BOOST_CHUNK - 1) / BOOST_CHUNK;
  if (groups > 65535 || chunks > 0x7fffffffL) return HARP_EUNSUPPORTED;
  class_round_kernel<<<dim3((unsigned)chunks, (unsigned)groups), dim3(256), (size_t)dg * B * C * 8, s>>>(
      Xb, dpad, n, y, w_in, w_out, rec, mul, r, scal, d, B, C, dg, H);
  return harp_launch_status();
}

// w_out = w_in times the previous stump's multiplier (the update pass of the unfused A/B)
HARP_EXPORT int harp_boost_class_update(const uint8_t* Xb, int dpad, long n, const int* y, const double* w_in,
                                        double* w_out, const int* rec, const double* mul, int d, hipStream_t s) {
  if (n < 0 || d < 1 || dpad < d || !y || !w_in || !w_out || !rec || !mul) return HARP_EBADARG;
  if (n == 0) return HARP_OK;
  const long blocks = (n + 255) / 256;
  if (blocks > 0x7fffffffL) return HARP_EUNSUPPORTED;
  class_update_kernel<<<dim3((unsigned)blocks), dim3(256), 0, s>>>(Xb, dpad, n, y, w_in, w_out, rec, mul, d);
  return harp_launch_status();
}

// From harp_forest_split_node's outputs of the root (M = 1): rec [4] int32, mul [2] fp64 and
// info [8 + 2 C] fp64 (see class_finish_kernel). n = rows over all shards.
HARP_EXPORT int harp_boost_class_finish(const int* bf, const int* bb, const int* sp, const double* L, const double* R,
                                        const double* T, int C, double n, int* rec, double* mul, double* info,
                                        hipStream_t s) {
  if (!bf || !bb || !sp || !L || !R || !T || !rec || !mul || !info) return HARP_EBADARG;
  const int st = shape_status(1, C);
  if (st) return st;
  class_finish_kernel<<<dim3(1), dim3(64), 0, s>>>(bf, bb, sp, L, R, T, C, n, rec, mul, info);
  return harp_launch_status();
}

// H [K, d, B, 3] fp64 (zeroed by the caller) += (w, w z, w z^2) of every class; F_out [n, K] =
// F_in + the previous round's centred stumps; wz [n, K, 2] = (w, z) per row and class or null.
HARP_EXPORT int harp_boost_logit_round(const uint8_t* Xb, int dpad, long n, const int* y, const double* F_in,
                                       double* F_out, const int* rec_i, const double* rec_v, double zmax, int d,
                                       int B, int K, double* H, double* wz, hipStream_t s) {
  if (n < 0 || d < 1 || dpad < d || !y || !F_in || !F_out || F_in == F_out || !rec_i || !rec_v || !H)
    return HARP_EBADARG;
  const int st = shape_status(B, K);
  if (st) return st;
  if (n == 0) return HARP_OK;
  int kg = BOOST_LDS_BYTES / (B * 24);
  if (kg < 1) return HARP_EUNSUPPORTED;
  if (kg > K) kg = K;
  const int ncg = (K + kg - 1) / kg;
  int dg = BOOST_LDS_BYTES / (B * kg * 24);
  if (dg < 1) return HARP_EUNSUPPORTED;
  if (dg > d) dg = d;
  const long groups = (long)((d + dg - 1) / dg) * ncg;
  const long chunks = (n + BOOST_CHUNK - 1) / BOOST_CHUNK;
  if (groups > 65535 || chunks > 0x7fffffffL) return HARP_EUNSUPPORTED;
  logit_round_kernel<<<dim3((unsigned)chunks, (unsigned)groups), dim3(256), (size_t)dg * kg * B * 24, s>>>(
      Xb, dpad, n, y, F_in, F_out, rec_i, rec_v, zmax, d, B, K, dg, kg, ncg, H, wz);
  return harp_launch_status();
}

// out [J, 2] = (pot_j, cor_j) of the J <= 64 candidates cand [J, 2] = (a_j, t_j); scal = (s, c);
// what: 1 = pot only, 2 = cor only, 3 = both; part: workspace of harp_boost_brown_blocks(n) *
// J * 2 doubles.
HARP_EXPORT int harp_boost_brown_blocks(long n) {
  long b = (n + 255) / 256;
  if (b > BOOST_SUM_BLOCKS) b = BOOST_SUM_BLOCKS;
  return (int)(b < 1 ? 1 : b);
}

HARP_EXPORT int harp_boost_brown_sums(const double* r, const double* u, long n, const double* scal,
                                      const double* cand, int J, int what, double* part, double* out,
                                      hipStream_t s) {
  if (n < 0 || !scal || !cand || !part || !out || (n > 0 && (!r || !u))) return HARP_EBADARG;
  if (J < 1 || what < 1 || what > 3) return HARP_EBADARG;
  if (J > BOOST_MAX_CAND) return HARP_EUNSUPPORTED;
  const int blocks = harp_boost_brown_blocks(n);
  brown_sums_kernel<<<dim3((unsigned)blocks), dim3(256), 0, s>>>(r, u, n, scal, cand, J, what, part);
  brown_reduce_kernel<<<dim3(1), dim3(128), 0, s>>>(part, blocks, J, out);
  return harp_launch_status();
}

// One step of the 64-way section for t (see brown_step_kernel); sums [64, 2] from
// harp_boost_brown_sums of the current candidates (ignored when pass < 0), cand [64, 2].
HARP_EXPORT int harp_boost_brown_step(const double* sums, double* srch, double a, double* cand, int pass,
                                      hipStream_t s) {
  if (!srch || !cand || (pass >= 0 && !sums)) return HARP_EBADARG;
  brown_step_kernel<<<dim3(1), dim3(64), 0, s>>>(sums, srch, a, cand, pass);
  return harp_launch_status();
}
