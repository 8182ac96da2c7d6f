// Variational LDA (contrib LDA-CVB) E-step, fp64: one document per wave (or per workgroup
// for a long document), gamma / digamma(gamma) / the pass accumulator in registers, the
// rows of the word-major log-beta table re-read through L2 on every pass. Nothing of size
// [nnz, K] is ever stored: the state is gamma [D, K] and the [V, K] statistics.
//
// Per document (LDAMapper.java:284-327): gamma_k = alpha_k + N_d / K, then passes of
//   phi_w = softmax_k(log_beta[k, w] + digamma(gamma_k)),  gamma' = alpha + sum_w n_w phi_w
// until max_k |gamma' - gamma| < tol (tol > 0) or max_passes passes (tol == 0: always
// max_passes), each document on its own count. One more evaluation at the returned gamma
// yields doc_ll = sum_w n_w logsumexp_k(.) and the scatter S_t[w, :] += n_w phi_w.
//
// Lane mapping. Lanes run over topics. 32 < K <= 1024: the wave is one group of 64 lanes with
// NV = ceil(K / 64) (rounded up to a power of two) values per lane, topic k = lane + 64 j.
// K <= 32: the wave is cut into 64 / G groups of G = 2, 4, 8, 16 or 32 lanes (the next power
// of two >= K), every group works on a term of its own and the reductions stay inside a
// group; the groups' accumulators are summed once per pass by xor shuffles G, 2G, .., 32 (a
// fixed order). A document with more than LDAVB_LONG_DOC_TERMS terms gets a workgroup of
// LDAVB_LONG_WAVES waves: the terms are dealt over the waves, every wave writes its pass
// partial to LDS, and after a barrier every wave adds the partials in wave order, so all
// waves carry the same gamma bits and take the same stopping decision. Lanes of one wave
// never hand data to each other through LDS (they exchange by DPP and shuffles), so the
// workgroup barriers are the only LDS ordering needed and no wavefront fences appear.
//
// The S_t scatter is an fp64 global atomic add of K contiguous values per term: sums are
// reproducible to rounding, not bitwise. A word that every document holds makes every
// workgroup add into one row (the slow contended case); stop words are not privatised.
#include "common.h"

#define LDAVB_MAX_TOPICS 1024
#define LDAVB_LONG_DOC_TERMS 256
#define LDAVB_LONG_WAVES 4
#define LDAVB_SHORT_WAVES 4  // independent documents per workgroup of the short kernel

// psi(x), x > 0: the recurrence psi(x) = psi(x + 1) - 1 / x up to x >= 10, then the
// asymptotic series ln x - 1 / (2x) - sum_n B_2n / (2n x^2n) through the B_14 term (the
// first dropped term is below 4.5e-18 at x = 10).
__device__ __forceinline__ double ldavb_digamma(double x) {
  if (!(x > 0.0)) return x == 0.0 ? -__builtin_inf() : __builtin_nan("");
  double r = 0.0;
  while (x < 10.0) {
    r -= 1.0 / x;
    x += 1.0;
  }
  const double xi = 1.0 / x, x2 = xi * xi;
  double s = 1.0 / 12.0;  // B_14 / 14
  s = s * x2 - 691.0 / 32760.0;
  s = s * x2 + 1.0 / 132.0;
  s = s * x2 - 1.0 / 240.0;
  s = s * x2 + 1.0 / 252.0;
  s = s * x2 - 1.0 / 120.0;
  s = s * x2 + 1.0 / 12.0;
  return r + (log(x) - 0.5 * xi - s * x2);
}

__global__ __launch_bounds__(256) void ldavb_digamma_kernel(const double* __restrict__ x, double* __restrict__ out,
                                                            long n) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i < n) out[i] = ldavb_digamma(x[i]);
}

// Sum or maximum over the G lanes of a group (G consecutive lanes, G a power of two), the
// result in every lane of the group. Inside a 16-lane row the exchange is on the DPP network:
// quad_perm [1,0,3,2] and [2,3,0,1], then row_half_mirror and row_mirror (a lane whose quad /
// half already holds that part's result reads the other part's). G = 32 adds one xor-16
// shuffle; G = 64 reads the four row results by readlane, as wave_sum_d_dpp does.
// Needs the whole wave active.
template <bool MAX>
__device__ __forceinline__ double ldavb_op(double a, double b) {
  return MAX ? fmax(a, b) : a + b;
}
template <int G, bool MAX>
__device__ __forceinline__ double group_red(double v) {
  if (G == 64 && !MAX) return wave_sum_d_dpp(v);
  if (G >= 2) v = ldavb_op<MAX>(v, dpp_mov_d<0xB1>(v));
  if (G >= 4) v = ldavb_op<MAX>(v, dpp_mov_d<0x4E>(v));
  if (G >= 8) v = ldavb_op<MAX>(v, dpp_mov_d<0x141>(v));   // row_half_mirror
  if (G >= 16) v = ldavb_op<MAX>(v, dpp_mov_d<0x140>(v));  // row_mirror
  if (G == 32) v = ldavb_op<MAX>(v, __shfl_xor(v, 16, 64));
  if (G == 64)
    v = ldavb_op<MAX>(ldavb_op<MAX>(readlane_d(v, 0), readlane_d(v, 16)),
                      ldavb_op<MAX>(readlane_d(v, 32), readlane_d(v, 48)));
  return v;
}

// One sweep over the document's terms at the current gamma. FINAL = false: acc[j] = this
// wave's sum_w n_w phi_wk (already summed over the wave's groups). FINAL = true: the S_t
// scatter, and the return value is this wave's share of doc_ll (in every lane).
template <int G, int NV, int W, bool FINAL>
__device__ __forceinline__ double ldavb_sweep(const int* __restrict__ word, const double* __restrict__ cnt,
                                              const double* __restrict__ lbt, double* __restrict__ S_t, long a,
                                              int len, int K, int wv, int g, int kl, const double (&gam)[NV],
                                              double (&acc)[NV]) {
  constexpr int NG = 64 / G;
  const double ninf = -__builtin_inf();
  double dg[NV];
#pragma unroll
  for (int j = 0; j < NV; ++j) {
    dg[j] = (kl + 64 * j < K) ? ldavb_digamma(gam[j]) : ninf;
    acc[j] = 0.0;
  }
  double ll = 0.0;
  const int off = wv * NG + g;
  constexpr int STEP = W * NG;
  // The chain term index -> word -> log-beta row is two dependent memory round trips per
  // term: the word and count of the next term are loaded while the current term is worked
  // on. A term index past the end is clamped to the last term (count 0), so every address
  // read ahead is inside the document.
  auto term = [&](int i, int& w, double& c, bool& valid) {
    const int t = i + off;
    valid = t < len;
    const long tt = a + (valid ? t : len - 1);
    w = word[tt];
    c = valid ? cnt[tt] : 0.0;
  };
  int w1;
  double c1;
  bool valid1;
  term(0, w1, c1, valid1);
  for (int i = 0; i < len; i += STEP) {  // the same trip count in every lane and wave
    const int w = w1;
    const double c = c1;
    const bool valid = valid1;
    term(i + STEP, w1, c1, valid1);
    const double* __restrict__ row = lbt + (long)w * K;
    double x[NV];
#pragma unroll
    for (int j = 0; j < NV; ++j) x[j] = (kl + 64 * j < K) ? row[kl + 64 * j] : ninf;
    double m = ninf;
#pragma unroll
    for (int j = 0; j < NV; ++j) {
      x[j] += dg[j];  // -inf stays -inf (dg is finite for k < K, -inf beyond)
      m = fmax(m, x[j]);
    }
    m = group_red<G, true>(m);
    double s = 0.0;
#pragma unroll
    for (int j = 0; j < NV; ++j) {
      x[j] = exp(x[j] - m);  // exactly 0 for a -inf entry
      s += x[j];
    }
    s = group_red<G, false>(s);
    const double r = c / s;
    if (FINAL) {
      ll += c * (m + log(s));
      if (valid) {
#pragma unroll
        for (int j = 0; j < NV; ++j) {
          const int k = kl + 64 * j;
          if (k < K) atomicAdd(&S_t[(long)w * K + k], x[j] * r);
        }
      }
    } else {
#pragma unroll
      for (int j = 0; j < NV; ++j) acc[j] += x[j] * r;
    }
  }
  if (FINAL) {
    ll = (kl == 0) ? ll : 0.0;  // every lane of a group holds the group's value
    return wave_sum_d_dpp(ll);
  }
#pragma unroll
  for (int j = 0; j < NV; ++j)
    for (int o = G; o < 64; o <<= 1) acc[j] += __shfl_xor(acc[j], o, 64);
  return 0.0;
}

// W == 1: LDAVB_SHORT_WAVES independent documents per workgroup, one per wave, no LDS.
// W  > 1: one document per workgroup of W waves; s_part holds W x (NV * G) pass partials.
template <int G, int NV, int W>
__global__ __launch_bounds__(64 * (W > 1 ? W : LDAVB_SHORT_WAVES)) void ldavb_estep_kernel(
    const long* __restrict__ rowptr, const int* __restrict__ word, const double* __restrict__ cnt,
    const double* __restrict__ lbt, const double* __restrict__ alpha, const int* __restrict__ sched, long first,
    long n, int K, int max_passes, double tol, double* __restrict__ gamma_out, int* __restrict__ passes_out,
    double* __restrict__ ll_out, double* __restrict__ S_t) {
  constexpr int KP = NV * G;
  extern __shared__ double s_part[];
  const int lane = threadIdx.x & 63;
  const int wid = threadIdx.x >> 6;
  const int g = lane / G, kl = lane % G;
  const long slot = (W > 1) ? (long)blockIdx.x : (long)blockIdx.x * LDAVB_SHORT_WAVES + wid;
  if (slot >= n) return;  // wave-uniform (W > 1: workgroup-uniform)
  const int wv = (W > 1) ? wid : 0;
  const int d = __builtin_amdgcn_readfirstlane(sched[first + slot]);
  const long a = rowptr[d];
  const int len = (int)(rowptr[d + 1] - a);

  double al[NV], gam[NV], acc[NV];
#pragma unroll
  for (int j = 0; j < NV; ++j) al[j] = (kl + 64 * j < K) ? alpha[kl + 64 * j] : 1.0;
  if (len == 0) {  // no terms: gamma = alpha, one pass, doc_ll = 0 (never a long document)
    if (g == 0) {
#pragma unroll
      for (int j = 0; j < NV; ++j)
        if (kl + 64 * j < K) gamma_out[(long)d * K + kl + 64 * j] = al[j];
    }
    if (lane == 0) {
      passes_out[d] = 1;
      ll_out[d] = 0.0;
    }
    return;
  }
  double nd = 0.0;
  for (int t = lane; t < len; t += 64) nd += cnt[a + t];
  nd = wave_sum_d_dpp(nd);
#pragma unroll
  for (int j = 0; j < NV; ++j) gam[j] = (kl + 64 * j < K) ? al[j] + nd / K : 1.0;

  int p = 0;
  for (;;) {
    ldavb_sweep<G, NV, W, false>(word, cnt, lbt, S_t, a, len, K, wv, g, kl, gam, acc);
    if (W > 1) {
      if (g == 0) {
#pragma unroll
        for (int j = 0; j < NV; ++j) s_part[wv * KP + kl + G * j] = acc[j];
      }
      __syncthreads();
#pragma unroll
      for (int j = 0; j < NV; ++j) {
        double s = s_part[kl + G * j];
        for (int u = 1; u < W; ++u) s += s_part[u * KP + kl + G * j];
        acc[j] = s;
      }
      __syncthreads();  // the partials are overwritten by the next pass
    }
    double delta = 0.0;
#pragma unroll
    for (int j = 0; j < NV; ++j) {
      const double nw = al[j] + acc[j];
      if (kl + 64 * j < K) {
        delta = fmax(delta, fabs(nw - gam[j]));
        gam[j] = nw;
      }
    }
    delta = group_red<G, true>(delta);  // every group holds all K values: the same in all lanes
    ++p;
    if (p >= max_passes || (tol > 0.0 && delta < tol)) break;
  }

  double ll = ldavb_sweep<G, NV, W, true>(word, cnt, lbt, S_t, a, len, K, wv, g, kl, gam, acc);
  if (W > 1) {
    if (lane == 0) s_part[wv] = ll;
    __syncthreads();
    ll = s_part[0];
    for (int u = 1; u < W; ++u) ll += s_part[u];
  }
  if (wv == 0) {
    if (g == 0) {
#pragma unroll
      for (int j = 0; j < NV; ++j)
        if (kl + 64 * j < K) gamma_out[(long)d * K + kl + 64 * j] = gam[j];
    }
    if (lane == 0) {
      passes_out[d] = p;
      ll_out[d] = ll;
    }
  }
}

template <int G, int NV>
static void ldavb_launch(const long* rowptr, const int* word, const double* cnt, const double* lbt,
                         const double* alpha, const int* sched, long n_docs, long n_long, int K, int max_passes,
                         double tol, double* gamma, int* passes, double* doc_ll, double* S_t, hipStream_t stream) {
  constexpr int W = LDAVB_LONG_WAVES;
  if (n_long > 0)
    hipLaunchKernelGGL((ldavb_estep_kernel<G, NV, W>), dim3((unsigned)n_long), dim3(64 * W),
                       sizeof(double) * W * NV * G, stream, rowptr, word, cnt, lbt, alpha, sched, 0L, n_long, K,
                       max_passes, tol, gamma, passes, doc_ll, S_t);
  const long n_short = n_docs - n_long;
  if (n_short > 0)
    hipLaunchKernelGGL((ldavb_estep_kernel<G, NV, 1>),
                       dim3((unsigned)((n_short + LDAVB_SHORT_WAVES - 1) / LDAVB_SHORT_WAVES)),
                       dim3(64 * LDAVB_SHORT_WAVES), 0, stream, rowptr, word, cnt, lbt, alpha, sched, n_long, n_short,
                       K, max_passes, tol, gamma, passes, doc_ll, S_t);
}

HARP_EXPORT int harp_ldavb_max_topics() { return LDAVB_MAX_TOPICS; }
HARP_EXPORT int harp_ldavb_long_doc_terms() { return LDAVB_LONG_DOC_TERMS; }

HARP_EXPORT int harp_ldavb_digamma(const void* x, void* out, long n, hipStream_t stream) {
  if (n < 0 || (n > 0 && (!x || !out))) return HARP_EBADARG;
  if (n == 0) return HARP_OK;
  hipLaunchKernelGGL(ldavb_digamma_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream,
                     (const double*)x, (double*)out, n);
  return harp_launch_status();
}

// sched: the documents longest-first; its first n_long entries are the documents with more
// than LDAVB_LONG_DOC_TERMS terms. S_t is added to (the caller zeroes it).
HARP_EXPORT int harp_ldavb_estep(const void* rowptr, const void* word, const void* cnt, const void* log_beta_t,
                                 const void* alpha, const void* sched, long n_docs, long n_long, int K,
                                 int max_passes, double tol, void* gamma, void* passes, void* doc_ll, void* S_t,
                                 hipStream_t stream) {
  if (K > LDAVB_MAX_TOPICS) return HARP_EUNSUPPORTED;
  if (K < 1 || n_docs < 0 || n_long < 0 || n_long > n_docs || max_passes < 1 || !(tol >= 0.0)) return HARP_EBADARG;
  if (n_docs == 0) return HARP_OK;
  if (!rowptr || !alpha || !sched || !gamma || !passes || !doc_ll) return HARP_EBADARG;
  if ((n_docs + LDAVB_SHORT_WAVES - 1) / LDAVB_SHORT_WAVES > 0x7fffffffL) return HARP_EUNSUPPORTED;
#define LDAVB_GO(G, NV)                                                                                        \
  ldavb_launch<G, NV>((const long*)rowptr, (const int*)word, (const double*)cnt, (const double*)log_beta_t,     \
                      (const double*)alpha, (const int*)sched, n_docs, n_long, K, max_passes, tol,             \
                      (double*)gamma, (int*)passes, (double*)doc_ll, (double*)S_t, stream)
  if (K <= 2) LDAVB_GO(2, 1);
  else if (K <= 4) LDAVB_GO(4, 1);
  else if (K <= 8) LDAVB_GO(8, 1);
  else if (K <= 16) LDAVB_GO(16, 1);
  else if (K <= 32) LDAVB_GO(32, 1);
  else if (K <= 64) LDAVB_GO(64, 1);
  else if (K <= 128) LDAVB_GO(64, 2);
  else if (K <= 256) LDAVB_GO(64, 4);
  else if (K <= 512) LDAVB_GO(64, 8);
  else LDAVB_GO(64, 16);
#undef LDAVB_GO
  return harp_launch_status();
}
