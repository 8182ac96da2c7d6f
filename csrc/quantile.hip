// Exact order statistics by most-significant-digit radix select for gfx950 (MI355X / CDNA4).
//
// Replaces the hot loop of the reference's DAAL quantile batch launcher (ml/daal daal_quantile,
// QTEDaalCollectiveMapper), which sorts every column. Here nothing is sorted and nothing is
// copied: every wanted order statistic of every column is found digit by digit, eight bits at a
// time from the top, and each digit costs one histogram pass over the block. The pass count is
// fixed by the dtype (bf16 2, fp32 4, fp64 8). harp_amd/ops/quantile.py drives the passes, sums
// the histograms over the workers between hist and pick, and holds the CPU torch mirror of both
// kernels (the oracle of tests/test_quantile_gpu.py).
//
// Keys. A value's bits map to an unsigned key of the same width whose integer order is the
// value's order: key = bits ^ (sign ? all-ones : sign-bit), with -0.0 first turned into +0.0
// (a sort treats them as equal). A NaN gets no key; pass 0 counts the NaNs of every column.
//
// hist. A target is one wanted order statistic. prefix[d, T] holds, per (column, target), the
// top 8p key bits found by the p picks so far. One workgroup owns a tile of QUANTILE_CHUNK rows
// by C columns (C: 64 bytes of a bf16 row, 64 of an fp32 row, 128 of an fp64 row) and up to
// 128 / C targets (grid.z covers the rest), and keeps one 256-bin uint32 histogram per (column,
// target) in LDS: 128 histograms, 128.5 KiB. Lane l of a wave reads column l % C of row l / C
// of the wave's 64 / C rows, so a wave-instruction reads whole 64-byte (or longer) row segments.
// A histogram is 257 dwords apart from the next, which puts equal digits of neighbouring columns
// on different banks. A row whose key's top 8p bits equal the prefix adds 1 at its next digit.
// Pass 0 has no prefix and one histogram per column. The tile is flushed once, nonzero bins
// only, with 64-bit global atomic adds. All counts are integers: the result does not depend on
// any order and is bitwise repeatable.
//
// Shared digits. Real data puts most keys of pass 0 in a few exponent bins and a constant or
// categorical column puts every row in one bin in every pass, so lanes of a wave often add to
// one address. Per wave-instruction and target: one ballot of the matching lanes (no lane
// matches, the common case of the later passes: nothing is issued), the digit of the first
// matching lane, one more ballot; when every matching lane has that digit, the lane of each
// column in the wave's first row adds the column's popcount, C adds to C banks instead of 64
// adds that collide 64 / C deep. Measured (profiles/quantile), the path loses: the plain adds of
// a constant block cost nothing over those of a block where no row matches, and the two ballots
// and the lane read per target make a pass up to twice as long. It is therefore off unless flags
// bit 0 asks for it (scripts/bench_quantile.py measures both).
//
// pick. One thread per (column, target) walks the summed 256 bins: the digit is the first bin
// whose inclusive running count exceeds the rank left inside the current bucket (255 if none
// does, which only an out-of-range rank or a NaN column can cause); it is appended to the
// prefix and the counts below it leave the rank. The last pick writes the value by the inverse
// key map into out[T, d] (NaN where the column has one, torch.quantile's rule).
//
// No kernel waits on another workgroup; all stores are vector stores.
#include "common.h"

#define QUANTILE_RADIX_BITS 8
#define QUANTILE_BINS 256
#define QUANTILE_CHUNK 4096
#define QUANTILE_MAX_TARGETS 8
#define QUANTILE_THREADS 1024
#define QUANTILE_LDS_HISTS 128  // (column, target) histograms of one workgroup
#define QUANTILE_HIST_STRIDE 257  // dwords from one LDS histogram to the next

namespace {

// L: the type a value is loaded as; K: the type its key is computed in; W: key bits; E: exponent
// bits; C: columns of a tile; U: loads a lane issues before it uses the first (32 bytes per lane
// in flight for fp32 and fp64, as much for bf16 as 64 VGPRs allow, so that pass 0 keeps two
// workgroups per CU; 8 against 4 loads gained 5 % at fp32)
struct KeyBf16 {
  typedef uint16_t L;
  typedef uint32_t K;
  static constexpr int W = 16, E = 8, C = 32, U = 12;
};
struct KeyFp32 {
  typedef uint32_t L;
  typedef uint32_t K;
  static constexpr int W = 32, E = 8, C = 16, U = 8;
};
struct KeyFp64 {
  typedef uint64_t L;
  typedef uint64_t K;
  static constexpr int W = 64, E = 11, C = 16, U = 4;
};

// false for a NaN; else the order-preserving key
template <typename F>
__device__ __forceinline__ bool float_key(typename F::K bits, typename F::K& key) {
  typedef typename F::K K;
  constexpr K SIGN = (K)1 << (F::W - 1);
  constexpr K INF = (((K)1 << F::E) - 1) << (F::W - 1 - F::E);
  const K mag = bits & (SIGN - 1);
  if (mag > INF) return false;
  if (mag == 0) bits = 0;
  key = (bits & SIGN) ? (~bits & (SIGN | (SIGN - 1))) : (bits | SIGN);
  return true;
}

// h: this lane's histogram. The call sits in wave-uniform control flow (the ballots need it).
template <int C, bool SHARE>
__device__ __forceinline__ void hist_add(uint32_t* h, int lane, int digit, bool m) {
  if constexpr (SHARE) {
    const unsigned long long bal = __ballot(m);
    if (bal == 0) return;  // wave-uniform
    const int first = __builtin_amdgcn_readlane(digit, __ffsll(bal) - 1);
    if (__ballot(m && digit != first) == 0) {
      // lanes c, c + C, c + 2C, .. hold column c: the first of them adds for all
      constexpr unsigned long long COLS = C == 16 ? 0x0001000100010001ull : 0x0000000100000001ull;
      const unsigned cnt = (unsigned)__popcll(bal & (COLS << (lane & (C - 1))));
      if (lane < C && cnt) atomicAdd(&h[first], cnt);
      return;
    }
  }
  if (m) atomicAdd(&h[digit], 1u);
}

template <typename F, bool SHARE>
__global__ __launch_bounds__(QUANTILE_THREADS) void hist_kernel(const typename F::L* __restrict__ X, long n, long ldx,
                                                                int d, int groups, int p, int T,
                                                                const unsigned long long* __restrict__ prefix,
                                                                unsigned long long* __restrict__ hist,
                                                                unsigned long long* __restrict__ nan_count) {
  typedef typename F::K K;
  constexpr int C = F::C, W = F::W;
  constexpr int TG = QUANTILE_LDS_HISTS / C;  // targets of one workgroup
  constexpr int RPB = QUANTILE_THREADS / C;   // rows of one step of the workgroup
  extern __shared__ uint32_t quantile_smem[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int lc = tid % C, lr = tid / C;
  // Consecutive workgroups go to the eight XCDs in turn. Workgroups 8 apart share an XCD, so the
  // column groups of one chunk are 8 apart: the cache lines two of them share (a row is rarely a
  // whole number of lines) are fetched into one L2, not two. Eight chunks interleave.
  const long per = 8L * groups;
  const long oct = (long)blockIdx.x / per;
  const int rem = (int)((long)blockIdx.x - oct * per);
  const long chunk = oct * 8 + (rem & 7);
  const int c0 = (rem >> 3) * C;
  const long r0 = chunk * QUANTILE_CHUNK;
  if (r0 >= n) return;  // block-uniform: the last eight chunks are padded
  const int nc = min(C, d - c0);
  const int rows = (int)min((long)QUANTILE_CHUNK, n - r0);
  const int t0 = p == 0 ? 0 : (int)blockIdx.z * TG;
  const int nt = p == 0 ? 1 : min(TG, T - t0);
  const int ht = p == 0 ? 1 : T;  // histograms per column in `hist`
  uint32_t* nan_lds = quantile_smem + nt * C * QUANTILE_HIST_STRIDE;
  for (int i = tid; i < nt * C * QUANTILE_HIST_STRIDE + C; i += QUANTILE_THREADS) quantile_smem[i] = 0;
  __syncthreads();

  const bool colok = lc < nc;
  K pre[TG];
#pragma unroll
  for (int t = 0; t < TG; ++t) pre[t] = (p > 0 && colok && t < nt) ? (K)prefix[(long)(c0 + lc) * T + t0 + t] : (K)0;
  const int lo = W - QUANTILE_RADIX_BITS * (p + 1);  // shift of this pass's digit
  const int hi = p == 0 ? 0 : W - QUANTILE_RADIX_BITS * p;  // shift that leaves the prefix bits
  const typename F::L* xp = X + r0 * ldx + c0 + lc;
  uint32_t* hl = quantile_smem + lc * QUANTILE_HIST_STRIDE;  // target t: + t * C histograms
  unsigned nans = 0;
  const int steps = (rows + RPB - 1) / RPB;
  for (int it = 0; it < steps; it += F::U) {
    K v[F::U];
    bool ok[F::U];
#pragma unroll
    for (int u = 0; u < F::U; ++u) {
      const int r = (it + u) * RPB + lr;
      ok[u] = colok && r < rows;
      v[u] = ok[u] ? (K)xp[(long)r * ldx] : (K)0;
    }
#pragma unroll
    for (int u = 0; u < F::U; ++u) {
      K key = 0;
      const bool valid = float_key<F>(v[u], key) && ok[u];
      nans += (ok[u] && !valid) ? 1u : 0u;
      const int digit = (int)((key >> lo) & (QUANTILE_BINS - 1));
      if (p == 0) {
        hist_add<C, SHARE>(hl, lane, digit, valid);
      } else {
        const K top = key >> hi;
#pragma unroll
        for (int t = 0; t < TG; ++t)
          if (t < nt)  // block-uniform
            hist_add<C, SHARE>(hl + t * C * QUANTILE_HIST_STRIDE, lane, digit, valid && top == pre[t]);
      }
    }
  }
  if (p == 0 && nans) atomicAdd(&nan_lds[lc], nans);
  __syncthreads();

  for (int i = tid; i < nt * nc * QUANTILE_BINS; i += QUANTILE_THREADS) {
    const int b = i & (QUANTILE_BINS - 1), j = i >> QUANTILE_RADIX_BITS;
    const int t = j / nc, c = j - t * nc;
    const uint32_t v = quantile_smem[(t * C + c) * QUANTILE_HIST_STRIDE + b];
    if (v) atomicAdd(&hist[((long)(c0 + c) * ht + t0 + t) * QUANTILE_BINS + b], (unsigned long long)v);
  }
  if (p == 0 && tid < nc && nan_lds[tid]) atomicAdd(&nan_count[c0 + tid], (unsigned long long)nan_lds[tid]);
}

template <typename F>
__global__ __launch_bounds__(64) void pick_kernel(const long long* __restrict__ hist, int ht,
                                                  unsigned long long* __restrict__ prefix,
                                                  long long* __restrict__ remaining, int d, int T, int last,
                                                  const long long* __restrict__ nan_count,
                                                  typename F::L* __restrict__ out) {
  typedef typename F::K K;
  const long i = (long)blockIdx.x * 64 + threadIdx.x;
  if (i >= (long)d * T) return;
  const int c = (int)(i / T), t = (int)(i - (long)c * T);
  const long long* h = hist + ((long)c * ht + (ht == 1 ? 0 : t)) * QUANTILE_BINS;
  const long long rank = remaining[i];
  long long cum = 0, below = 0;
  int digit = 0;
#pragma unroll 8
  for (int b = 0; b < QUANTILE_BINS - 1; ++b) {
    cum += h[b];
    if (cum <= rank) {  // the running count only grows: true for a leading run of bins
      digit = b + 1;
      below = cum;
    }
  }
  const unsigned long long key = (prefix[i] << QUANTILE_RADIX_BITS) | (unsigned long long)digit;
  prefix[i] = key;
  remaining[i] = rank - below;
  if (!last) return;
  constexpr K SIGN = (K)1 << (F::W - 1);
  constexpr K ALL = SIGN | (SIGN - 1);
  const K k = (K)key & ALL;
  K bits = (k & SIGN) ? (k ^ SIGN) : (~k & ALL);
  if (nan_count && nan_count[c] > 0) bits = ((((K)1 << (F::E + 1)) - 1) << (F::W - 2 - F::E));  // quiet NaN
  out[(long)t * d + c] = (typename F::L)bits;
}

template <typename F>
int launch_hist(const void* X, long n, long ldx, int d, int p, const void* prefix, int T, void* hist, void* nan_count,
                int flags, hipStream_t s) {
  constexpr int TG = QUANTILE_LDS_HISTS / F::C;
  if (p >= F::W / QUANTILE_RADIX_BITS) return HARP_EBADARG;
  const int groups = (d + F::C - 1) / F::C;
  const long chunks = (n + QUANTILE_CHUNK - 1) / QUANTILE_CHUNK;
  const long padded = (chunks + 7) / 8 * 8;  // the kernel's block order works in eights of chunks
  if (padded * groups > 0x7fffffffL) return HARP_EUNSUPPORTED;
  const int nt = p == 0 ? 1 : (T < TG ? T : TG);
  const dim3 g((unsigned)(padded * groups), 1, p == 0 ? 1u : (unsigned)((T + TG - 1) / TG)), b(QUANTILE_THREADS);
  const size_t lds = sizeof(uint32_t) * ((size_t)nt * F::C * QUANTILE_HIST_STRIDE + F::C);
  auto* k = (flags & 1) ? hist_kernel<F, true> : hist_kernel<F, false>;
  if (lds > 32 * 1024 &&
      hipFuncSetAttribute((const void*)k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess)
    return HARP_ELAUNCH;
  k<<<g, b, lds, s>>>((const typename F::L*)X, n, ldx, d, groups, p, T, (const unsigned long long*)prefix,
                      (unsigned long long*)hist, (unsigned long long*)nan_count);
  return harp_launch_status();
}

template <typename F>
int launch_pick(const void* hist, int ht, void* prefix, void* remaining, int d, int T, int last, const void* nan_count,
                void* out, hipStream_t s) {
  const long total = (long)d * T;
  pick_kernel<F><<<dim3((unsigned)((total + 63) / 64)), dim3(64), 0, s>>>(
      (const long long*)hist, ht, (unsigned long long*)prefix, (long long*)remaining, d, T, last,
      (const long long*)nan_count, (typename F::L*)out);
  return harp_launch_status();
}

}  // namespace

// The constants the Python side mirrors (ops/quantile.py checks them when the library loads):
// 0 radix bits, 1 rows of a tile, 2 targets of one sweep, 3 / 4 / 5 columns of a bf16 / fp32 /
// fp64 tile. -1 for any other index.
HARP_EXPORT int harp_quantile_param(int which) {
  switch (which) {
    case 0: return QUANTILE_RADIX_BITS;
    case 1: return QUANTILE_CHUNK;
    case 2: return QUANTILE_MAX_TARGETS;
    case 3: return KeyBf16::C;
    case 4: return KeyFp32::C;
    case 5: return KeyFp64::C;
    default: return -1;
  }
}

// One radix pass. X [n, d] row-major with row stride ldx >= d elements, dtype 0 bf16 / 1 fp32 /
// 2 fp64; prefix [d, T] int64 (read when p > 0). hist (int64, zeroed by the caller) is [d, 256]
// for p == 0 and [d, T, 256] after; nan_count [d] (int64, zeroed by the caller) is written by
// pass 0 only. flags bit 0: take the shared-digit path.
HARP_EXPORT int harp_quantile_hist(const void* X, int dtype, long n, long ldx, int d, int p, const void* prefix, int T,
                                   void* hist, void* nan_count, int flags, hipStream_t s) {
  if (n < 0 || d < 1 || ldx < d || p < 0 || T < 1 || !hist) return HARP_EBADARG;
  if ((p == 0 && !nan_count) || (p > 0 && !prefix) || (n > 0 && !X)) return HARP_EBADARG;
  if (dtype < 0 || dtype > 2 || T > QUANTILE_MAX_TARGETS) return HARP_EUNSUPPORTED;
  if (n == 0) return HARP_OK;
  if (dtype == 0) return launch_hist<KeyBf16>(X, n, ldx, d, p, prefix, T, hist, nan_count, flags, s);
  if (dtype == 1) return launch_hist<KeyFp32>(X, n, ldx, d, p, prefix, T, hist, nan_count, flags, s);
  return launch_hist<KeyFp64>(X, n, ldx, d, p, prefix, T, hist, nan_count, flags, s);
}

// One digit of every (column, target) from the summed hist ([d, ht, 256], ht = 1 or T), in place
// on prefix [d, T] and remaining [d, T] (int64). last != 0 (the pick of the dtype's last pass): the
// prefix is now the whole key and its value goes to out [T, d] in that dtype (dtype as for
// harp_quantile_hist); nan_count [d] or null.
HARP_EXPORT int harp_quantile_pick(const void* hist, int ht, void* prefix, void* remaining, int d, int T, int last,
                                   int dtype, const void* nan_count, void* out, hipStream_t s) {
  if (!hist || !prefix || !remaining || d < 1 || T < 1 || (ht != 1 && ht != T)) return HARP_EBADARG;
  if (last && !out) return HARP_EBADARG;
  if (dtype < 0 || dtype > 2) return HARP_EUNSUPPORTED;
  if (dtype == 0) return launch_pick<KeyBf16>(hist, ht, prefix, remaining, d, T, last, nan_count, out, s);
  if (dtype == 1) return launch_pick<KeyFp32>(hist, ht, prefix, remaining, d, T, last, nan_count, out, s);
  return launch_pick<KeyFp64>(hist, ht, prefix, remaining, d, T, last, nan_count, out, s);
}
