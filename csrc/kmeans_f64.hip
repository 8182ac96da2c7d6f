// Dense K-means step in fp64 for gfx950 (MI355X / CDNA4): exact labels on the fp64 matrix
// cores, then sums, counts and the objective in one pass over the label-sorted rows. Nothing
// of size n x K is ever built and X (bf16 / fp32 / fp64) is read in place through its row
// stride and widened in registers.
//
// Reference: ml/daal daal_kmeans/regroupallgather (DAAL kmeans DistributedStep1Local on a
// dense table, Double throughout). harp_amd/ops/kmeans_f64.py drives the kernels.
//
// prepare_kernel. The sweep operand of the fp64 centroids C [K, d]. The width is padded to
// dpad = 4 S (S from kmf_steps: the MFMA steps of one row), K to whole stages of TILES tiles of
// 16 centroids. A tile is S * 64 + 16 doubles: first W[s][lane] = -2 C[16 t + (lane & 15)]
// [(lane >> 4) S + s] (exact; zero in padding rows and columns), the value lane `lane` feeds to
// MFMA step s, then cn[r] = ||c_{16 t + r}||^2 (+inf for a padding row, so it can never win).
// A stage is therefore one contiguous run of global memory whose copy to LDS is linear, and a
// lane's operand read is one ds_read_b64 at stride 64 doubles.
//
// assign_kernel. labels[i] = argmin_k (cn[k] - 2 x_i . c_k), ties to the lowest k.
//  * v_mfma_f64_16x16x4_f64 in the lane layout csrc/outlier.hip documents: centroids are operand
//    A (rows), points operand B (columns), so register r of lane l holds centroid (l >> 4) + 4 r
//    of the tile for point l & 15. The k index of a step is a free permutation as long as both
//    operands agree: lane group g = l >> 4 takes the contiguous columns [g S, (g + 1) S) of its
//    row, one vectorised run of the point's row per lane.
//  * A workgroup of four waves owns 128 points (two 16-point tiles per wave, S <= 32) or 64
//    (one tile, S > 32); the points stay in registers (S doubles per tile and lane) for the
//    whole sweep over K. A resident grid takes point blocks b, b + grid, ...
//  * Centroid stages stream through two LDS buffers shared by the four waves; the global loads
//    of stage st + 1 are issued before the MFMAs of stage st and land in LDS after them, one
//    barrier per stage. When all of K is one stage it is filled once per workgroup.
//  * Two centroid tiles are swept together. With two point tiles that is four independent
//    accumulator chains; with one, every chain is split into even and odd steps (four again),
//    added once at the end. Accumulators start at cn, so a chain ends holding the distance
//    term and the epilogue is four compare / selects per chain: strict <, ascending centroid
//    order, nothing crosses lanes. At the end of the sweep the four lane groups of a point
//    merge on (distance, index) with the project's tie rule.
//  * A NaN distance fails every compare, so a row of NaNs keeps label 0. Stores are plain and
//    every sum has one fixed order: labels are bitwise repeatable.
//
// sums_kernel, in the style of segsum.hip's row sum. Over the permutation that sorts the rows
// by label, every 16-lane slot takes a fixed run of KMF_RUN entries (balanced whatever the
// cluster sizes), lane l the columns l, l + 16, ... It gathers the rows in their own dtype and
// keeps the row sum and sum (x - c_k)^2 in fp64 registers, c_k held by the slot and reloaded at
// a bucket boundary: the objective has no ||x||^2 + ||c||^2 - 2 x.c cancellation. Partials
// flush at bucket boundaries with global_atomic_add_f64 (as kmeans_csr.hip does; wss after a
// sum over the slot's lanes), so sums and wss are exact only up to the order of those adds;
// counts come from the bucket offsets.
#include "common.h"

#define KMF_THREADS 256
#define KMF_MAX_D 256
#define KMF_MAX_K 16384  // the counting sort's limit
#define KMF_RUN 128      // sorted rows per slot of the sums pass

namespace {

typedef double doublex4 __attribute__((ext_vector_type(4)));
typedef double doublex2 __attribute__((ext_vector_type(2)));

struct InBf16 {
  typedef uint16_t L;
  typedef uint16_t V __attribute__((ext_vector_type(8)));
  static __device__ __forceinline__ double wide(L v) { return (double)__uint_as_float((uint32_t)v << 16); }
};
struct InFp32 {
  typedef float L;
  typedef float V __attribute__((ext_vector_type(4)));
  static __device__ __forceinline__ double wide(L v) { return (double)v; }
};
struct InFp64 {
  typedef double L;
  typedef double V __attribute__((ext_vector_type(2)));
  static __device__ __forceinline__ double wide(L v) { return v; }
};

// MFMA steps per row: the instantiated widths dpad = 4 S
constexpr int kmf_steps(int d) {
  constexpr int list[] = {1, 2, 4, 8, 16, 24, 28, 32, 48, 64};
  for (int s : list)
    if (4 * s >= d) return s;
  return 0;
}

template <int S>
struct Shape {
  static constexpr int PT = S <= 32 ? 2 : 1;   // point tiles of a wave
  static constexpr int KH = PT == 1 ? 2 : 1;   // chains per (point tile, centroid tile)
  static constexpr int PPB = 4 * PT * 16;      // points of a workgroup
  static constexpr int TILES = (64 / S < 2 ? 2 : 64 / S > 16 ? 16 : 64 / S) & ~1;  // per stage
  static constexpr int TD = S * 64 + 16;       // doubles of a tile: operand, then cn
  static constexpr int STAGE = TILES * TD;     // doubles of a stage
  static constexpr int CHUNKS = STAGE / 2;     // its 16-byte pieces
  static constexpr int NLD = (CHUNKS + KMF_THREADS - 1) / KMF_THREADS;
  static constexpr int WG_PER_CU = S <= 16 ? 2 : 1;  // what the registers of the instantiation allow
  static_assert(2 * STAGE * sizeof(double) <= 160 * 1024, "both buffers fit the LDS");
  static_assert(S % KH == 0 && TILES % 2 == 0, "chains and tile pairs come out even");
};

// ---- the operand -----------------------------------------------------------------------------
template <int S>
__global__ __launch_bounds__(256) void prepare_kernel(const double* __restrict__ C, long ldc, int K, int d,
                                                      double* __restrict__ W, long total) {
  constexpr int TD = Shape<S>::TD;
  const long e = (long)blockIdx.x * 256 + threadIdx.x;
  if (e >= total) return;
  const long t = e / TD;
  const int o = (int)(e - t * TD);
  double v;
  if (o < S * 64) {
    const int s = o >> 6, l = o & 63;
    const long row = t * 16 + (l & 15);
    const int col = (l >> 4) * S + s;
    v = row < K && col < d ? -2.0 * C[row * ldc + col] : 0.0;
  } else {
    const long row = t * 16 + (o - S * 64);
    v = __builtin_inf();
    if (row < K) {
      v = 0.0;
      for (int j = 0; j < d; ++j) v = fma(C[row * ldc + j], C[row * ldc + j], v);
    }
  }
  W[e] = v;
}

// ---- assign ----------------------------------------------------------------------------------
// The S columns from col0 of one row, widened; zero past d and for a row past n.
template <typename F, int S>
__device__ __forceinline__ void load_point(double (&x)[S], const typename F::L* __restrict__ row, bool valid,
                                           int col0, int d, int vec) {
  typedef typename F::V V;
  constexpr int VW = 16 / sizeof(typename F::L);
  // No branch per load: an address out of range is replaced by one inside the row and the value
  // dropped. S % VW == 0 implies d > VW (kmf_steps), so the vector at column 0 is inside the row.
  if constexpr (S % VW == 0) {
    if (vec) {
      // the one vector of the row that straddles d, element by element
      const int cs = d / VW * VW;
      double tail[VW];
#pragma unroll
      for (int e = 0; e < VW; ++e) {
        const double t = F::wide(row[cs + e < d ? cs + e : 0]);
        tail[e] = cs + e < d ? t : 0.0;
      }
#pragma unroll
      for (int v = 0; v < S / VW; ++v) {
        const int c = col0 + v * VW;
        const bool full = c + VW <= d;
        const V u = *reinterpret_cast<const V*>(row + (full ? c : 0));
#pragma unroll
        for (int e = 0; e < VW; ++e) {
          const double t = full ? F::wide(u[e]) : c == cs ? tail[e] : 0.0;
          x[v * VW + e] = valid ? t : 0.0;
        }
      }
      return;
    }
  }
#pragma unroll
  for (int s = 0; s < S; ++s) {
    const int c = col0 + s;
    const double t = F::wide(row[c < d ? c : 0]);
    x[s] = valid && c < d ? t : 0.0;
  }
}

template <typename F, int S>
__global__ __launch_bounds__(KMF_THREADS) void assign_kernel(const typename F::L* __restrict__ X, long n, long ldx,
                                                             int d, int vec, const double* __restrict__ W,
                                                             int ntiles, long nblocks, int* __restrict__ labels) {
  typedef Shape<S> SH;
  constexpr int PT = SH::PT, KH = SH::KH, TD = SH::TD, STAGE = SH::STAGE;
  constexpr int G = S < 4 ? S : 4;  // steps per group of operand reads
  extern __shared__ __attribute__((aligned(16))) double lds[];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int p = lane & 15, g = lane >> 4;
  const int nst = (ntiles + SH::TILES - 1) / SH::TILES;

  doublex2 pre[SH::NLD];
  auto fetch = [&](int st) {
    const doublex2* src = reinterpret_cast<const doublex2*>(W + (long)st * STAGE);
#pragma unroll
    for (int q = 0; q < SH::NLD; ++q) {
      const int c = q * KMF_THREADS + tid;
      if (SH::CHUNKS % KMF_THREADS == 0 || c < SH::CHUNKS) pre[q] = src[c];
    }
  };
  auto stash = [&](int b) {
    doublex2* dst = reinterpret_cast<doublex2*>(lds + b * STAGE);
#pragma unroll
    for (int q = 0; q < SH::NLD; ++q) {
      const int c = q * KMF_THREADS + tid;
      if (SH::CHUNKS % KMF_THREADS == 0 || c < SH::CHUNKS) dst[c] = pre[q];
    }
  };

  bool filled = false;
  for (long blk = blockIdx.x; blk < nblocks; blk += gridDim.x) {
    double x[PT][S];
#pragma unroll
    for (int pt = 0; pt < PT; ++pt) {
      const long row = blk * SH::PPB + (wv * PT + pt) * 16 + p;
      load_point<F, S>(x[pt], X + (row < n ? row : 0) * ldx, row < n, g * S, d, vec);
    }
    if (nst > 1 || !filled) {  // buffer 0 was last read before the barrier that ended the sweep
      fetch(0);
      stash(0);
      filled = true;
    }
    __syncthreads();

    double best[PT];
    int bi[PT];
#pragma unroll
    for (int pt = 0; pt < PT; ++pt) {
      best[pt] = __builtin_inf();
      bi[pt] = 0;
    }
    for (int st = 0; st < nst; ++st) {
      const bool more = st + 1 < nst;
      if (more) fetch(st + 1);
      const double* buf = lds + (st & 1) * STAGE;
      const int left = ntiles - st * SH::TILES;
      const int nt = left < SH::TILES ? left : SH::TILES;
      // an odd last tile is swept with the padding tile behind it (inside the stage: TILES is even)
      for (int t = 0; t < nt; t += 2) {
        const double* ap = buf + t * TD + lane;
        const double* cp = buf + t * TD + S * 64 + g;
        doublex4 acc[PT][2][KH];
#pragma unroll
        for (int c = 0; c < 2; ++c) {
          doublex4 cn;
#pragma unroll
          for (int r = 0; r < 4; ++r) cn[r] = cp[c * TD + 4 * r];
#pragma unroll
          for (int pt = 0; pt < PT; ++pt)
#pragma unroll
            for (int h = 0; h < KH; ++h) acc[pt][c][h] = h == 0 ? cn : doublex4{0.0, 0.0, 0.0, 0.0};
        }
        // operand reads run one group of G steps ahead of the MFMAs; the scheduling barrier keeps
        // the compiler from hoisting all 2 S reads of the pair to the top (S = 64 then spills)
        double a[2][G][2];
#pragma unroll
        for (int u = 0; u < G; ++u) {
          a[0][u][0] = ap[u * 64];
          a[0][u][1] = ap[TD + u * 64];
        }
#pragma unroll
        for (int s0 = 0; s0 < S; s0 += G) {
          const int cur = (s0 / G) & 1;
          if (s0 + G < S) {
#pragma unroll
            for (int u = 0; u < G; ++u) {
              a[cur ^ 1][u][0] = ap[(s0 + G + u) * 64];
              a[cur ^ 1][u][1] = ap[TD + (s0 + G + u) * 64];
            }
          }
#pragma unroll
          for (int u = 0; u < G; ++u) {
            const int s = s0 + u;
#pragma unroll
            for (int pt = 0; pt < PT; ++pt) {
              acc[pt][0][s % KH] =
                  __builtin_amdgcn_mfma_f64_16x16x4f64(a[cur][u][0], x[pt][s], acc[pt][0][s % KH], 0, 0, 0);
              acc[pt][1][s % KH] =
                  __builtin_amdgcn_mfma_f64_16x16x4f64(a[cur][u][1], x[pt][s], acc[pt][1][s % KH], 0, 0, 0);
            }
          }
          __builtin_amdgcn_sched_barrier(0);
        }
        const int k0 = (st * SH::TILES + t) * 16 + g;
#pragma unroll
        for (int pt = 0; pt < PT; ++pt)
#pragma unroll
          for (int c = 0; c < 2; ++c) {
            doublex4 v = acc[pt][c][0];
            if constexpr (KH == 2) v += acc[pt][c][1];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
              const bool w = v[r] < best[pt];
              best[pt] = w ? v[r] : best[pt];
              bi[pt] = w ? k0 + c * 16 + 4 * r : bi[pt];
            }
          }
      }
      if (more) stash((st + 1) & 1);
      __syncthreads();
    }

    // the four lane groups of a point: lowest (distance, index)
#pragma unroll
    for (int pt = 0; pt < PT; ++pt) {
      double v = best[pt];
      int i = bi[pt];
#pragma unroll
      for (int o = 16; o < 64; o <<= 1) {
        const double ov = __shfl_xor(v, o, 64);
        const int oi = __shfl_xor(i, o, 64);
        arg_take<false>(v, i, ov, oi);
      }
      const long row = blk * SH::PPB + (wv * PT + pt) * 16 + p;
      if (g == 0 && row < n) labels[row] = i;
    }
  }
}

// ---- sums, objective -------------------------------------------------------------------------
template <typename F, int NQ>
__global__ __launch_bounds__(256) void sums_kernel(const typename F::L* __restrict__ X, long n, long ldx, int d,
                                                   const double* __restrict__ C, const int* __restrict__ perm,
                                                   const int* __restrict__ start, int K, double* __restrict__ sums,
                                                   double* __restrict__ wss) {
  typedef typename F::L L;
  constexpr int ROWS = NQ >= 16 ? 2 : 4;  // rows in flight (16 columns per lane: two fill the registers)
  const int sl = threadIdx.x & 15;
  const long slot = ((long)blockIdx.x * 256 + threadIdx.x) >> 4;
  const long j0 = slot * KMF_RUN;
  if (j0 >= n) return;
  const long j1 = j0 + KMF_RUN < n ? j0 + KMF_RUN : n;
  // bucket containing j0: last k with start[k] <= j0
  int lo = 0, hi = K;
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (start[mid] <= j0) lo = mid; else hi = mid;
  }
  int k = lo;
  long kend = start[k + 1];
  double acc[NQ], c[NQ], w = 0.0;
#pragma unroll
  for (int q = 0; q < NQ; ++q) acc[q] = 0.0;
  auto centre = [&](int kk) {
#pragma unroll
    for (int q = 0; q < NQ; ++q) c[q] = sl + 16 * q < d ? C[(long)kk * d + sl + 16 * q] : 0.0;
  };
  auto flush = [&](int kk) {
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
      if (sl + 16 * q < d && acc[q] != 0.0) atomicAdd(sums + (long)kk * d + sl + 16 * q, acc[q]);
      acc[q] = 0.0;
    }
    // the slot's 16 lanes are one DPP row and run this together: the row moves of wave.h read
    // no lane outside it, so they are safe although other slots of the wave may be elsewhere
    w += dpp_mov_d<0x128>(w);  // row_ror:8
    w += dpp_mov_d<0x124>(w);  // row_ror:4
    w += dpp_mov_d<0x4E>(w);   // quad_perm [2,3,0,1]
    w += dpp_mov_d<0xB1>(w);   // quad_perm [1,0,3,2]
    if (sl == 0 && w != 0.0) atomicAdd(wss + kk, w);
    w = 0.0;
  };
  auto add = [&](const L (&v)[NQ]) {
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
      const double xv = sl + 16 * q < d ? F::wide(v[q]) : 0.0;
      const double t = xv - c[q];
      acc[q] += xv;
      w = fma(t, t, w);
    }
  };
  centre(k);
  long j = j0;
  while (j < j1) {
    if (j >= kend) {  // crossed into the next non-empty bucket
      flush(k);
      do {
        ++k;
        kend = start[k + 1];
      } while (j >= kend);
      centre(k);
    }
    const long stop = kend < j1 ? kend : j1;
    for (; j + ROWS <= stop; j += ROWS) {  // ROWS rows in flight inside one bucket
      L v[ROWS][NQ];
      long pj[ROWS];
#pragma unroll
      for (int r = 0; r < ROWS; ++r) pj[r] = perm[j + r];
#pragma unroll
      for (int r = 0; r < ROWS; ++r)
#pragma unroll
        for (int q = 0; q < NQ; ++q) v[r][q] = X[pj[r] * ldx + (sl + 16 * q < d ? sl + 16 * q : 0)];
#pragma unroll
      for (int r = 0; r < ROWS; ++r) add(v[r]);
    }
    for (; j < stop; ++j) {
      L v[NQ];
      const long pj = perm[j];
#pragma unroll
      for (int q = 0; q < NQ; ++q) v[q] = X[pj * ldx + (sl + 16 * q < d ? sl + 16 * q : 0)];
      add(v);
    }
  }
  flush(k);
}

// ---- launchers -------------------------------------------------------------------------------
int cu_count() {
  static const int cus = [] {
    int dev = 0, v = 0;
    if (hipGetDevice(&dev) != hipSuccess ||
        hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || v < 1)
      v = 256;
    return v;
  }();
  return cus;
}

template <int S>
long operand_doubles(int K) {
  const int ntiles = (K + 15) / 16;
  return (long)((ntiles + Shape<S>::TILES - 1) / Shape<S>::TILES) * Shape<S>::STAGE;
}

template <int S>
int launch_prepare(const double* C, long ldc, int K, int d, double* W, hipStream_t s) {
  const long total = operand_doubles<S>(K);
  prepare_kernel<S><<<dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s>>>(C, ldc, K, d, W, total);
  return harp_launch_status();
}

template <typename F, int S>
int launch_assign(const void* X, long n, long ldx, int d, const double* W, int K, int* labels, hipStream_t s) {
  typedef Shape<S> SH;
  typedef typename F::L L;
  const size_t lds = 2 * SH::STAGE * sizeof(double);
  if (lds > 65536 && hipFuncSetAttribute((const void*)assign_kernel<F, S>,
                                         hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess)
    return HARP_ELAUNCH;
  const long nblocks = (n + SH::PPB - 1) / SH::PPB;
  const long resident = (long)cu_count() * SH::WG_PER_CU;
  const int vec = (uintptr_t)X % 16 == 0 && (ldx * sizeof(L)) % 16 == 0;
  assign_kernel<F, S><<<dim3((unsigned)(nblocks < resident ? nblocks : resident)), dim3(KMF_THREADS), lds, s>>>(
      (const L*)X, n, ldx, d, vec, W, (K + 15) / 16, nblocks, labels);
  return harp_launch_status();
}

template <int S>
int launch_assign_t(const void* X, int dtype, long n, long ldx, int d, const double* W, int K, int* labels,
                    hipStream_t s) {
  if (dtype == 0) return launch_assign<InBf16, S>(X, n, ldx, d, W, K, labels, s);
  if (dtype == 1) return launch_assign<InFp32, S>(X, n, ldx, d, W, K, labels, s);
  return launch_assign<InFp64, S>(X, n, ldx, d, W, K, labels, s);
}

template <typename F>
int launch_sums(const void* X, long n, long ldx, int d, const double* C, const int* perm, const int* start, int K,
                double* sums, double* wss, hipStream_t s) {
  typedef typename F::L L;
  const long slots = (n + KMF_RUN - 1) / KMF_RUN;
  const dim3 g((unsigned)((slots + 15) / 16)), b(256);
#define KMF_SUMS(NQ) sums_kernel<F, NQ><<<g, b, 0, s>>>((const L*)X, n, ldx, d, C, perm, start, K, sums, wss)
  if (d <= 16) KMF_SUMS(1);
  else if (d <= 32) KMF_SUMS(2);
  else if (d <= 64) KMF_SUMS(4);
  else if (d <= 128) KMF_SUMS(8);
  else KMF_SUMS(16);
#undef KMF_SUMS
  return harp_launch_status();
}

}  // namespace

// every instantiated width: CALL(S) for the S that serves d
#define KMF_DISPATCH(d, CALL)   \
  switch (kmf_steps(d)) {       \
    case 1: return CALL(1);     \
    case 2: return CALL(2);     \
    case 4: return CALL(4);     \
    case 8: return CALL(8);     \
    case 16: return CALL(16);   \
    case 24: return CALL(24);   \
    case 28: return CALL(28);   \
    case 32: return CALL(32);   \
    case 48: return CALL(48);   \
    default: return CALL(64);   \
  }

HARP_EXPORT int harp_kmeans_f64_max_d() { return KMF_MAX_D; }

// What ops/kmeans_f64.py mirrors for width d (checked on first use): 0 the padded width, 1 the
// centroids of one LDS stage, 2 the points of a workgroup; -1 for anything else.
HARP_EXPORT int harp_kmeans_f64_param(int which, int d) {
  if (d < 1 || d > KMF_MAX_D || which < 0 || which > 2) return -1;
#define KMF_PARAM(S) (which == 0 ? 4 * S : which == 1 ? 16 * Shape<S>::TILES : Shape<S>::PPB)
  KMF_DISPATCH(d, KMF_PARAM)
#undef KMF_PARAM
}

// doubles of the operand harp_kmeans_f64_prepare writes for C [K, d] (0: a shape it rejects)
HARP_EXPORT long harp_kmeans_f64_operand_doubles(int K, int d) {
  if (K < 1 || K > KMF_MAX_K || d < 1 || d > KMF_MAX_D) return 0;
#define KMF_SIZE(S) operand_doubles<S>(K)
  KMF_DISPATCH(d, KMF_SIZE)
#undef KMF_SIZE
}

// W = the sweep operand of the fp64 centroids C [K, d] (row stride ldc), every element written
HARP_EXPORT int harp_kmeans_f64_prepare(const double* C, long ldc, int K, int d, double* W, hipStream_t s) {
  if (!C || !W || K < 1 || d < 1 || ldc < d) return HARP_EBADARG;
  if (K > KMF_MAX_K || d > KMF_MAX_D) return HARP_EUNSUPPORTED;
#define KMF_PREP(S) launch_prepare<S>(C, ldc, K, d, W, s)
  KMF_DISPATCH(d, KMF_PREP)
#undef KMF_PREP
}

// labels [n] int32 = the nearest of the K centroids behind W for the rows of X [n, d] (dtype 0
// bf16 / 1 fp32 / 2 fp64, unit column stride, row stride ldx >= d elements; 16-byte aligned rows
// are read with vector loads, any others with scalar loads). n = 0 launches nothing.
HARP_EXPORT int harp_kmeans_f64_assign(const void* X, int dtype, long n, long ldx, int d, const double* W, int K,
                                       int* labels, hipStream_t s) {
  if (n < 0 || d < 1 || ldx < d || K < 1 || !W || (n > 0 && (!X || !labels))) return HARP_EBADARG;
  if (K > KMF_MAX_K || d > KMF_MAX_D || dtype < 0 || dtype > 2 || n > 0x7fffffffL) return HARP_EUNSUPPORTED;
  if (n == 0) return HARP_OK;
#define KMF_ASSIGN(S) launch_assign_t<S>(X, dtype, n, ldx, d, W, K, labels, s)
  KMF_DISPATCH(d, KMF_ASSIGN)
#undef KMF_ASSIGN
}

// sums [K, d] += the rows of each bucket, wss [K] += their sum (x - c_k)^2 (both fp64, zeroed by
// the caller: partials arrive as fp64 atomic adds). perm [n], start [K + 1]: the rows sorted by
// label (ops.segment.bucket_labels). C [K, d] fp64, contiguous.
HARP_EXPORT int harp_kmeans_f64_sums(const void* X, int dtype, long n, long ldx, int d, const double* C,
                                     const int* perm, const int* start, int K, double* sums, double* wss,
                                     hipStream_t s) {
  if (n < 0 || d < 1 || ldx < d || K < 1 || !C || !sums || !wss || (n > 0 && (!X || !perm || !start)))
    return HARP_EBADARG;
  if (K > KMF_MAX_K || d > KMF_MAX_D || dtype < 0 || dtype > 2 || n > 0x7fffffffL) return HARP_EUNSUPPORTED;
  if (n == 0) return HARP_OK;
  if (dtype == 0) return launch_sums<InBf16>(X, n, ldx, d, C, perm, start, K, sums, wss, s);
  if (dtype == 1) return launch_sums<InFp32>(X, n, ldx, d, C, perm, start, K, sums, wss, s);
  return launch_sums<InFp64>(X, n, ldx, d, C, perm, start, K, sums, wss, s);
}
