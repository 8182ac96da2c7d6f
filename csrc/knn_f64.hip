// Exact k-nearest-neighbour search in fp64 for gfx950 (MI355X / CDNA4): squared Euclidean
// distances on the fp64 matrix cores with the top-k fused into the sweep. No buffer proportional
// to M x N exists: a distance lives in an accumulator register and either enters a lane's list
// or is dropped. Training rows and queries (bf16 / fp32 / fp64, unit column stride, any row
// stride) are read in place and widened in registers; 16-byte aligned rows take vector loads,
// any others scalar loads.
//
// Reference: ml/daal daal_knn (DAAL kdtree_knn_classification, Double throughout). The sweep is
// the one of csrc/kmeans_f64.hip with a running top-k in place of its running arg-min; the list
// and its tie rule are those of csrc/knn.hip. harp_amd/ops/knn_f64.py drives the kernels.
//
// prepare_kernel. The sweep operand of the training rows T [N, d], in the layout
// kmeans_f64.hip's prepare_kernel documents: the width is padded to 4 S (S from knf_steps), N to
// whole stages of TILES tiles of 16 rows. A tile is S * 64 + 16 doubles: W[s][lane] =
// -2 T[16 t + (lane & 15)][(lane >> 4) S + s] (exact; zero in padding), then the 16 squared
// norms, +inf for a padding row: its distance is +inf and +inf never enters a list. The operand
// depends on the training rows alone and serves any number of searches.
//
// search_kernel<S, KK>, grid (query blocks, splits), four waves.
//  * v_mfma_f64_16x16x4_f64: training rows are operand A, queries operand B, so register r of
//    lane l holds training row (l >> 4) + 4 r of the tile for query l & 15. The lanes l & 15,
//    + 16, + 32, + 48 share a query and see disjoint training rows.
//  * A wave keeps QT 16-query tiles in registers for the whole sweep (S doubles per tile and
//    lane). QT = 2 where S <= 16 and KK <= 16, else 1: see the table below.
//  * Split sp sweeps the stages [sp per, (sp + 1) per) of the operand through two LDS buffers,
//    one barrier per stage, the global loads of stage st + 1 issued before the MFMAs of stage st.
//  * Two training tiles are swept together. Accumulators start at |t|^2 + |q|^2, so a chain
//    ends holding the distance (with QT = 1 and even S every chain is split into even and odd
//    steps, added once at the end). A negative distance is clamped to 0 before any compare; a
//    NaN stays a NaN, fails every compare and never enters a list.
//  * Every lane keeps, per query tile, a sorted register list of KK (distance, index) pairs,
//    KK = 4 / 8 / 16 / 32 >= k, key lexicographic, empty = (+inf, INT_MAX). A lane meets its
//    candidates in ascending index order, so `d < own worst` is the exact test for its own list.
//  * THE THRESHOLD INVARIANT. thr is the minimum over the query's four lanes of a full list's
//    last entry (+inf while none is full), refreshed across the lanes only at a stage boundary.
//    At that moment the lane that supplied thr holds KK >= k entries with distance <= thr, all
//    from earlier stages, hence all with a LOWER index than any candidate still to come. A later
//    candidate with d >= thr therefore has at least k entries before it in (distance, index)
//    order and cannot be among the k best: the strict reject `d >= thr` is exact under ties.
//    (A refresh inside a stage would break this: the four lanes' rows of one stage interleave.)
//    A candidate is rejected with one compare against min(own worst, thr).
//  * Epilogue: the four lists of a query merge in k rounds on the (distance, index) key and
//    row sp of a [splits, M, k] result is written with plain stores; with one split that is the
//    final [M, k]. Empty slots come out as (+inf, -1).
//
// merge_kernel<KK>: one thread per query folds the splits' sorted partials, in split order, into
// one list on the same key. Every sum has one fixed order and every store is plain: results are
// bitwise repeatable.
//
// Which (width, list length) got which form, and the compiler's resource report (hipcc -O3
// --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage): VGPRs + AGPRs per lane, one wave
// per SIMD, NO instantiation uses scratch (ScratchSize 0, no VGPR spill) and none of prepare_kernel
// (14 VGPRs) or merge_kernel (29 / 45 / 77 / 256 + 72) does. "2t" = two query tiles per wave
// (128 queries per workgroup), "1t" = one (64 queries).
//   S \ KK       4             8             16             32
//    1       2t 128+32     2t 164+24     2t 236+32     1t 256+73
//    2       2t 146+32     2t 178+32     2t 250+32     1t 256+94
//    4       2t 166+32     2t 202+32     2t 256+48     1t 256+114
//    8       2t 183+32     2t 219+32     2t 253+68     1t 256+122
//   16       2t 211+32     2t 247+32     2t 256+95     1t 256+136
//   32       1t 177+32     1t 189+32     1t 223+32     1t 256+120
//   48       1t 226+32     1t 238+32     1t 256+48     1t 256+169
//   64       1t 256+50     1t 256+64     1t 256+98     1t 256+218
// Two tiles are not taken at KK = 32 (two sets of lists are 192 registers before any query) nor
// at S >= 32 (the queries alone are 4 S registers).
#include "common.h"

#define KNF_THREADS 256
#define KNF_MAX_D 256
#define KNF_MAX_K 32
#define KNF_MAX_SPLITS 1024

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

// MFMA steps per row: the instantiated widths 4 S
constexpr int knf_steps(int d) {
  constexpr int list[] = {1, 2, 4, 8, 16, 32, 48, 64};
  for (int s : list)
    if (4 * s >= d) return s;
  return 0;
}
// training tiles of one LDS stage, doubles of a tile (operand, then norms) and of a stage
__host__ __device__ constexpr int knf_tiles(int S) { return (64 / S < 2 ? 2 : 64 / S > 16 ? 16 : 64 / S) & ~1; }
__host__ __device__ constexpr int knf_tile_doubles(int S) { return S * 64 + 16; }
__host__ __device__ constexpr int knf_stage_doubles(int S) { return knf_tiles(S) * knf_tile_doubles(S); }
constexpr int knf_list(int k) { return k <= 4 ? 4 : k <= 8 ? 8 : k <= 16 ? 16 : 32; }

template <int S, int KK>
struct Shape {
  static constexpr int QT = S <= 16 && KK <= 16 ? 2 : 1;      // query tiles of a wave
  static constexpr int KH = QT == 1 && S % 2 == 0 ? 2 : 1;    // chains per (query tile, training tile)
  static constexpr int QPB = 4 * QT * 16;                     // queries of a workgroup
  static constexpr int TILES = knf_tiles(S);
  static constexpr int TD = knf_tile_doubles(S);
  static constexpr int STAGE = knf_stage_doubles(S);
  static constexpr int CHUNKS = STAGE / 2;                    // its 16-byte pieces
  static constexpr int NLD = (CHUNKS + KNF_THREADS - 1) / KNF_THREADS;
  static_assert(2 * STAGE * sizeof(double) <= 160 * 1024, "both buffers fit the LDS");
  static_assert(S % KH == 0 && TILES % 2 == 0, "chains and tile pairs come out even");
};

// ---- the operand -----------------------------------------------------------------------------
template <typename F>
__global__ __launch_bounds__(256) void prepare_kernel(const typename F::L* __restrict__ T, long ldt, long N, int d,
                                                      int S, double* __restrict__ W, long total) {
  const int TD = knf_tile_doubles(S);
  const long e = (long)blockIdx.x * 256 + threadIdx.x;
  if (e >= total) return;
  const long t = e / TD;
  const int o = (int)(e - t * TD);
  double v;
  if (o < S * 64) {
    const int s = o >> 6, l = o & 63;
    const long row = t * 16 + (l & 15);
    const int col = (l >> 4) * S + s;
    v = row < N && col < d ? -2.0 * F::wide(T[row * ldt + col]) : 0.0;
  } else {
    const long row = t * 16 + (o - S * 64);
    v = __builtin_inf();
    if (row < N) {
      v = 0.0;
      for (int j = 0; j < d; ++j) {
        const double a = F::wide(T[row * ldt + j]);
        v = fma(a, a, v);
      }
    }
  }
  W[e] = v;
}

// ---- search ----------------------------------------------------------------------------------
// The S columns from col0 of one row, widened; zero past d and for a row past the last.
template <typename F, int S>
__device__ __forceinline__ void load_point(double (&x)[S], const typename F::L* __restrict__ row, bool valid,
                                           int col0, int d, int vec) {
  typedef typename F::V V;
  constexpr int VW = 16 / sizeof(typename F::L);
  // No branch per load: an address out of range is replaced by one inside the row and the value
  // dropped. S % VW == 0 implies d > VW (knf_steps), so the vector at column 0 is inside the row.
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

// knn.hip's list_insert on doubles: one branchless compare-exchange sweep, key (distance, index)
template <int KK>
__device__ __forceinline__ void list_insert(double (&dl)[KK], int (&il)[KK], double d, int j) {
  double cd = d;
  int cj = j;
#pragma unroll
  for (int i = 0; i < KK; ++i) {
    const bool s = cd < dl[i] || (cd == dl[i] && cj < il[i]);
    const double td = s ? dl[i] : cd;
    const int tj = s ? il[i] : cj;
    dl[i] = s ? cd : dl[i];
    il[i] = s ? cj : il[i];
    cd = td;
    cj = tj;
  }
}

template <int S, int KK>
__global__ __launch_bounds__(KNF_THREADS) void search_kernel(const void* __restrict__ Q, int dtype, long M, long ldq,
                                                             int d, int vec, const double* __restrict__ W, int nst,
                                                             int per, int k, double* __restrict__ outD,
                                                             int* __restrict__ outI) {
  typedef Shape<S, KK> SH;
  constexpr int QT = SH::QT, KH = SH::KH, TD = SH::TD, STAGE = SH::STAGE;
  constexpr int G = S < 4 ? S : 4;  // steps per group of operand reads
  extern __shared__ __attribute__((aligned(16))) double lds[];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int p = lane & 15, g = lane >> 4;
  const long s0l = (long)blockIdx.y * per;
  const int st0 = s0l < nst ? (int)s0l : nst;
  const int st1 = st0 + per < nst ? st0 + per : nst;  // an empty range writes empty lists

  doublex2 pre[SH::NLD];
  auto fetch = [&](int st) {
    const doublex2* src = reinterpret_cast<const doublex2*>(W + (long)st * STAGE);
#pragma unroll
    for (int q = 0; q < SH::NLD; ++q) {
      const int c = q * KNF_THREADS + tid;
      if (SH::CHUNKS % KNF_THREADS == 0 || c < SH::CHUNKS) pre[q] = src[c];
    }
  };
  auto stash = [&](int b) {
    doublex2* dst = reinterpret_cast<doublex2*>(lds + b * STAGE);
#pragma unroll
    for (int q = 0; q < SH::NLD; ++q) {
      const int c = q * KNF_THREADS + tid;
      if (SH::CHUNKS % KNF_THREADS == 0 || c < SH::CHUNKS) dst[c] = pre[q];
    }
  };

  // the queries of this wave and their squared norms, the same bits in the query's four lanes
  double x[QT][S], qn[QT];
#pragma unroll
  for (int qt = 0; qt < QT; ++qt) {
    const long row = (long)blockIdx.x * SH::QPB + (wv * QT + qt) * 16 + p;
    const bool valid = row < M;
    const long off = (valid ? row : 0) * ldq;
    if (dtype == 0) load_point<InBf16, S>(x[qt], (const uint16_t*)Q + off, valid, g * S, d, vec);
    else if (dtype == 1) load_point<InFp32, S>(x[qt], (const float*)Q + off, valid, g * S, d, vec);
    else load_point<InFp64, S>(x[qt], (const double*)Q + off, valid, g * S, d, vec);
    double part = 0.0;
#pragma unroll
    for (int s = 0; s < S; ++s) part = fma(x[qt][s], x[qt][s], part);
    qn[qt] = (__shfl(part, p, 64) + __shfl(part, p + 16, 64)) + (__shfl(part, p + 32, 64) + __shfl(part, p + 48, 64));
  }

  double dl[QT][KK], thr[QT];
  int il[QT][KK];
#pragma unroll
  for (int qt = 0; qt < QT; ++qt) {
    thr[qt] = __builtin_inf();
#pragma unroll
    for (int i = 0; i < KK; ++i) {
      dl[qt][i] = __builtin_inf();
      il[qt][i] = 0x7fffffff;
    }
  }

  if (st0 < st1) {
    fetch(st0);
    stash(0);
  }
  __syncthreads();
  for (int st = st0; st < st1; ++st) {
    const bool more = st + 1 < st1;
    if (more) fetch(st + 1);
    const double* buf = lds + ((st - st0) & 1) * STAGE;
    // every tile of the stage: the operand is padded to whole stages with rows at +inf
    // (not unrolled: the list code of one pair is long enough)
#pragma unroll 1
    for (int t = 0; t < SH::TILES; t += 2) {
      const double* ap = buf + t * TD + lane;
      const double* cp = buf + t * TD + S * 64 + g;
      doublex4 acc[QT][2][KH];
#pragma unroll
      for (int c = 0; c < 2; ++c) {
        doublex4 tn;
#pragma unroll
        for (int r = 0; r < 4; ++r) tn[r] = cp[c * TD + 4 * r];
#pragma unroll
        for (int qt = 0; qt < QT; ++qt)
#pragma unroll
          for (int h = 0; h < KH; ++h) acc[qt][c][h] = h == 0 ? tn + qn[qt] : doublex4{0.0, 0.0, 0.0, 0.0};
      }
      // operand reads run one group of G steps ahead of the MFMAs; the scheduling barrier keeps
      // the compiler from hoisting all 2 S reads of the pair to the top
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
          for (int qt = 0; qt < QT; ++qt) {
            acc[qt][0][s % KH] =
                __builtin_amdgcn_mfma_f64_16x16x4f64(a[cur][u][0], x[qt][s], acc[qt][0][s % KH], 0, 0, 0);
            acc[qt][1][s % KH] =
                __builtin_amdgcn_mfma_f64_16x16x4f64(a[cur][u][1], x[qt][s], acc[qt][1][s % KH], 0, 0, 0);
          }
        }
        __builtin_amdgcn_sched_barrier(0);
      }
      // ascending training index within the lane: tile c, then register r
      const int j0 = (int)(((unsigned)st * SH::TILES + t) * 16u + g);
#pragma unroll
      for (int qt = 0; qt < QT; ++qt)
#pragma unroll
        for (int c = 0; c < 2; ++c) {
          doublex4 v = acc[qt][c][0];
          if constexpr (KH == 2) v += acc[qt][c][1];
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const double dist = v[r] < 0.0 ? 0.0 : v[r];  // a NaN stays a NaN
            // The branch is wave-uniform: a lane that rejects inserts the empty pair, which moves
            // nothing. (A per-lane branch costs the wave the same and made the compiler keep
            // copies of the lists: the KK = 32 forms with S <= 16 then used scratch.)
            const bool take = dist < fmin(dl[qt][KK - 1], thr[qt]);
            if (__builtin_amdgcn_ballot_w64(take) != 0)
              list_insert<KK>(dl[qt], il[qt], take ? dist : __builtin_inf(), take ? j0 + c * 16 + 4 * r : 0x7fffffff);
          }
        }
    }
    if (more) stash((st + 1 - st0) & 1);
    __syncthreads();
    // the stage boundary: the only place where the four lanes of a query exchange their bound
#pragma unroll
    for (int qt = 0; qt < QT; ++qt) {
      double w = dl[qt][KK - 1];
      w = fmin(w, __shfl_xor(w, 16, 64));
      thr[qt] = fmin(w, __shfl_xor(w, 32, 64));
    }
  }

  // the four lists of a query, k rounds: the lowest head by (distance, index) goes out, its lane
  // shifts its list by one
#pragma unroll
  for (int qt = 0; qt < QT; ++qt) {
    const long row = (long)blockIdx.x * SH::QPB + (wv * QT + qt) * 16 + p;
    const long o = ((long)blockIdx.y * M + row) * k;
    for (int r = 0; r < k; ++r) {
      double mv = dl[qt][0];
      int mi = il[qt][0];
#pragma unroll
      for (int sh = 16; sh < 64; sh <<= 1) {
        const double ov = __shfl_xor(mv, sh, 64);
        const int oi = __shfl_xor(mi, sh, 64);
        arg_take<false>(mv, mi, ov, oi);
      }
      if (g == 0 && row < M) {
        outD[o + r] = mv;
        outI[o + r] = mi == 0x7fffffff ? -1 : mi;
      }
      if (il[qt][0] == mi) {  // indices are distinct across the lanes (all four when all are empty)
#pragma unroll
        for (int i = 0; i + 1 < KK; ++i) {
          dl[qt][i] = dl[qt][i + 1];
          il[qt][i] = il[qt][i + 1];
        }
        dl[qt][KK - 1] = __builtin_inf();
        il[qt][KK - 1] = 0x7fffffff;
      }
    }
  }
}

// ---- merge of the splits ---------------------------------------------------------------------
template <int KK>
__global__ __launch_bounds__(64) void merge_kernel(const double* __restrict__ pd, const int* __restrict__ pi,
                                                   int splits, long M, int k, double* __restrict__ outD,
                                                   int* __restrict__ outI) {
  const long q = (long)blockIdx.x * 64 + threadIdx.x;
  if (q >= M) return;
  double dl[KK];
  int il[KK];
#pragma unroll
  for (int i = 0; i < KK; ++i) {
    dl[i] = __builtin_inf();
    il[i] = 0x7fffffff;
  }
  for (int sp = 0; sp < splits; ++sp) {
    const long o = ((long)sp * M + q) * k;
    for (int j = 0; j < k; ++j) {
      const double dv = pd[o + j];
      const int iv = pi[o + j];
      // a partial is sorted on the key: behind its first reject (or empty slot) all are rejects
      if (iv < 0 || !(dv < dl[KK - 1] || (dv == dl[KK - 1] && iv < il[KK - 1]))) break;
      list_insert<KK>(dl, il, dv, iv);
    }
  }
#pragma unroll
  for (int i = 0; i < KK; ++i)
    if (i < k) {
      outD[q * k + i] = dl[i];
      outI[q * k + i] = il[i] == 0x7fffffff ? -1 : il[i];
    }
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

long stage_count(long N, int S) {
  const long ntiles = (N + 15) / 16;
  return (ntiles + knf_tiles(S) - 1) / knf_tiles(S);
}

template <int S, int KK>
int launch_search(const void* Q, int dtype, long M, long ldq, int d, const double* W, long N, int k, int splits,
                  double* outD, int* outI, hipStream_t s) {
  typedef Shape<S, KK> SH;
  const size_t lds = 2 * SH::STAGE * sizeof(double);
  if (lds > 65536 && hipFuncSetAttribute((const void*)search_kernel<S, KK>,
                                         hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess)
    return HARP_ELAUNCH;
  const long nst = stage_count(N, S);
  const long qblocks = (M + SH::QPB - 1) / SH::QPB;
  if (nst > 0x7fffffffL || qblocks > 0x7fffffffL) return HARP_EUNSUPPORTED;
  const size_t esz = dtype == 0 ? 2 : dtype == 1 ? 4 : 8;
  const int vec = (uintptr_t)Q % 16 == 0 && (ldq * esz) % 16 == 0;
  const int per = (int)((nst + splits - 1) / splits);
  search_kernel<S, KK><<<dim3((unsigned)qblocks, (unsigned)splits), dim3(KNF_THREADS), lds, s>>>(
      Q, dtype, M, ldq, d, vec, W, (int)nst, per, k, outD, outI);
  return harp_launch_status();
}

// The launcher's split count: enough workgroups to cover the CUs when the queries alone do not,
// every split at least 8 stages long.
template <int S, int KK>
int choose_splits(long M, long N) {
  const long qblocks = (M + Shape<S, KK>::QPB - 1) / Shape<S, KK>::QPB;
  const long nst = stage_count(N, S);
  long sp = qblocks > 0 ? cu_count() / qblocks : 1;
  if (sp > nst / 8) sp = nst / 8;
  if (sp > KNF_MAX_SPLITS) sp = KNF_MAX_SPLITS;
  return sp < 1 ? 1 : (int)sp;
}

}  // namespace

// every instantiated (width, list length): CALL(S, KK)
#define KNF_DISPATCH_K(k, S, CALL)          \
  switch (knf_list(k)) {                    \
    case 4: return CALL(S, 4);              \
    case 8: return CALL(S, 8);              \
    case 16: return CALL(S, 16);            \
    default: return CALL(S, 32);            \
  }
#define KNF_DISPATCH(d, k, CALL)                 \
  switch (knf_steps(d)) {                        \
    case 1: KNF_DISPATCH_K(k, 1, CALL)           \
    case 2: KNF_DISPATCH_K(k, 2, CALL)           \
    case 4: KNF_DISPATCH_K(k, 4, CALL)           \
    case 8: KNF_DISPATCH_K(k, 8, CALL)           \
    case 16: KNF_DISPATCH_K(k, 16, CALL)         \
    case 32: KNF_DISPATCH_K(k, 32, CALL)         \
    case 48: KNF_DISPATCH_K(k, 48, CALL)         \
    default: KNF_DISPATCH_K(k, 64, CALL)         \
  }

HARP_EXPORT int harp_knn_f64_max_d() { return KNF_MAX_D; }
HARP_EXPORT int harp_knn_f64_max_k() { return KNF_MAX_K; }

// What ops/knn_f64.py mirrors for width d and list length k (checked on first use): 0 the padded
// width, 1 the training rows of one LDS stage, 2 the queries of a workgroup; -1 for anything else.
HARP_EXPORT int harp_knn_f64_param(int which, int d, int k) {
  if (d < 1 || d > KNF_MAX_D || k < 1 || k > KNF_MAX_K || which < 0 || which > 2) return -1;
#define KNF_PARAM(S, KK) (which == 0 ? 4 * S : which == 1 ? 16 * Shape<S, KK>::TILES : Shape<S, KK>::QPB)
  KNF_DISPATCH(d, k, KNF_PARAM)
#undef KNF_PARAM
}

// doubles of the operand harp_knn_f64_prepare writes for T [N, d] (0: a shape it rejects)
HARP_EXPORT long harp_knn_f64_operand_doubles(long N, int d) {
  if (N < 1 || N > 0x7fffffffL || d < 1 || d > KNF_MAX_D) return 0;
  const int S = knf_steps(d);
  return stage_count(N, S) * knf_stage_doubles(S);
}

// W = the sweep operand of the training rows T [N, d] (dtype 0 bf16 / 1 fp32 / 2 fp64, unit
// column stride, row stride ldt >= d elements), every element written
HARP_EXPORT int harp_knn_f64_prepare(const void* T, int dtype, long N, long ldt, int d, double* W, hipStream_t s) {
  if (!T || !W || N < 1 || d < 1 || ldt < d) return HARP_EBADARG;
  if (N > 0x7fffffffL || d > KNF_MAX_D || dtype < 0 || dtype > 2) return HARP_EUNSUPPORTED;
  const int S = knf_steps(d);
  const long total = stage_count(N, S) * knf_stage_doubles(S);
  const long blocks = (total + 255) / 256;
  if (blocks > 0x7fffffffL) return HARP_EUNSUPPORTED;
  const dim3 g((unsigned)blocks), b(256);
  if (dtype == 0) prepare_kernel<InBf16><<<g, b, 0, s>>>((const uint16_t*)T, ldt, N, d, S, W, total);
  else if (dtype == 1) prepare_kernel<InFp32><<<g, b, 0, s>>>((const float*)T, ldt, N, d, S, W, total);
  else prepare_kernel<InFp64><<<g, b, 0, s>>>((const double*)T, ldt, N, d, S, W, total);
  return harp_launch_status();
}

// the split count harp_knn_f64_search's caller should use for M queries on N training rows
HARP_EXPORT int harp_knn_f64_splits(long M, long N, int d, int k) {
  if (M < 1 || N < 1 || d < 1 || d > KNF_MAX_D || k < 1 || k > KNF_MAX_K) return 1;
#define KNF_SPLITS(S, KK) choose_splits<S, KK>(M, N)
  KNF_DISPATCH(d, k, KNF_SPLITS)
#undef KNF_SPLITS
}

// outD / outI [splits, M, k] (fp64, int32): row sp holds, for each query of Q [M, d] (dtype and
// strides as for prepare), the k nearest among the training rows of split sp behind W, ascending
// on (distance, index), empty slots (+inf, -1). splits = 1 gives the final result. M = 0
// launches nothing.
HARP_EXPORT int harp_knn_f64_search(const void* Q, int dtype, long M, long ldq, int d, const double* W, long N,
                                    int k, int splits, double* outD, int* outI, hipStream_t s) {
  if (M < 0 || N < 1 || d < 1 || ldq < d || k < 1 || splits < 1 || !W || (M > 0 && (!Q || !outD || !outI)))
    return HARP_EBADARG;
  if (N > 0x7fffffffL || d > KNF_MAX_D || k > KNF_MAX_K || splits > KNF_MAX_SPLITS || dtype < 0 || dtype > 2)
    return HARP_EUNSUPPORTED;
  if (M == 0) return HARP_OK;
#define KNF_SEARCH(S, KK) launch_search<S, KK>(Q, dtype, M, ldq, d, W, N, k, splits, outD, outI, s)
  KNF_DISPATCH(d, k, KNF_SEARCH)
#undef KNF_SEARCH
}

// out [M, k] = the k best of the partials pd / pi [splits, M, k], taken in split order
HARP_EXPORT int harp_knn_f64_merge(const double* pd, const int* pi, int splits, long M, int k, double* outD,
                                   int* outI, hipStream_t s) {
  if (M < 0 || k < 1 || k > KNF_MAX_K || splits < 1 || (M > 0 && (!pd || !pi || !outD || !outI))) return HARP_EBADARG;
  if (M == 0) return HARP_OK;
  const long blocks = (M + 63) / 64;
  if (blocks > 0x7fffffffL) return HARP_EUNSUPPORTED;
  const dim3 g((unsigned)blocks), b(64);
  switch (knf_list(k)) {
    case 4: merge_kernel<4><<<g, b, 0, s>>>(pd, pi, splits, M, k, outD, outI); break;
    case 8: merge_kernel<8><<<g, b, 0, s>>>(pd, pi, splits, M, k, outD, outI); break;
    case 16: merge_kernel<16><<<g, b, 0, s>>>(pd, pi, splits, M, k, outD, outI); break;
    default: merge_kernel<32><<<g, b, 0, s>>>(pd, pi, splits, M, k, outD, outI); break;
  }
  return harp_launch_status();
}
