// Dense multinomial naive Bayes in fp64 for gfx950 (MI355X / CDNA4): per-class feature sums and
// counts in one pass over the rows, and prediction on the fp64 matrix cores with the argmax
// fused. X (bf16 / fp32 / fp64) is read in place through its row stride and widened in
// registers; nothing of size n x C is ever built.
//
// Reference: ml/daal daal_naive/densedistri (DAAL multinomial_naive_bayes training step 1 and
// prediction on a dense table, Double throughout). harp_amd/ops/nb.py drives the kernels.
//
// class_sums_kernel. sums[y[r], :] += x_r, counts[y[r]] += 1.
//  * Workgroup (tile, split) owns the 256 columns of its tile and the row chunks split, split +
//    splits, ... (NB_CHUNK rows each); splits = min(chunks, NB_GRID / tiles), so the grid has at
//    most NB_GRID workgroups when tiles <= NB_GRID.
//  * Thread t owns column 256 tile + t and with it the LDS cells acc[c][t], C x 256 fp64 (up to
//    128 KB at C = 64; sized by C, so small C leaves room for several workgroups on a CU). No
//    other thread touches them: no atomics, no barrier inside the pass.
//  * Rows go by in blocks of NB_ROW_BYTES / sizeof(element): the labels are wave-uniform (scalar
//    loads), the values of a lane are independent global loads, and the cells are updated in row
//    pairs. Two
//    rows of different classes are two independent read-add-write chains; two rows of one class
//    are added first and take one, so a run of one class costs half the chains. The order of every
//    sum is fixed by the shape alone.
//  * A label outside [0, C) raises the error flag (a plain store of 1) and the row is skipped.
//  * Each workgroup stores its [C, tile] cells into partial [splits, C, d]; the workgroups of
//    tile 0 then count their rows per class (integer LDS adds over the labels alone: exact in
//    any order) into partial's tail [splits, C].
//
// reduce_kernel: one thread per cell adds the partials in split order: sums are bitwise
// repeatable.
//
// prepare_kernel. logTheta [C, d] in the lane order of the MFMA operand: features in slabs of
// NB_SLAB = 64, classes in tiles of 16, W[slab][tile][s][lane] = logTheta[16 tile + (lane & 15)]
// [64 slab + 16 (lane >> 4) + s], zero for a padding class or feature. A slab is one contiguous
// run whose copy to LDS is linear, a lane's operand one conflict-free ds_read_b64.
//
// predict_kernel. labels[i] = argmax_c (x_i . logTheta_c + logPrior_c).
//  * v_mfma_f64_16x16x4_f64 in the lane layout csrc/kmeans_f64.hip uses: classes are operand A
//    (rows), points operand B (columns), so register r of lane l holds class (l >> 4) + 4 r of
//    the tile for point l & 15 and the argmax over a lane's classes crosses no lane. The k index
//    of a step is permuted the same way in both operands: lane group g = l >> 4 takes the
//    contiguous features [16 g, 16 g + 16) of the slab.
//  * A workgroup of four waves owns 64 rows, a wave 16. The X slab [64, 64] is read with
//    coalesced loads (a wave-instruction reads 64 consecutive elements of one row), staged in
//    LDS in the input dtype and read back as one contiguous run of 16 elements per lane. Rows
//    past n and features past d are zero-filled in LDS, never read.
//  * Both the operand slab and the X slab have two LDS buffers: the global loads of slab s + 1
//    are issued before the MFMAs of slab s and stored after them, one barrier per slab.
//  * Epilogue: add logPrior, a running argmax over the lane's classes in ascending order (strict
//    >), then the four lane groups merge on (score, index): ties go to the lowest class. A
//    padding class is never admitted; a NaN score fails every compare and never wins; a row
//    whose scores are all NaN gets label 0. Plain stores, bitwise repeatable.
#include "common.h"

#define NB_MAX_C 64
#define NB_THREADS 256
#define NB_TILE 256   // columns of a class-sums workgroup
#define NB_CHUNK 256  // rows of a chunk
#define NB_GRID 512   // class-sums workgroups (while tiles <= NB_GRID)
#define NB_ROW_BYTES 64  // bytes in flight per lane: 8 fp64, 16 fp32 or 32 bf16 rows
#define NB_SLAB 64    // features of a predict slab
#define NB_NONE 0x7fffffff

namespace {

typedef double doublex4 __attribute__((ext_vector_type(4)));
typedef double doublex2 __attribute__((ext_vector_type(2)));

struct InBf16 {
  typedef uint16_t L;
  static constexpr int PAD = 8;
  static __device__ __forceinline__ double wide(L v) { return (double)__uint_as_float((uint32_t)v << 16); }
};
struct InFp32 {
  typedef float L;
  static constexpr int PAD = 4;
  static __device__ __forceinline__ double wide(L v) { return (double)v; }
};
struct InFp64 {
  typedef double L;
  static constexpr int PAD = 2;
  static __device__ __forceinline__ double wide(L v) { return v; }
};

// ---- class sums ------------------------------------------------------------------------------
inline int sums_tiles(int d) { return (d + NB_TILE - 1) / NB_TILE; }
inline int sums_splits(long n, int d) {
  const long chunks = (n + NB_CHUNK - 1) / NB_CHUNK;
  const int tiles = sums_tiles(d);
  const long cap = NB_GRID / tiles > 0 ? NB_GRID / tiles : 1;
  return (int)(chunks < cap ? (chunks > 0 ? chunks : 1) : cap);
}

template <typename F>
__global__ __launch_bounds__(NB_THREADS) void class_sums_kernel(const typename F::L* __restrict__ X, long n,
                                                                long ldx, int d, const int* __restrict__ y, int C,
                                                                int splits, double* __restrict__ partial,
                                                                int* __restrict__ err) {
  typedef typename F::L L;
  extern __shared__ __attribute__((aligned(16))) double lds[];
  double* cell = lds + threadIdx.x;                       // acc[c][t] at cell[c * NB_TILE]
  int* cnt = reinterpret_cast<int*>(lds + C * NB_TILE);   // [C]
  const int tid = threadIdx.x, tile = blockIdx.x, split = blockIdx.y;
  const int col = tile * NB_TILE + tid;
  const bool live = col < d;
  for (int c = 0; c < C; ++c) cell[c * NB_TILE] = 0.0;
  const L* xc = X + (live ? col : 0);
  const unsigned uc = (unsigned)C;
  bool bad = false;

  auto one = [&](int c, double x) {
    if ((unsigned)c < uc) {
      cell[c * NB_TILE] += x;
    } else {
      bad = true;
    }
  };
  auto two = [&](int ca, double xa, int cb, double xb) {
    if ((unsigned)ca < uc && (unsigned)cb < uc) {  // wave-uniform
      if (ca == cb) {
        cell[ca * NB_TILE] += xa + xb;
      } else {
        const double ra = cell[ca * NB_TILE], rb = cell[cb * NB_TILE];
        cell[ca * NB_TILE] = ra + xa;
        cell[cb * NB_TILE] = rb + xb;
      }
    } else {
      one(ca, xa);
      one(cb, xb);
    }
  };

  constexpr int ROWS = NB_ROW_BYTES / sizeof(L);
  const long chunks = (n + NB_CHUNK - 1) / NB_CHUNK;
  for (long k = split; k < chunks; k += splits) {
    const long r0 = k * NB_CHUNK;
    const long r1 = r0 + NB_CHUNK < n ? r0 + NB_CHUNK : n;
    long r = r0;
    for (; r + ROWS <= r1; r += ROWS) {
      int c[ROWS];
      L v[ROWS];
#pragma unroll
      for (int i = 0; i < ROWS; ++i) c[i] = __builtin_amdgcn_readfirstlane(y[r + i]);
#pragma unroll
      for (int i = 0; i < ROWS; ++i) v[i] = xc[(r + i) * ldx];
#pragma unroll
      for (int i = 0; i < ROWS; i += 2)
        two(c[i], live ? F::wide(v[i]) : 0.0, c[i + 1], live ? F::wide(v[i + 1]) : 0.0);
    }
    for (; r < r1; ++r) {
      const int c = __builtin_amdgcn_readfirstlane(y[r]);
      const L v = xc[r * ldx];
      one(c, live ? F::wide(v) : 0.0);
    }
  }

  if (bad && tid == 0) *err = 1;
  if (live) {
    double* out = partial + (long)split * C * d + col;
    for (int c = 0; c < C; ++c) out[(long)c * d] = cell[c * NB_TILE];
  }
  if (tile == 0) {  // the rows per class: integers, so the order of the LDS adds does not matter
    if (tid < C) cnt[tid] = 0;
    __syncthreads();
    for (long k = split; k < chunks; k += splits) {
      const long r = k * NB_CHUNK + tid;
      if (r < n && (unsigned)y[r] < uc) atomicAdd(&cnt[y[r]], 1);
    }
    __syncthreads();
    if (tid < C) partial[(long)splits * C * d + (long)split * C + tid] = (double)cnt[tid];
  }
}

// out[e] = sum over the splits of partial's cell e, in split order; out = sums [C, d], then
// counts [C]
__global__ __launch_bounds__(256) void reduce_kernel(const double* __restrict__ partial, int splits, long cd, int C,
                                                     double* __restrict__ sums, double* __restrict__ counts) {
  const long e = (long)blockIdx.x * 256 + threadIdx.x;
  if (e >= cd + C) return;
  const bool is_sum = e < cd;
  const double* p = is_sum ? partial + e : partial + (long)splits * cd + (e - cd);
  const long stride = is_sum ? cd : C;
  double s = 0.0;
  for (int k = 0; k < splits; ++k) s += p[k * stride];
  if (is_sum) sums[e] = s; else counts[e - cd] = s;
}

// ---- predict ---------------------------------------------------------------------------------
inline int class_tiles(int C) { return (C + 15) / 16; }
inline long operand_doubles(int C, int d) {
  return (long)((d + NB_SLAB - 1) / NB_SLAB) * class_tiles(C) * 16 * 64;
}

__global__ __launch_bounds__(256) void prepare_kernel(const double* __restrict__ LT, long ldt, int C, int d, int T,
                                                      double* __restrict__ W, long total) {
  const long e = (long)blockIdx.x * 256 + threadIdx.x;
  if (e >= total) return;
  const int lane = (int)(e & 63), s = (int)((e >> 6) & 15);
  const long ts = e >> 10;  // slab * T + tile
  const int t = (int)(ts % T);
  const long slab = ts / T;
  const int cls = 16 * t + (lane & 15);
  const long f = slab * NB_SLAB + 16 * (lane >> 4) + s;
  W[e] = cls < C && f < d ? LT[cls * ldt + f] : 0.0;
}

template <typename F, int T>
struct PredictShape {
  typedef typename F::L L;
  static constexpr int SS = NB_SLAB + F::PAD;                // row stride of the staged X slab, elements
  static constexpr int WSLAB = T * 16 * 64;                  // doubles of an operand slab
  static constexpr int XBYTES = 64 * SS * sizeof(L);         // one X buffer (a multiple of 16)
  static constexpr int LDS = 2 * (WSLAB * 8 + XBYTES);
  static constexpr int NW = WSLAB / 2 / NB_THREADS;          // 16-byte pieces of the operand per thread
  static constexpr int NX = 64 * NB_SLAB / NB_THREADS;       // X elements per thread
  static_assert(LDS <= 160 * 1024 && XBYTES % 16 == 0, "both buffers of both slabs fit the LDS");
};

template <typename F, int T>
__global__ __launch_bounds__(NB_THREADS) void predict_kernel(const typename F::L* __restrict__ X, long n, long ldx,
                                                             int d, const double* __restrict__ W,
                                                             const double* __restrict__ prior, int C,
                                                             int* __restrict__ labels) {
  typedef typename F::L L;
  typedef PredictShape<F, T> SH;
  extern __shared__ __attribute__((aligned(16))) double lds[];
  // [W buffer 0][W buffer 1][X buffer 0][X buffer 1]
  L* xlds = reinterpret_cast<L*>(lds + 2 * SH::WSLAB);
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int p = lane & 15, g = lane >> 4;
  const long row0 = (long)blockIdx.x * 64;
  const int nsl = (d + NB_SLAB - 1) / NB_SLAB;

  doublex2 wpre[SH::NW];
  L xpre[SH::NX];
  auto fetch = [&](int sl) {
    const doublex2* src = reinterpret_cast<const doublex2*>(W + (long)sl * SH::WSLAB);
#pragma unroll
    for (int q = 0; q < SH::NW; ++q) wpre[q] = src[q * NB_THREADS + tid];
    // element (row 4 q + wv, column lane) of the slab; out of range: a valid address, value dropped
    const int f = sl * NB_SLAB + lane;
#pragma unroll
    for (int q = 0; q < SH::NX; ++q) {
      const long row = row0 + 4 * q + wv;
      const bool in = row < n && f < d;
      const L v = X[in ? row * ldx + f : 0];
      xpre[q] = in ? v : (L)0;
    }
  };
  auto stash = [&](int b) {
    doublex2* wd = reinterpret_cast<doublex2*>(lds + b * SH::WSLAB);
#pragma unroll
    for (int q = 0; q < SH::NW; ++q) wd[q * NB_THREADS + tid] = wpre[q];
    L* xd = xlds + b * (64 * SH::SS);
#pragma unroll
    for (int q = 0; q < SH::NX; ++q) xd[(4 * q + wv) * SH::SS + lane] = xpre[q];
  };

  doublex4 acc[T];
#pragma unroll
  for (int t = 0; t < T; ++t) acc[t] = doublex4{0.0, 0.0, 0.0, 0.0};

  fetch(0);
  stash(0);
  __syncthreads();
  for (int sl = 0; sl < nsl; ++sl) {
    const bool more = sl + 1 < nsl;
    if (more) fetch(sl + 1);
    const double* wb = lds + (sl & 1) * SH::WSLAB + lane;
    const L* xb = xlds + (sl & 1) * (64 * SH::SS) + (wv * 16 + p) * SH::SS + 16 * g;
    double x[16];
#pragma unroll
    for (int s = 0; s < 16; ++s) x[s] = F::wide(xb[s]);
#pragma unroll
    for (int s = 0; s < 16; ++s)
#pragma unroll
      for (int t = 0; t < T; ++t)
        acc[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(wb[(t * 16 + s) * 64], x[s], acc[t], 0, 0, 0);
    if (more) stash((sl + 1) & 1);
    __syncthreads();
  }

  // the lane's classes in ascending order, then the four lane groups of a point
  double best = -__builtin_inf();
  int bi = NB_NONE;
#pragma unroll
  for (int t = 0; t < T; ++t)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int cls = 16 * t + g + 4 * r;
      const double v = acc[t][r] + prior[cls < C ? cls : 0];
      // a number is admitted over nothing even at -inf; a NaN fails both compares
      const bool w = cls < C && (v > best || (bi == NB_NONE && v == best));
      best = w ? v : best;
      bi = w ? cls : bi;
    }
#pragma unroll
  for (int o = 16; o < 64; o <<= 1) {
    const double ov = __shfl_xor(best, o, 64);
    const int oi = __shfl_xor(bi, o, 64);
    arg_take<true>(best, bi, ov, oi);
  }
  const long row = row0 + wv * 16 + p;
  if (g == 0 && row < n) labels[row] = bi == NB_NONE ? 0 : bi;
}

template <typename F, int T>
int launch_predict(const void* X, long n, long ldx, int d, const double* W, const double* prior, int C, int* labels,
                   hipStream_t s) {
  typedef PredictShape<F, T> SH;
  if (SH::LDS > 65536 && hipFuncSetAttribute((const void*)predict_kernel<F, T>,
                                             hipFuncAttributeMaxDynamicSharedMemorySize, SH::LDS) != hipSuccess)
    return HARP_ELAUNCH;
  const long blocks = (n + 63) / 64;
  predict_kernel<F, T><<<dim3((unsigned)blocks), dim3(NB_THREADS), SH::LDS, s>>>((const typename F::L*)X, n, ldx, d,
                                                                                 W, prior, C, labels);
  return harp_launch_status();
}

template <typename F>
int launch_predict_t(const void* X, long n, long ldx, int d, const double* W, const double* prior, int C,
                     int* labels, hipStream_t s) {
  switch (class_tiles(C)) {
    case 1: return launch_predict<F, 1>(X, n, ldx, d, W, prior, C, labels, s);
    case 2: return launch_predict<F, 2>(X, n, ldx, d, W, prior, C, labels, s);
    case 3: return launch_predict<F, 3>(X, n, ldx, d, W, prior, C, labels, s);
    default: return launch_predict<F, 4>(X, n, ldx, d, W, prior, C, labels, s);
  }
}

template <typename F>
int launch_class_sums(const void* X, long n, long ldx, int d, const int* y, int C, double* partial, int* err,
                      hipStream_t s) {
  const size_t lds = (size_t)C * NB_TILE * sizeof(double) + (size_t)C * sizeof(int);
  if (lds > 65536 && hipFuncSetAttribute((const void*)class_sums_kernel<F>,
                                         hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess)
    return HARP_ELAUNCH;
  const int splits = sums_splits(n, d);
  class_sums_kernel<F><<<dim3((unsigned)sums_tiles(d), (unsigned)splits), dim3(NB_THREADS), lds, s>>>(
      (const typename F::L*)X, n, ldx, d, y, C, splits, partial, err);
  return harp_launch_status();
}

}  // namespace

HARP_EXPORT int harp_nb_max_c() { return NB_MAX_C; }

// Row splits of harp_nb_class_sums for n rows of d columns (0: a shape it rejects). The partial
// buffer holds splits * C * (d + 1) doubles.
HARP_EXPORT int harp_nb_splits(long n, int d) {
  if (n < 1 || d < 1) return 0;
  return sums_splits(n, d);
}

// partial [splits, C, d] then [splits, C] (fp64, every element written) = the per-class sums and
// counts of each split's rows of X [n, d] (dtype 0 bf16 / 1 fp32 / 2 fp64, unit column stride, row
// stride ldx >= d elements, n > 0) with labels y [n] int32. *err (int32, zeroed by the caller) is
// set to 1 when a label lies outside [0, C); such a row is skipped.
HARP_EXPORT int harp_nb_class_sums(const void* X, int dtype, long n, long ldx, int d, const int* y, int C,
                                   double* partial, int* err, hipStream_t s) {
  if (n < 1 || d < 1 || ldx < d || C < 1 || !X || !y || !partial || !err) return HARP_EBADARG;
  if (C > NB_MAX_C || dtype < 0 || dtype > 2 || sums_tiles(d) > 65535) return HARP_EUNSUPPORTED;
  if (dtype == 0) return launch_class_sums<InBf16>(X, n, ldx, d, y, C, partial, err, s);
  if (dtype == 1) return launch_class_sums<InFp32>(X, n, ldx, d, y, C, partial, err, s);
  return launch_class_sums<InFp64>(X, n, ldx, d, y, C, partial, err, s);
}

// sums [C, d], counts [C] = the splits of partial added in split order
HARP_EXPORT int harp_nb_reduce(const double* partial, int splits, int C, int d, double* sums, double* counts,
                               hipStream_t s) {
  if (!partial || !sums || !counts || splits < 1 || C < 1 || C > NB_MAX_C || d < 1) return HARP_EBADARG;
  const long cd = (long)C * d;
  reduce_kernel<<<dim3((unsigned)((cd + C + 255) / 256)), dim3(256), 0, s>>>(partial, splits, cd, C, sums, counts);
  return harp_launch_status();
}

// doubles of the operand harp_nb_prepare writes for logTheta [C, d] (0: a shape it rejects)
HARP_EXPORT long harp_nb_operand_doubles(int C, int d) {
  if (C < 1 || C > NB_MAX_C || d < 1) return 0;
  return operand_doubles(C, d);
}

// W = the predict operand of logTheta [C, d] (fp64, row stride ldt), every element written
HARP_EXPORT int harp_nb_prepare(const double* LT, long ldt, int C, int d, double* W, hipStream_t s) {
  if (!LT || !W || C < 1 || d < 1 || ldt < d) return HARP_EBADARG;
  if (C > NB_MAX_C) return HARP_EUNSUPPORTED;
  const long total = operand_doubles(C, d);
  prepare_kernel<<<dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s>>>(LT, ldt, C, d, class_tiles(C), W, total);
  return harp_launch_status();
}

// labels [n] int32 = argmax_c (x_i . logTheta_c + prior[c]) for the rows of X [n, d] (dtype and
// strides as above), W from harp_nb_prepare, prior fp64 [C]. n = 0 launches nothing.
HARP_EXPORT int harp_nb_predict(const void* X, int dtype, long n, long ldx, int d, const double* W,
                                const double* prior, int C, int* labels, hipStream_t s) {
  if (n < 0 || d < 1 || ldx < d || C < 1 || !W || !prior || (n > 0 && (!X || !labels))) return HARP_EBADARG;
  if (C > NB_MAX_C || dtype < 0 || dtype > 2 || (n + 63) / 64 > 0x7fffffffL) return HARP_EUNSUPPORTED;
  if (n == 0) return HARP_OK;
  if (dtype == 0) return launch_predict_t<InBf16>(X, n, ldx, d, W, prior, C, labels, s);
  if (dtype == 1) return launch_predict_t<InFp32>(X, n, ldx, d, W, prior, C, labels, s);
  return launch_predict_t<InFp64>(X, n, ldx, d, W, prior, C, labels, s);
}
