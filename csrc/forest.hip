// Level-wise decision-forest training and packed-forest inference for gfx950 (MI355X / CDNA4).
//
// Replaces the hot loops of the reference's DAAL decision tree / decision forest batch
// launchers (ml/daal daal_dtree, daal_dforest) and of the contrib random forests: histogram
// split search over quantile-binned features, all trees of a batch grown together one level
// at a time. harp_amd/ops/forest.py drives one hist -> split -> route pass per level and
// holds the CPU torch mirror of every kernel here (the oracle of tests/test_forest_gpu.py).
//
// Layout. Binned features are uint8 [n, dpad], dpad = d rounded up to 16: a row is a whole
// number of 16-byte segments, so the histogram and route passes, which visit rows through a
// permutation, touch whole aligned segments of the rows they visit and nothing of the rows
// they skip (a feature-major layout would gather one byte per cache line per feature).
//
// Frontier. A level's frontier is flat over the batch: node j (0 <= j < M) belongs to tree
// fr_tree[j], has id fr_node[j] inside it and owns rows order[start[j] .. start[j]+cnt[j]).
// Rows with multiplicity 0 never enter `order`; rows of nodes that became leaves drop out.
// A chunk is at most FOREST_CHUNK consecutive rows of ONE node; chunk_off[j] is the number of
// chunks before node j (exclusive scan, chunk_off[M] = total). Kernels are launched with the
// host-side upper bound on the number of chunks; a block finds its node by binary search and
// blocks past chunk_off[M] exit, so no chunk count has to travel to the host.
//
// hist. One workgroup per (chunk, feature group). It accumulates the chunk in LDS (integer
// ds_add for `count`, ds_add_f64 for `real`) and flushes once: at most one global atomic per
// (chunk, feature-group cell), zero cells are skipped. A feature group is as many features as
// fit 64 KiB of LDS (n_bins * classes * 8 B <= 64 KiB holds at the limits 256 x 32). `count`
// adds are integer, so the histogram is exact and independent of order; `real` sums depend
// on arrival order in the last bits. Sibling subtraction is NOT used: both children are
// accumulated from their rows.
//
// feature subsets. harp_forest_feature_subset hashes (seed, tree, node, feature) and marks the k
// smallest per node in a [M, d] byte mask (M * d threads, d hashes each: noise next to the
// histogram pass); the split kernel reads one byte per (node, feature) instead of hashing d
// times per wave.
//
// split. harp_forest_split_feature runs one wave per (node, feature): the slice is staged in
// LDS, scanned over bins (class per lane; `real` scans each class sequentially so the sums
// equal a sequential cumsum bit for bit, `count` scans segments in parallel since integer sums
// have no order), then every lane scores bins lane, lane+64, .. in fp64 and a wave arg-max
// keeps the best bin (lowest bin among bitwise-equal gains). The arithmetic is written
// without fused multiply-add and sums classes in index order, and entropy uses the log2
// below built from + - * / only, so the torch mirror reproduces every gain bit for bit.
// harp_forest_split_node runs one wave per node: it reduces the per-feature candidates (tie:
// lowest feature, hence lowest feature*(B-1)+bin), decides gain > 1e-12 and writes the left /
// right / total statistics. Child numbering and the next frontier are prefix sums over the
// split flags, done with torch scans on the device between the kernels (no host read).
//
// route. harp_forest_route_count counts the rows of each split node that go left (one integer
// atomic per chunk); harp_forest_route_scatter moves the rows into the children's ranges,
// reserving slots through LDS counters and one global atomic per (block pass, side). The order
// inside a child is arbitrary.
//
// predict / apply. One thread per sample walks every tree of the packed forest on raw
// x >= threshold and sums the leaf values in tree order: no atomics, reproducible.
//
// No kernel waits on another workgroup; all stores are vector stores.
#include "common.h"

#pragma clang fp contract(off)

#define FOREST_CHUNK 2048
#define FOREST_LDS_BYTES 65536
#define FOREST_MAX_BINS 256
#define FOREST_MAX_CLASSES 32

namespace {

// ------------------------------------------------------------------ counter-based hash
__device__ __forceinline__ uint32_t fmix(uint32_t h) {
  h ^= h >> 16;
  h *= 0x85EBCA6Bu;
  h ^= h >> 13;
  h *= 0xC2B2AE35u;
  h ^= h >> 16;
  return h;
}
__device__ __forceinline__ uint32_t hash3(uint32_t a, uint32_t b, uint32_t c) {
  uint32_t h = fmix(a + 0x9E3779B9u);
  h = fmix(h ^ (b * 0x85EBCA77u));
  h = fmix(h ^ (c * 0xC2B2AE3Du));
  return h;
}
__device__ __forceinline__ uint32_t hash4(uint32_t a, uint32_t b, uint32_t c, uint32_t d) {
  return fmix(hash3(a, b, c) ^ (d * 0x27D4EB2Fu));
}

// node of chunk `b`: the j with chunk_off[j] <= b < chunk_off[j + 1]; -1 past the end
__device__ __forceinline__ int chunk_node(const int* __restrict__ chunk_off, int M, int b) {
  if (b >= chunk_off[M]) return -1;
  int lo = 0, hi = M - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (chunk_off[mid] <= b) lo = mid;
    else hi = mid - 1;
  }
  return lo;
}

// ------------------------------------------------------------------ bin
template <typename T>
__global__ __launch_bounds__(256) void bin_kernel(const T* __restrict__ X, long n, int d, const double* __restrict__ th,
                                                  int nth, uint8_t* __restrict__ Xb, int dpad) {
  const long total = n * d;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const long r = i / d;
    const int f = (int)(i - r * d);
    const double x = (double)X[i];
    const double* t = th + (long)f * nth;
    int lo = 0, hi = nth;  // number of thresholds <= x
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (t[mid] <= x) lo = mid + 1;
      else hi = mid;
    }
    Xb[r * dpad + f] = (uint8_t)lo;
  }
}

// ------------------------------------------------------------------ bootstrap
__global__ __launch_bounds__(256) void bootstrap_kernel(uint32_t seed, int tree0, int T, long row0, long n,
                                                        const uint32_t* __restrict__ table,
                                                        uint8_t* __restrict__ w) {
  uint32_t tab[15];
#pragma unroll
  for (int k = 0; k < 15; ++k) tab[k] = table[k];
  const long total = (long)T * n;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const long t = i / n;
    const long r = i - t * n;
    const uint32_t u = hash3(seed, (uint32_t)(tree0 + t), (uint32_t)(row0 + r));
    int m = 0;
#pragma unroll
    for (int k = 0; k < 15; ++k) m += u >= tab[k] ? 1 : 0;
    w[i] = (uint8_t)m;
  }
}

// ------------------------------------------------------------------ feature subset
__global__ __launch_bounds__(256) void subset_kernel(uint32_t seed, const int* __restrict__ fr_tree,
                                                     const int* __restrict__ fr_node, int M, int d, int k,
                                                     uint8_t* __restrict__ mask) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (long)M * d) return;
  const int j = (int)(i / d), f = (int)(i % d);
  const uint32_t t = (uint32_t)fr_tree[j], nd = (uint32_t)fr_node[j];
  const uint32_t hf = hash4(seed, t, nd, (uint32_t)f);
  int below = 0;
  for (int g = 0; g < d; ++g) {
    const uint32_t hg = hash4(seed, t, nd, (uint32_t)g);
    below += (hg < hf || (hg == hf && g < f)) ? 1 : 0;
  }
  mask[i] = below < k ? 1 : 0;
}

// ------------------------------------------------------------------ hist
// KIND 0: count (uint32 cells, label y + multiplicity); KIND 1: real (fp64 cells, stats [n, C]
// times multiplicity).
template <typename T>
__global__ __launch_bounds__(256) void hist_kernel(const uint8_t* __restrict__ Xb, int dpad,
                                                   const int* __restrict__ order, const int* __restrict__ start,
                                                   const int* __restrict__ cnt, const int* __restrict__ fr_tree,
                                                   const int* __restrict__ chunk_off, int M,
                                                   const uint8_t* __restrict__ mult, long n,
                                                   const int* __restrict__ y, const double* __restrict__ stats,
                                                   int d, int B, int C, int dg, T* __restrict__ H) {
  extern __shared__ double forest_smem[];
  T* cell = reinterpret_cast<T*>(forest_smem);
  const int j = chunk_node(chunk_off, M, (int)blockIdx.x);
  if (j < 0) return;  // block-uniform
  const int f0 = (int)blockIdx.y * dg;
  const int nf = min(dg, d - f0);
  if (nf <= 0) return;
  const int ncell = nf * B * C;
  for (int i = threadIdx.x; i < ncell; i += blockDim.x) cell[i] = (T)0;
  __syncthreads();
  const int c0 = ((int)blockIdx.x - chunk_off[j]) * FOREST_CHUNK;
  const int rows = min(FOREST_CHUNK, cnt[j] - c0);
  const int* ord = order + start[j] + c0;
  const uint8_t* mw = mult + (long)fr_tree[j] * n;
  const int work = rows * nf;
  for (int i = threadIdx.x; i < work; i += blockDim.x) {
    const int r = i / nf, f = i - r * nf;
    const long row = ord[r];
    const int bin = Xb[row * dpad + f0 + f];
    const unsigned m = mw[row];
    if (bin >= B || m == 0) continue;
    if constexpr (sizeof(T) == 4) {
      const int cl = y[row];
      if (cl >= 0 && cl < C) atomicAdd(&cell[(f * B + bin) * C + cl], (T)m);
    } else {
      const double* s = stats + row * C;
      for (int c = 0; c < C; ++c) {
        const double v = s[c] * (double)m;
        if (v != 0.0) atomicAdd(&cell[(f * B + bin) * C + c], (T)v);
      }
    }
  }
  __syncthreads();
  T* dst = H + ((size_t)j * d + f0) * B * C;
  for (int i = threadIdx.x; i < ncell; i += blockDim.x) {
    const T v = cell[i];
    if (v != (T)0) atomicAdd(&dst[i], v);
  }
}

// ------------------------------------------------------------------ split
// log2 of a normal positive double from + - * / only (frexp is exact): the torch mirror in
// ops/forest.py runs the same operations in the same order, so both give the same bits.
__device__ __forceinline__ double forest_log2(double p) {
  int e;
  double m = frexp(p, &e);  // m in [0.5, 1)
  if (m < 0.70710678118654752) {
    m = m * 2.0;
    e -= 1;
  }
  const double s = (m - 1.0) / (m + 1.0);
  const double z = s * s;
  double q = 1.0 / 23.0;
  q = q * z + 1.0 / 21.0;
  q = q * z + 1.0 / 19.0;
  q = q * z + 1.0 / 17.0;
  q = q * z + 1.0 / 15.0;
  q = q * z + 1.0 / 13.0;
  q = q * z + 1.0 / 11.0;
  q = q * z + 1.0 / 9.0;
  q = q * z + 1.0 / 7.0;
  q = q * z + 1.0 / 5.0;
  q = q * z + 1.0 / 3.0;
  q = q * z + 1.0;
  return (double)e + (2.0 * s * q) * 1.4426950408889634;
}

// statistics of one side of a candidate: mode 0 = left (inclusive prefix at `pre`), 1 = right
// (total - prefix), 2 = the total alone
template <typename T>
__device__ __forceinline__ double side_stat(const T* pre, const T* tot, int c, int mode) {
  if (mode == 0) return (double)pre[c];
  if (mode == 1) return (double)(T)(tot[c] - pre[c]);
  return (double)tot[c];
}

// task 0: classification gini, 1: classification entropy, 2: regression mse. Returns the
// impurity times the weight and the weight itself in *cnt (DecisionTree._impurity / _count).
template <typename T>
__device__ __forceinline__ double impurity(const T* pre, const T* tot, int C, int mode, int task, double* cnt) {
  if (task == 2) {
    const double w = side_stat(pre, tot, 0, mode), s = side_stat(pre, tot, 1, mode), ss = side_stat(pre, tot, 2, mode);
    *cnt = w;
    return ss - (s * s) / fmax(w, 1e-300);
  }
  double nn = 0.0;
  for (int c = 0; c < C; ++c) nn = nn + side_stat(pre, tot, c, mode);
  *cnt = nn;
  const double n = fmax(nn, 1e-300);
  double acc = 0.0;
  for (int c = 0; c < C; ++c) {
    const double p = side_stat(pre, tot, c, mode) / n;
    if (task == 1) acc = acc + p * forest_log2(fmax(p, 1e-300));
    else acc = acc + p * p;
  }
  return task == 1 ? (-acc) * n : (1.0 - acc) * n;
}

template <typename T>
__global__ __launch_bounds__(64) void split_feature_kernel(const T* __restrict__ H, int d, int B, int C, int task,
                                                           double min_leaf, const uint8_t* __restrict__ mask,
                                                           double* __restrict__ cand_gain,
                                                           int* __restrict__ cand_bin) {
  extern __shared__ double forest_smem[];
  T* pre = reinterpret_cast<T*>(forest_smem);
  const int lane = threadIdx.x;
  const size_t jf = blockIdx.x;  // node * d + feature
  const double ninf = -__builtin_inf();
  if ((mask && !mask[jf]) || B < 2) {  // block-uniform
    if (lane == 0) {
      cand_gain[jf] = ninf;
      cand_bin[jf] = 0;
    }
    return;
  }
  const T* src = H + jf * B * C;
  for (int i = lane; i < B * C; i += 64) pre[i] = src[i];
  __syncthreads();
  // inclusive scan over bins, class per lane; integer cells split the bins into G segments
  const int G = sizeof(T) == 4 ? max(1, 64 / C) : 1;
  const int seglen = (B + G - 1) / G;
  const int seg = lane / C, c = lane % C;
  const int b0 = seg * seglen, b1 = min(B, b0 + seglen);
  const bool act = lane < G * C && b0 < B;
  if (act) {
    T run = (T)0;
    for (int b = b0; b < b1; ++b) {
      run = run + pre[b * C + c];
      pre[b * C + c] = run;
    }
  }
  __syncthreads();
  T off = (T)0;
  if (act)
    for (int s = 0; s < seg; ++s) off = off + pre[(min(B, (s + 1) * seglen) - 1) * C + c];
  __syncthreads();
  if (act && seg > 0)
    for (int b = b0; b < b1; ++b) pre[b * C + c] = pre[b * C + c] + off;
  __syncthreads();
  const T* tot = pre + (B - 1) * C;
  double nT;
  const double impT = impurity(tot, tot, C, 2, task, &nT);
  double best = ninf;
  int bb = 0x7fffffff;
  for (int b = lane; b < B - 1; b += 64) {
    double nL, nR;
    const double iL = impurity(pre + b * C, tot, C, 0, task, &nL);
    const double iR = impurity(pre + b * C, tot, C, 1, task, &nR);
    double g = (impT - iL) - iR;
    if (!(nL >= min_leaf && nR >= min_leaf)) g = ninf;
    if (g > best) {
      best = g;
      bb = b;
    }
  }
  wave_arg_xor<true>(best, bb);
  if (lane == 0) {
    cand_gain[jf] = best;
    cand_bin[jf] = bb == 0x7fffffff ? 0 : bb;
  }
}

template <typename T>
__global__ __launch_bounds__(64) void split_node_kernel(const T* __restrict__ H, int d, int B, int C,
                                                        const double* __restrict__ cand_gain,
                                                        const int* __restrict__ cand_bin, int* __restrict__ out_f,
                                                        int* __restrict__ out_bin, double* __restrict__ out_gain,
                                                        int* __restrict__ do_split, double* __restrict__ Lst,
                                                        double* __restrict__ Rst, double* __restrict__ Tst) {
  const int lane = threadIdx.x;
  const size_t j = blockIdx.x;
  double best = -__builtin_inf();
  int bf = 0x7fffffff;
  for (int f = lane; f < d; f += 64) {
    const double g = cand_gain[j * d + f];
    if (g > best || (g == best && f < bf)) {
      best = g;
      bf = f;
    }
  }
  wave_arg_xor<true>(best, bf);
  if (bf < 0 || bf >= d) bf = 0;  // only if every gain is NaN (overflowed statistics)
  int bin = cand_bin[j * d + bf];
  if (bin < 0 || bin >= B) bin = 0;
  const bool sp = best > 1e-12;
  if (lane == 0) {
    out_f[j] = bf;
    out_bin[j] = bin;
    out_gain[j] = best;
    do_split[j] = sp ? 1 : 0;
  }
  if (lane < C) {
    const T* h = H + (j * d + bf) * B * C;
    T l = (T)0, t = (T)0;
    for (int b = 0; b < B; ++b) {
      t = t + h[b * C + lane];
      if (b == bin) l = t;
    }
    Lst[j * C + lane] = (double)l;
    Rst[j * C + lane] = (double)(T)(t - l);
    const T* h0 = H + (j * d) * B * C;
    T t0 = (T)0;
    for (int b = 0; b < B; ++b) t0 = t0 + h0[b * C + lane];
    Tst[j * C + lane] = (double)t0;
  }
}

// ------------------------------------------------------------------ route
__global__ __launch_bounds__(256) void route_count_kernel(const uint8_t* __restrict__ Xb, int dpad,
                                                          const int* __restrict__ order,
                                                          const int* __restrict__ start, const int* __restrict__ cnt,
                                                          const int* __restrict__ chunk_off, int M,
                                                          const int* __restrict__ do_split,
                                                          const int* __restrict__ sf, const int* __restrict__ sbin,
                                                          int* __restrict__ nleft) {
  __shared__ int total;
  const int j = chunk_node(chunk_off, M, (int)blockIdx.x);
  if (j < 0 || !do_split[j]) return;  // block-uniform
  if (threadIdx.x == 0) total = 0;
  __syncthreads();
  const int c0 = ((int)blockIdx.x - chunk_off[j]) * FOREST_CHUNK;
  const int rows = min(FOREST_CHUNK, cnt[j] - c0);
  const int* ord = order + start[j] + c0;
  const int f = sf[j], bin = sbin[j];
  int mine = 0;
  for (int r = threadIdx.x; r < rows; r += blockDim.x) mine += Xb[(long)ord[r] * dpad + f] > bin ? 0 : 1;
  mine = wave_sum_i(mine);
  if ((threadIdx.x & 63) == 0 && mine) atomicAdd(&total, mine);
  __syncthreads();
  if (threadIdx.x == 0 && total) atomicAdd(&nleft[j], total);
}

// child_start[j]: first slot of node j's left child in new_order; the right child follows
// its nleft[j] rows. cursor [M, 2] starts at zero.
__global__ __launch_bounds__(256) void route_scatter_kernel(const uint8_t* __restrict__ Xb, int dpad,
                                                            const int* __restrict__ order,
                                                            const int* __restrict__ start,
                                                            const int* __restrict__ cnt,
                                                            const int* __restrict__ chunk_off, int M,
                                                            const int* __restrict__ do_split,
                                                            const int* __restrict__ sf, const int* __restrict__ sbin,
                                                            const int* __restrict__ nleft,
                                                            const int* __restrict__ child_start,
                                                            int* __restrict__ cursor, int* __restrict__ new_order,
                                                            long new_len) {
  __shared__ int lcnt[2];
  __shared__ int lbase[2];
  const int j = chunk_node(chunk_off, M, (int)blockIdx.x);
  if (j < 0 || !do_split[j]) return;  // block-uniform
  const int c0 = ((int)blockIdx.x - chunk_off[j]) * FOREST_CHUNK;
  const int rows = min(FOREST_CHUNK, cnt[j] - c0);
  const int* ord = order + start[j] + c0;
  const int f = sf[j], bin = sbin[j];
  const int base0 = child_start[j], base1 = child_start[j] + nleft[j];
  for (int r0 = 0; r0 < rows; r0 += blockDim.x) {  // block-uniform trip count
    if (threadIdx.x < 2) lcnt[threadIdx.x] = 0;
    __syncthreads();
    const int r = r0 + threadIdx.x;
    int row = 0, side = 0, slot = 0;
    if (r < rows) {
      row = ord[r];
      side = Xb[(long)row * dpad + f] > bin ? 1 : 0;
      slot = atomicAdd(&lcnt[side], 1);
    }
    __syncthreads();
    if (threadIdx.x < 2 && lcnt[threadIdx.x])
      lbase[threadIdx.x] = atomicAdd(&cursor[2 * j + threadIdx.x], lcnt[threadIdx.x]);
    __syncthreads();
    if (r < rows) {
      const long at = (long)(side ? base1 : base0) + lbase[side] + slot;
      if (at >= 0 && at < new_len) new_order[at] = row;
    }
    __syncthreads();
  }
}

// ------------------------------------------------------------------ predict / apply
template <typename T>
__global__ __launch_bounds__(256) void predict_kernel(const T* __restrict__ X, long n, int d, const int* __restrict__ feat,
                                                      const double* __restrict__ thr, const int* __restrict__ left,
                                                      const double* __restrict__ value, const long* __restrict__ off,
                                                      int ntrees, int C, int max_steps, double* __restrict__ out,
                                                      long* __restrict__ leaf) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const T* x = X + i * d;
  double acc[FOREST_MAX_CLASSES];
#pragma unroll
  for (int c = 0; c < FOREST_MAX_CLASSES; ++c) acc[c] = 0.0;
  for (int t = 0; t < ntrees; ++t) {
    const long base = off[t], size = off[t + 1] - off[t];
    long node = 0;
    for (int s = 0; s < max_steps; ++s) {  // bounded: a malformed tree cannot loop forever
      const int l = left[base + node];
      if (l < 0) break;
      const int f = feat[base + node];
      if (f < 0 || f >= d) break;
      const long nx = (long)l + ((double)x[f] >= thr[base + node] ? 1 : 0);
      if (nx >= size) break;
      node = nx;
    }
    if (leaf) leaf[(long)t * n + i] = node;
    if (out) {
      const double* v = value + (base + node) * C;
#pragma unroll
      for (int c = 0; c < FOREST_MAX_CLASSES; ++c)
        if (c < C) acc[c] = acc[c] + v[c];
    }
  }
  if (out) {
#pragma unroll
    for (int c = 0; c < FOREST_MAX_CLASSES; ++c)
      if (c < C) out[i * C + c] = acc[c] / (double)ntrees;
  }
}

inline unsigned grid_for(long total, int block) {
  long g = (total + block - 1) / block;
  if (g > 8192) g = 8192;
  if (g < 1) g = 1;
  return (unsigned)g;
}

inline int shape_status(int B, int C) {
  if (B < 1 || C < 1) return HARP_EBADARG;
  if (B > FOREST_MAX_BINS || C > FOREST_MAX_CLASSES) return HARP_EUNSUPPORTED;
  return HARP_OK;
}

}  // namespace

// X [n, d] fp32 (is64 = 0) or fp64 (is64 = 1); th [d, nth] fp64, rows ascending; Xb [n, dpad]
// uint8, padding columns are left as the caller set them. bin = number of thresholds <= x.
HARP_EXPORT int harp_forest_bin(const void* X, int is64, long n, int d, const double* th, int nth, uint8_t* Xb,
                                int dpad, hipStream_t s) {
  if (n < 0 || d < 1 || nth < 0 || dpad < d) return HARP_EBADARG;
  if (nth + 1 > FOREST_MAX_BINS) return HARP_EUNSUPPORTED;
  if (n == 0) return HARP_OK;
  const dim3 g(grid_for(n * d, 256)), b(256);
  if (is64) bin_kernel<double><<<g, b, 0, s>>>((const double*)X, n, d, th, nth, Xb, dpad);
  else bin_kernel<float><<<g, b, 0, s>>>((const float*)X, n, d, th, nth, Xb, dpad);
  return harp_launch_status();
}

// w [T, n] uint8 Poisson(1) multiplicities of trees tree0 .. tree0+T-1 for the rows with
// global index row0 .. row0+n-1; table: the 15 ascending uint32 inversion thresholds.
HARP_EXPORT int harp_forest_bootstrap(unsigned seed, int tree0, int T, long row0, long n, const uint32_t* table,
                                      uint8_t* w, hipStream_t s) {
  if (T < 0 || n < 0 || row0 < 0 || tree0 < 0 || !table) return HARP_EBADARG;
  if (row0 + n > 0xffffffffL / 15) return HARP_EUNSUPPORTED;
  if (T == 0 || n == 0) return HARP_OK;
  bootstrap_kernel<<<dim3(grid_for((long)T * n, 256)), dim3(256), 0, s>>>(seed, tree0, T, row0, n, table, w);
  return harp_launch_status();
}

// mask [M, d] uint8: 1 where feature f is among the k smallest hashes of (seed, tree, node, f)
HARP_EXPORT int harp_forest_feature_subset(unsigned seed, const int* fr_tree, const int* fr_node, int M, int d, int k,
                                           uint8_t* mask, hipStream_t s) {
  if (M < 0 || d < 1 || k < 1) return HARP_EBADARG;
  if (M == 0) return HARP_OK;
  const long total = (long)M * d;
  if ((total + 255) / 256 > 0x7fffffffL) return HARP_EBADARG;
  subset_kernel<<<dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s>>>(seed, fr_tree, fr_node, M, d, k, mask);
  return harp_launch_status();
}

// H [M, d, B, C] (zeroed by the caller; uint32 for kind 0, fp64 for kind 1) += the level's
// histograms. max_chunks >= chunk_off[M]. kind 0 reads y [n] int32, kind 1 stats [n, C] fp64.
HARP_EXPORT int harp_forest_hist(const uint8_t* Xb, int dpad, const int* order, const int* start, const int* cnt,
                                 const int* fr_tree, const int* chunk_off, int M, int max_chunks,
                                 const uint8_t* mult, long n, const int* y, const double* stats, int d, int B, int C,
                                 int kind, void* H, hipStream_t s) {
  if (M < 0 || max_chunks < 0 || d < 1 || dpad < d || n < 0 || (kind != 0 && kind != 1)) return HARP_EBADARG;
  if ((kind == 0 && !y) || (kind == 1 && !stats)) return HARP_EBADARG;
  const int st = shape_status(B, C);
  if (st) return st;
  if (M == 0 || max_chunks == 0) return HARP_OK;
  const int cs = kind == 0 ? 4 : 8;
  int dg = FOREST_LDS_BYTES / (B * C * cs);
  if (dg < 1) return HARP_EUNSUPPORTED;
  if (dg > d) dg = d;
  const int groups = (d + dg - 1) / dg;
  if (groups > 65535) return HARP_EUNSUPPORTED;
  const dim3 g((unsigned)max_chunks, (unsigned)groups), b(256);
  const size_t lds = (size_t)dg * B * C * cs;
  if (kind == 0)
    hist_kernel<uint32_t><<<g, b, lds, s>>>(Xb, dpad, order, start, cnt, fr_tree, chunk_off, M, mult, n, y, stats, d,
                                            B, C, dg, (uint32_t*)H);
  else
    hist_kernel<double><<<g, b, lds, s>>>(Xb, dpad, order, start, cnt, fr_tree, chunk_off, M, mult, n, y, stats, d, B,
                                          C, dg, (double*)H);
  return harp_launch_status();
}

// Per (node, feature) best bin and gain. task 0 gini, 1 entropy, 2 mse (C = 3). mask [M, d]
// uint8 or null (all features allowed).
HARP_EXPORT int harp_forest_split_feature(const void* H, int kind, int M, int d, int B, int C, int task,
                                          double min_leaf, const uint8_t* mask, double* cand_gain, int* cand_bin,
                                          hipStream_t s) {
  if (M < 0 || d < 1 || (kind != 0 && kind != 1) || task < 0 || task > 2) return HARP_EBADARG;
  if (task == 2 && (C != 3 || kind != 1)) return HARP_EBADARG;
  const int st = shape_status(B, C);
  if (st) return st;
  if (M == 0) return HARP_OK;
  const long blocks = (long)M * d;
  if (blocks > 0x7fffffffL) return HARP_EBADARG;
  const size_t lds = (size_t)B * C * (kind == 0 ? 4 : 8);
  if (kind == 0)
    split_feature_kernel<uint32_t><<<dim3((unsigned)blocks), dim3(64), lds, s>>>((const uint32_t*)H, d, B, C, task,
                                                                              min_leaf, mask, cand_gain, cand_bin);
  else
    split_feature_kernel<double><<<dim3((unsigned)blocks), dim3(64), lds, s>>>((const double*)H, d, B, C, task,
                                                                            min_leaf, mask, cand_gain, cand_bin);
  return harp_launch_status();
}

// Per node: best feature / bin / gain over the candidates, the split decision (gain > 1e-12)
// and the left / right / total statistics [M, C] as fp64.
HARP_EXPORT int harp_forest_split_node(const void* H, int kind, int M, int d, int B, int C, const double* cand_gain,
                                       const int* cand_bin, int* out_f, int* out_bin, double* out_gain, int* do_split,
                                       double* Lst, double* Rst, double* Tst, hipStream_t s) {
  if (M < 0 || d < 1 || (kind != 0 && kind != 1)) return HARP_EBADARG;
  const int st = shape_status(B, C);
  if (st) return st;
  if (M == 0) return HARP_OK;
  if (kind == 0)
    split_node_kernel<uint32_t><<<dim3((unsigned)M), dim3(64), 0, s>>>((const uint32_t*)H, d, B, C, cand_gain,
                                                                      cand_bin, out_f, out_bin, out_gain, do_split,
                                                                      Lst, Rst, Tst);
  else
    split_node_kernel<double><<<dim3((unsigned)M), dim3(64), 0, s>>>((const double*)H, d, B, C, cand_gain, cand_bin,
                                                                    out_f, out_bin, out_gain, do_split, Lst, Rst,
                                                                    Tst);
  return harp_launch_status();
}

// nleft [M] (zeroed by the caller) += rows of each split node with Xb[row, f] <= bin
HARP_EXPORT int harp_forest_route_count(const uint8_t* Xb, int dpad, const int* order, const int* start,
                                        const int* cnt, const int* chunk_off, int M, int max_chunks,
                                        const int* do_split, const int* sf, const int* sbin, int* nleft,
                                        hipStream_t s) {
  if (M < 0 || max_chunks < 0 || dpad < 1) return HARP_EBADARG;
  if (M == 0 || max_chunks == 0) return HARP_OK;
  route_count_kernel<<<dim3((unsigned)max_chunks), dim3(256), 0, s>>>(Xb, dpad, order, start, cnt, chunk_off, M,
                                                                     do_split, sf, sbin, nleft);
  return harp_launch_status();
}

// new_order [new_len]: rows of every split node moved to its children's ranges; cursor
// [M, 2] zeroed by the caller.
HARP_EXPORT int harp_forest_route_scatter(const uint8_t* Xb, int dpad, const int* order, const int* start,
                                          const int* cnt, const int* chunk_off, int M, int max_chunks,
                                          const int* do_split, const int* sf, const int* sbin, const int* nleft,
                                          const int* child_start, int* cursor, int* new_order, long new_len,
                                          hipStream_t s) {
  if (M < 0 || max_chunks < 0 || dpad < 1 || new_len < 0) return HARP_EBADARG;
  if (M == 0 || max_chunks == 0) return HARP_OK;
  route_scatter_kernel<<<dim3((unsigned)max_chunks), dim3(256), 0, s>>>(Xb, dpad, order, start, cnt, chunk_off, M,
                                                                       do_split, sf, sbin, nleft, child_start, cursor,
                                                                       new_order, new_len);
  return harp_launch_status();
}

// Packed forest: feat / thr / left / value [N(, C)] concatenated over trees, off [ntrees + 1].
// `left` holds ids local to the tree (-1 = leaf). out [n, C] mean leaf value over trees (or
// null), leaf [ntrees, n] local leaf ids (or null). max_steps bounds the walk (depth + 1).
HARP_EXPORT int harp_forest_predict(const void* X, int is64, long n, int d, const int* feat, const double* thr,
                                    const int* left, const double* value, const long* off, int ntrees, int C,
                                    int max_steps, double* out, long* leaf, hipStream_t s) {
  if (n < 0 || d < 1 || ntrees < 1 || max_steps < 0 || (!out && !leaf)) return HARP_EBADARG;
  if (C < 1) return HARP_EBADARG;
  if (C > FOREST_MAX_CLASSES) return HARP_EUNSUPPORTED;
  if (n == 0) return HARP_OK;
  const long blocks = (n + 255) / 256;
  if (blocks > 0x7fffffffL) return HARP_EBADARG;
  const dim3 g((unsigned)blocks), b(256);
  if (is64)
    predict_kernel<double><<<g, b, 0, s>>>((const double*)X, n, d, feat, thr, left, value, off, ntrees, C, max_steps,
                                           out, leaf);
  else
    predict_kernel<float><<<g, b, 0, s>>>((const float*)X, n, d, feat, thr, left, value, off, ntrees, C, max_steps,
                                          out, leaf);
  return harp_launch_status();
}
