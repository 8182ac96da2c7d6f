// Apriori support counting for gfx950 on vertical bitmaps: one row of bits per item, one bit
// per local transaction (bit t of item i = word t >> 5, bit t & 31 of row i). Rows are W
// 32-bit words long, W a multiple of 4 (16 bytes), padding bits zero, so every row is read
// with 16-byte loads and every support is a popcount of ANDed rows. Counts are int32 (a rank
// holds fewer than 2^31 transactions); every cross-workgroup merge is an integer atomicAdd,
// so the results do not depend on the arrival order.
//
// Replaces the dense incidence matrix of the DAAL association_rules batch application
// (ml/daal/.../daal_ar): nothing here or in ops/apriori.py forms an n x items array.
//
//   pack      (tid, item) pairs -> bitmaps with atomicOr (a duplicated pair sets its bit twice)
//   popcount  per-row popcount: the level-1 supports
//   pairs     S[a][b] = sum_w popc(B[idx[a]][w] & B[idx[b]][w]) for a <= b, a bit "GEMM": a
//             workgroup owns one upper-triangular TI x TI tile of items and one slab of words,
//             stages KW-word pieces of both item tiles in LDS, each thread a 4 x 4 register
//             tile of counters; slabs are merged with atomicAdd
//   count     level-k candidates in runs that share their first k-1 items: a workgroup takes
//             one (run, word slab), ANDs the k-1 prefix rows once per word into registers and
//             counts every extension row against them; words whose prefix AND is zero are
//             skipped, and a workgroup whose whole slab is zero returns at once
//   prune     Apriori property: binary search of every (k-1)-subset that drops one of the
//             first k-2 positions in the sorted large (k-1)-itemsets
#include "common.h"

#define APRIORI_PAIR_TILE 64   // items per side of a pair tile
#define APRIORI_PAIR_KW 32     // words of a row staged per step
#define APRIORI_EXT_CAP 64     // extensions (candidates) of one count workgroup
#define APRIORI_MAX_K 64       // longest itemset the count / prune kernels take
#define APRIORI_SLAB4 1024     // 16-byte words of a count slab: 4 per thread

namespace {

constexpr int TI = APRIORI_PAIR_TILE;
constexpr int KW = APRIORI_PAIR_KW;
constexpr int LDW = KW + 4;  // LDS row stride in words: 16 rows x 36 words hit 16 distinct 16-B slots
constexpr int CP = APRIORI_SLAB4 / 256;

__device__ __forceinline__ int popc4(uint4 v) { return __popc(v.x) + __popc(v.y) + __popc(v.z) + __popc(v.w); }
__device__ __forceinline__ uint4 and4(uint4 a, uint4 b) { return make_uint4(a.x & b.x, a.y & b.y, a.z & b.z, a.w & b.w); }

__global__ __launch_bounds__(256) void apriori_pack_kernel(const int* __restrict__ tid, const int* __restrict__ item,
                                                           long npairs, int n, int n_items, long W,
                                                           unsigned* __restrict__ bits, int* __restrict__ err) {
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < npairs; i += (long)gridDim.x * blockDim.x) {
    const int t = tid[i], it = item[i];
    if ((unsigned)t >= (unsigned)n || (unsigned)it >= (unsigned)n_items) {
      *err = 1;
      continue;
    }
    atomicOr(&bits[(long)it * W + (t >> 5)], 1u << (t & 31));
  }
}

// one workgroup per row
__global__ __launch_bounds__(256) void apriori_popcount_kernel(const unsigned* __restrict__ bits, long W,
                                                               int* __restrict__ out) {
  __shared__ int red[4];
  const uint4* row = reinterpret_cast<const uint4*>(bits + (long)blockIdx.x * W);
  const long W4 = W >> 2;
  int c = 0;
  for (long w = threadIdx.x; w < W4; w += 256) c += popc4(row[w]);
  c = wave_sum_i(c);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = c;
  __syncthreads();
  if (threadIdx.x == 0) out[blockIdx.x] = red[0] + red[1] + red[2] + red[3];
}

// grid.x = upper-triangular tile pairs (bi <= bj), grid.y = word slabs of slab_words (a
// multiple of KW). Thread (ty, tx) owns items a = bi*TI + 16 i + ty, b = bj*TI + 16 j + tx.
__global__ __launch_bounds__(256) void apriori_pairs_kernel(const unsigned* __restrict__ bits, const int* __restrict__ idx,
                                                            int m, long W, long slab_words, int* __restrict__ S) {
  __shared__ __attribute__((aligned(16))) unsigned sA[TI * LDW];
  __shared__ __attribute__((aligned(16))) unsigned sB[TI * LDW];
  int bi = 0, rem = blockIdx.x;
  const int nt = (m + TI - 1) / TI;
  while (rem >= nt - bi) {
    rem -= nt - bi;
    ++bi;
  }
  const int bj = bi + rem;
  const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
  const long w0 = (long)blockIdx.y * slab_words;
  const long w1 = min(w0 + slab_words, W);

  // staging: thread -> (row, 16-byte piece) of each tile, two rows per thread
  const int sp = threadIdx.x & 7, sr = threadIdx.x >> 3;  // piece 0..7, row 0..31 (+32)
  const uint4* rowA[2];
  const uint4* rowB[2];
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const int a = bi * TI + sr + 32 * h, b = bj * TI + sr + 32 * h;
    rowA[h] = a < m ? reinterpret_cast<const uint4*>(bits + (long)idx[a] * W) : nullptr;
    rowB[h] = b < m ? reinterpret_cast<const uint4*>(bits + (long)idx[b] * W) : nullptr;
  }

  int acc[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = 0;

  const uint4 zero = make_uint4(0, 0, 0, 0);
  for (long w = w0; w < w1; w += KW) {
    const long wp = w + 4 * sp;  // W and w are multiples of 4: a piece is inside the row or outside it
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const uint4 va = (rowA[h] && wp < w1) ? rowA[h][wp >> 2] : zero;
      const uint4 vb = (rowB[h] && wp < w1) ? rowB[h][wp >> 2] : zero;
      *reinterpret_cast<uint4*>(&sA[(sr + 32 * h) * LDW + 4 * sp]) = va;
      *reinterpret_cast<uint4*>(&sB[(sr + 32 * h) * LDW + 4 * sp]) = vb;
    }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < KW / 4; ++q) {
      uint4 a[4], b[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) a[i] = *reinterpret_cast<const uint4*>(&sA[(16 * i + ty) * LDW + 4 * q]);
#pragma unroll
      for (int j = 0; j < 4; ++j) b[j] = *reinterpret_cast<const uint4*>(&sB[(16 * j + tx) * LDW + 4 * q]);
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] += popc4(and4(a[i], b[j]));
    }
    __syncthreads();
  }
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int a = bi * TI + 16 * i + ty, b = bj * TI + 16 * j + tx;
      if (a < m && b < m && a <= b && acc[i][j]) atomicAdd(&S[(long)a * m + b], acc[i][j]);
    }
}

// grid.x = runs, grid.y = word slabs of slab4 <= APRIORI_SLAB4 16-byte words. A run is
// cand[group_off[g] .. group_off[g+1]) (at most APRIORI_EXT_CAP rows of k items), all with the
// first k-1 items of its first row.
__global__ __launch_bounds__(256) void apriori_count_kernel(const unsigned* __restrict__ bits, const int* __restrict__ cand,
                                                            const int* __restrict__ group_off, int k, long W,
                                                            int slab4, int* __restrict__ out) {
  __shared__ int s_pre[APRIORI_MAX_K];
  __shared__ int s_ext[APRIORI_EXT_CAP];
  __shared__ int s_cnt[APRIORI_EXT_CAP];
  const int c0 = group_off[blockIdx.x];
  const int ne = min(group_off[blockIdx.x + 1] - c0, APRIORI_EXT_CAP);
  if (ne <= 0) return;
  if (threadIdx.x < k - 1) s_pre[threadIdx.x] = cand[(long)c0 * k + threadIdx.x];
  if (threadIdx.x < ne) {
    s_ext[threadIdx.x] = cand[(long)(c0 + threadIdx.x) * k + (k - 1)];
    s_cnt[threadIdx.x] = 0;
  }
  __syncthreads();
  const long W4 = W >> 2;
  const long base = (long)blockIdx.y * slab4;
  const long end = min(base + slab4, W4);

  uint4 pre[CP];
  int any = 0;
#pragma unroll
  for (int p = 0; p < CP; ++p) {
    const long w = base + threadIdx.x + 256 * p;
    uint4 v = make_uint4(0, 0, 0, 0);
    if (w < end) {
      v = reinterpret_cast<const uint4*>(bits + (long)s_pre[0] * W)[w];
      for (int j = 1; j < k - 1; ++j) v = and4(v, reinterpret_cast<const uint4*>(bits + (long)s_pre[j] * W)[w]);
    }
    pre[p] = v;
    any |= (v.x | v.y | v.z | v.w) != 0;
  }
  if (!__syncthreads_or(any)) return;  // the prefix occurs nowhere in this slab

  for (int e = 0; e < ne; ++e) {
    const uint4* row = reinterpret_cast<const uint4*>(bits + (long)s_ext[e] * W);
    int c = 0;
#pragma unroll
    for (int p = 0; p < CP; ++p) {
      const uint4 v = pre[p];
      if (v.x | v.y | v.z | v.w) c += popc4(and4(v, row[base + threadIdx.x + 256 * p]));
    }
    c = wave_sum_i(c);
    if ((threadIdx.x & 63) == 0 && c) atomicAdd(&s_cnt[e], c);
  }
  __syncthreads();
  if (threadIdx.x < ne && s_cnt[threadIdx.x]) atomicAdd(&out[c0 + threadIdx.x], s_cnt[threadIdx.x]);
}

// -1 / 0 / +1: row p (k-1 items) against candidate c with position drop left out
__device__ __forceinline__ int cmp_subset(const int* __restrict__ p, const int* __restrict__ c, int k, int drop) {
  for (int j = 0; j < k - 1; ++j) {
    const int x = p[j], y = c[j + (j >= drop)];
    if (x != y) return x < y ? -1 : 1;
  }
  return 0;
}

__global__ __launch_bounds__(256) void apriori_prune_kernel(const int* __restrict__ cand, long c, int k,
                                                            const int* __restrict__ prev, long m,
                                                            unsigned char* __restrict__ keep) {
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < c; i += (long)gridDim.x * blockDim.x) {
    const int* ci = cand + i * k;
    bool ok = true;
    for (int drop = 0; drop < k - 2 && ok; ++drop) {
      long lo = 0, hi = m;  // first row >= the subset
      while (lo < hi) {
        const long mid = (lo + hi) >> 1;
        if (cmp_subset(prev + mid * (k - 1), ci, k, drop) < 0) lo = mid + 1;
        else hi = mid;
      }
      ok = lo < m && cmp_subset(prev + lo * (k - 1), ci, k, drop) == 0;
    }
    keep[i] = ok ? 1 : 0;
  }
}

unsigned grid_for(long items, int per_block) {
  long blocks = (items + per_block - 1) / per_block;
  if (blocks > 65536) blocks = 65536;
  return (unsigned)(blocks < 1 ? 1 : blocks);
}

}  // namespace

HARP_EXPORT int harp_apriori_pair_tile() { return APRIORI_PAIR_TILE; }
HARP_EXPORT int harp_apriori_pair_kw() { return APRIORI_PAIR_KW; }
HARP_EXPORT int harp_apriori_ext_cap() { return APRIORI_EXT_CAP; }
HARP_EXPORT int harp_apriori_max_k() { return APRIORI_MAX_K; }
HARP_EXPORT int harp_apriori_slab4() { return APRIORI_SLAB4; }

// ORs the pairs into bits [n_items][W] (uint32 words, W a multiple of 4, W * 32 >= n);
// err[0] = 1 if a tid is outside [0, n) or an item outside [0, n_items) (that pair is skipped)
HARP_EXPORT int harp_apriori_pack(const int* tid, const int* item, long npairs, int n, int n_items, long W,
                                  unsigned* bits, int* err, hipStream_t s) {
  if (npairs <= 0) return HARP_OK;
  if (n <= 0 || n_items <= 0 || (W & 3) || W * 32 < n) return HARP_EBADARG;
  apriori_pack_kernel<<<dim3(grid_for(npairs, 256)), dim3(256), 0, s>>>(tid, item, npairs, n, n_items, W, bits, err);
  return harp_launch_status();
}

// out [rows] = popcount of every row of bits [rows][W]
HARP_EXPORT int harp_apriori_popcount(const unsigned* bits, int rows, long W, int* out, hipStream_t s) {
  if (rows <= 0) return HARP_OK;
  if (W <= 0 || (W & 3)) return HARP_EBADARG;
  apriori_popcount_kernel<<<dim3((unsigned)rows), dim3(256), 0, s>>>(bits, W, out);
  return harp_launch_status();
}

// ADDS the supports of all pairs (a <= b) of the rows idx [m] into S [m][m]; slab_words: words
// of a row per workgroup, a multiple of APRIORI_PAIR_KW
HARP_EXPORT int harp_apriori_pairs(const unsigned* bits, const int* idx, int m, long W, long slab_words, int* S,
                                   hipStream_t s) {
  if (m <= 0) return HARP_OK;
  if (W <= 0 || (W & 3) || slab_words <= 0 || slab_words % APRIORI_PAIR_KW) return HARP_EBADARG;
  const long nt = (m + TI - 1) / TI;
  const long tiles = nt * (nt + 1) / 2;
  const long slabs = (W + slab_words - 1) / slab_words;
  if (tiles > 0x7fffffffL || slabs > 65535) return HARP_EUNSUPPORTED;
  apriori_pairs_kernel<<<dim3((unsigned)tiles, (unsigned)slabs), dim3(256), 0, s>>>(bits, idx, m, W, slab_words, S);
  return harp_launch_status();
}

// ADDS the supports of cand [c][k] (item rows of bits) into out [c]; group_off [g + 1] bounds
// runs of at most APRIORI_EXT_CAP candidates that share their first k-1 items; slab4: 16-byte
// words of a row per workgroup, at most APRIORI_SLAB4
HARP_EXPORT int harp_apriori_count(const unsigned* bits, const int* cand, const int* group_off, int g, int k, long W,
                                   int slab4, int* out, hipStream_t s) {
  if (g <= 0) return HARP_OK;
  if (k < 2 || W <= 0 || (W & 3) || slab4 <= 0 || slab4 > APRIORI_SLAB4) return HARP_EBADARG;
  if (k > APRIORI_MAX_K) return HARP_EUNSUPPORTED;
  const long slabs = ((W >> 2) + slab4 - 1) / slab4;
  if (slabs > 65535) return HARP_EUNSUPPORTED;
  apriori_count_kernel<<<dim3((unsigned)g, (unsigned)slabs), dim3(256), 0, s>>>(bits, cand, group_off, k, W, slab4, out);
  return harp_launch_status();
}

// keep [c] = 1 where every (k-1)-subset of cand [c][k] that drops one of its first k-2 items is
// a row of prev [m][k-1] (sorted lexicographically)
HARP_EXPORT int harp_apriori_prune(const int* cand, long c, int k, const int* prev, long m, unsigned char* keep,
                                   hipStream_t s) {
  if (c <= 0) return HARP_OK;
  if (k < 2) return HARP_EBADARG;
  apriori_prune_kernel<<<dim3(grid_for(c, 256)), dim3(256), 0, s>>>(cand, c, k, prev, m, keep);
  return harp_launch_status();
}
