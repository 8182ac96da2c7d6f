// CSR statistics for gfx950, fp64 like the reference: sparse Gram (X^T X), per-column
// moments, per-class feature sums and a sparse-dense product with an optional fused argmax.
//
// Replaces the step-1 partials of the reference's csr applications (ml/daal/.../
// daal_cov/csrdistri, daal_mom/csrdistri, daal_pca/corcsrdistr, daal_naive/csrdistri) without
// ever forming the dense n x d block. Operands as in kmeans_csr.hip: rowptr int64 [n+1],
// col int32 [nnz] (sorted within a row, no duplicates), val fp64 [nnz].
//
// Gram, two paths (the host picks, ops/csr_stats.py):
//   * tiled: a workgroup owns one T x T tile (block row bi <= block column bj) of G in LDS
//     and a span of rows. blk [nb+1][n] (int32, feature-block-major so that 64 lanes read
//     64 consecutive rows in one 256-B load) holds, per row, the offset of the first
//     nonzero with col >= b*T, so the row's segment in a column block is two loads. A wave
//     takes 64 rows, one per lane: rows with at most SMALL products and a segment of at
//     most NC entries are finished by their own lane, that segment held in registers
//     (about one nonzero per block: no lane waits for a 63-lane-idle wave); the others are
//     then taken by the whole wave one after another, the shorter segment broadcast by
//     readlane and the lanes running over the longer one. Products are added with
//     ds_add_f64; at the end of the span the tile is added into G once, each wave
//     instruction 512 or 256 contiguous bytes of one G row (global_atomic_add_f64). The
//     kernel is bound by the latency of the row loads, hence 1024-thread workgroups.
//   * direct: every row's m(m+1)/2 products go straight to G with global atomics, LPR lanes
//     per row. No row is visited more than once: the choice for very sparse rows or many
//     tiles, where the tiled path's n * npairs row visits outweigh the products.
// Only the upper triangle (col_i <= col_j) is written; the caller mirrors it.
#include "common.h"

#define CSR_GRAM_TILE 96  // 96*96*8 = 72 KB of LDS: two workgroups per CU
#define CSR_MOM_LDS_MAX_D 1024  // 5 accumulators * 1024 * 8 = 40 KB
#define CSR_GRAM_SMALL 32  // products a lane finishes by itself

namespace {

constexpr int T = CSR_GRAM_TILE;
constexpr int NC = 8;  // entries of a row segment a lane keeps in registers

// unsorted or duplicated columns (the op layer rules them out) must not leave the tile
__device__ __forceinline__ bool in_tile(int ja, int jb) { return (unsigned)ja < (unsigned)T && (unsigned)jb < (unsigned)T; }

// blkT[b][r] = first position p (relative to rowptr[r]) with col[p] >= b*T, b = 0..nb
__global__ __launch_bounds__(256) void csr_block_offsets_kernel(const long* __restrict__ rowptr,
                                                                const int* __restrict__ col, long n, int nb,
                                                                int* __restrict__ blkT) {
  const long total = n * (long)(nb + 1);
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const long r = i % n;
    const int b = (int)(i / n);
    const long a = rowptr[r];
    const int m = (int)(rowptr[r + 1] - a);
    const int key = b * T;
    int lo = 0, hi = m;  // first index with col >= key
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (col[a + mid] < key) lo = mid + 1;
      else hi = mid;
    }
    blkT[i] = lo;
  }
}

__global__ __launch_bounds__(1024) void csr_gram_tiled_kernel(const long* __restrict__ rowptr,
                                                              const int* __restrict__ col,
                                                              const double* __restrict__ val, long n, int d, int nb,
                                                              const int* __restrict__ blkT, long rows_per_split,
                                                              double* __restrict__ G) {
  extern __shared__ double tile[];  // [T][T]
  // blockIdx.x -> (bi, bj) of the upper triangle, row-major
  int bi = 0, rem = (int)blockIdx.x;
  while (rem >= nb - bi) {
    rem -= nb - bi;
    ++bi;
  }
  const int bj = bi + rem;
  const bool diag = bi == bj;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nwave = blockDim.x >> 6;
  for (int i = threadIdx.x; i < T * T; i += blockDim.x) tile[i] = 0.0;
  __syncthreads();

  const long r0 = (long)blockIdx.y * rows_per_split;
  const long r1 = r0 + rows_per_split < n ? r0 + rows_per_split : n;
  const int* ba0 = blkT + (long)bi * n;
  const int* ba1 = ba0 + n;
  const int* bb0 = blkT + (long)bj * n;
  const int* bb1 = bb0 + n;
  const int ca = bi * T, cb = bj * T;
  for (long rb = r0 + 64L * wave; rb < r1; rb += 64L * nwave) {
    const long r = rb + lane;
    long pa = 0, pb = 0;
    int la = 0, lb = 0;
    if (r < r1) {
      const long a = rowptr[r];
      const int sa = ba0[r], sb = bb0[r];
      la = ba1[r] - sa;
      lb = bb1[r] - sb;
      pa = a + sa;
      pb = a + sb;
    }
    const int prod = la * lb;  // la, lb <= T
    // lane per row: the shorter segment (at most NC entries) is loaded once into registers,
    // so a row costs one load round trip per entry of the other segment, not per product
    const bool mine = prod > 0 && prod <= CSR_GRAM_SMALL && (la <= NC || lb <= NC);
    if (mine) {
      const bool sw = lb > NC;  // cache A instead of B
      const long pc = sw ? pa : pb, pl = sw ? pb : pa;
      const int lc = sw ? la : lb, ll = sw ? lb : la;
      const int cc = sw ? ca : cb, cl = sw ? cb : ca;
      int jc[NC];
      double vc[NC];
#pragma unroll
      for (int u = 0; u < NC; ++u) {
        const bool on = u < lc;
        jc[u] = on ? col[pc + u] - cc : -1;  // -1 is outside every tile
        vc[u] = on ? val[pc + u] : 0.0;
      }
      for (int p = 0; p < ll; ++p) {
        const int jl = col[pl + p] - cl;
        const double vl = val[pl + p];
#pragma unroll
        for (int u = 0; u < NC; ++u) {
          const int ja = sw ? jc[u] : jl, jb = sw ? jl : jc[u];
          if (in_tile(ja, jb) && (!diag || ja <= jb)) unsafeAtomicAdd(&tile[ja * T + jb], vc[u] * vl);
        }
      }
    }
    unsigned long long big = __ballot(prod > 0 && !mine);
    while (big) {
      const int t = __builtin_ctzll(big);
      big &= big - 1;
      const int wla = __builtin_amdgcn_readlane(la, t), wlb = __builtin_amdgcn_readlane(lb, t);
      const long wpa = ((long)__builtin_amdgcn_readlane((int)(pa >> 32), t) << 32) |
                       (unsigned)__builtin_amdgcn_readlane((int)pa, t);
      const long wpb = ((long)__builtin_amdgcn_readlane((int)(pb >> 32), t) << 32) |
                       (unsigned)__builtin_amdgcn_readlane((int)pb, t);
      // broadcast the shorter segment (S), lanes over the longer one (L)
      const bool sw = wla > wlb;
      const long ps = sw ? wpb : wpa, pl = sw ? wpa : wpb;
      const int ls = sw ? wlb : wla, ll = sw ? wla : wlb;
      const int cs = sw ? cb : ca, cl = sw ? ca : cb;
      for (int s0 = 0; s0 < ls; s0 += 64) {
        const int cnt = ls - s0 < 64 ? ls - s0 : 64;
        const int jsl = lane < cnt ? col[ps + s0 + lane] - cs : 0;
        const double vsl = lane < cnt ? val[ps + s0 + lane] : 0.0;
        for (int q0 = 0; q0 < ll; q0 += 64) {  // wave-uniform trip count: the readlanes see every lane
          const bool on = q0 + lane < ll;
          const int jl = on ? col[pl + q0 + lane] - cl : 0;
          const double vl = on ? val[pl + q0 + lane] : 0.0;
          for (int u = 0; u < cnt; ++u) {
            const int js = __builtin_amdgcn_readlane(jsl, u);
            const double vs = readlane_d(vsl, u);
            const int ja = sw ? jl : js, jb = sw ? js : jl;
            if (on && in_tile(ja, jb) && (!diag || ja <= jb)) unsafeAtomicAdd(&tile[ja * T + jb], vs * vl);
          }
        }
      }
    }
  }
  __syncthreads();
  // flush: wave w takes tile rows w, w + nwave, ...; lanes over 64 + 32 consecutive columns
  for (int i = wave; i < T; i += nwave) {
    const int gi = ca + i;
    if (gi >= d) break;
    double* grow = G + (long)gi * d + cb;
    for (int j = lane; j < T; j += 64) {
      const int gj = cb + j;
      if (gj < d && gj >= gi) {
        const double v = tile[i * T + j];
        if (v != 0.0) unsafeAtomicAdd(&grow[j], v);
      }
    }
  }
}

template <int LPR>
__global__ __launch_bounds__(256) void csr_gram_direct_kernel(const long* __restrict__ rowptr,
                                                              const int* __restrict__ col,
                                                              const double* __restrict__ val, long n, int d,
                                                              double* __restrict__ G) {
  const int sub = threadIdx.x % LPR;
  const long ng = ((long)gridDim.x * blockDim.x) / LPR;
  for (long r = ((long)blockIdx.x * blockDim.x + threadIdx.x) / LPR; r < n; r += ng) {
    const long a = rowptr[r], b = rowptr[r + 1];
    for (long p = a; p < b; ++p) {
      const double vp = val[p];
      double* grow = G + (long)col[p] * d;
      for (long q = p + sub; q < b; q += LPR) unsafeAtomicAdd(&grow[col[q]], vp * val[q]);  // col[q] >= col[p]
    }
  }
}

// out [5][d]: count, sum (v - c), sum (v - c)^2, min v, max v over the stored values
template <bool LDS>
__global__ __launch_bounds__(256) void csr_col_moments_kernel(const int* __restrict__ col,
                                                              const double* __restrict__ val, long nnz, int d,
                                                              const double* __restrict__ center,
                                                              double* __restrict__ out) {
  __shared__ double acc[LDS ? 5 * CSR_MOM_LDS_MAX_D : 1];
  double* cnt = LDS ? acc : out;
  double* s1 = cnt + d;
  double* s2 = s1 + d;
  double* mn = s2 + d;
  double* mx = mn + d;
  if (LDS) {
    for (int j = threadIdx.x; j < d; j += blockDim.x) {
      cnt[j] = 0.0;
      s1[j] = 0.0;
      s2[j] = 0.0;
      mn[j] = __builtin_inf();
      mx[j] = -__builtin_inf();
    }
    __syncthreads();
  }
  for (long p = (long)blockIdx.x * blockDim.x + threadIdx.x; p < nnz; p += (long)gridDim.x * blockDim.x) {
    const int j = col[p];
    const double v = val[p];
    const double c = v - center[j];
    unsafeAtomicAdd(&cnt[j], 1.0);
    unsafeAtomicAdd(&s1[j], c);
    unsafeAtomicAdd(&s2[j], c * c);
    atomicMin(&mn[j], v);
    atomicMax(&mx[j], v);
  }
  if (LDS) {
    __syncthreads();
    for (int j = threadIdx.x; j < d; j += blockDim.x) {
      if (cnt[j] > 0.0) {
        unsafeAtomicAdd(&out[j], cnt[j]);
        unsafeAtomicAdd(&out[d + j], s1[j]);
        unsafeAtomicAdd(&out[2 * d + j], s2[j]);
        atomicMin(&out[3 * d + j], mn[j]);
        atomicMax(&out[4 * d + j], mx[j]);
      }
    }
  }
}

__global__ __launch_bounds__(256) void csr_class_sums_kernel(const long* __restrict__ rowptr,
                                                             const int* __restrict__ col,
                                                             const double* __restrict__ val, long n, int d,
                                                             const int* __restrict__ y, int C,
                                                             double* __restrict__ sums, double* __restrict__ counts,
                                                             int* __restrict__ err) {
  const int lane = threadIdx.x & 63;
  const long nw = ((long)gridDim.x * blockDim.x) >> 6;
  for (long r = ((long)blockIdx.x * blockDim.x + threadIdx.x) >> 6; r < n; r += nw) {
    const int c = y[r];
    if (c < 0 || c >= C) {
      if (lane == 0) err[0] = 1;
      continue;
    }
    if (lane == 0) unsafeAtomicAdd(&counts[c], 1.0);
    double* srow = sums + (long)c * d;
    for (long p = rowptr[r] + lane; p < rowptr[r + 1]; p += 64) unsafeAtomicAdd(&srow[col[p]], val[p]);
  }
}

// out[r][c] = sum_p val[p] * BP[col[p]][c] + bias[c]; one wave per row, lanes over the
// output columns in KPL register slots (64 * KPL columns per pass, as kmeans_csr.hip)
template <int KPL>
__global__ __launch_bounds__(256) void csr_spmm_kernel(const long* __restrict__ rowptr, const int* __restrict__ col,
                                                       const double* __restrict__ val, long n,
                                                       const double* __restrict__ BP, int m, int mp,
                                                       const double* __restrict__ bias, double* __restrict__ out,
                                                       int* __restrict__ amax) {
  const int lane = threadIdx.x & 63;
  const long nw = ((long)gridDim.x * blockDim.x) >> 6;
  for (long r = ((long)blockIdx.x * blockDim.x + threadIdx.x) >> 6; r < n; r += nw) {
    const long a = rowptr[r], b = rowptr[r + 1];
    double best = -__builtin_inf();
    int besti = 0x7fffffff;
    for (int c0 = 0; c0 < m; c0 += 64 * KPL) {
      double acc[KPL];
#pragma unroll
      for (int i = 0; i < KPL; ++i) acc[i] = 0.0;
      for (long p0 = a; p0 < b; p0 += 64) {
        const int cnt = (int)((b - p0) < 64 ? (b - p0) : 64);
        const int jl = lane < cnt ? col[p0 + lane] : 0;
        const double vl = lane < cnt ? val[p0 + lane] : 0.0;
        for (int t = 0; t < cnt; ++t) {
          const int j = __builtin_amdgcn_readlane(jl, t);
          const double v = readlane_d(vl, t);
          const double* bp = BP + (long)j * mp + c0 + lane;
#pragma unroll
          for (int i = 0; i < KPL; ++i)
            if (c0 + 64 * i < mp) acc[i] = fma(v, bp[64 * i], acc[i]);
        }
      }
#pragma unroll
      for (int i = 0; i < KPL; ++i) {
        const int c = c0 + 64 * i + lane;
        if (c < m) {
          const double s = bias ? acc[i] + bias[c] : acc[i];
          if (out) out[r * (long)m + c] = s;
          if (s > best) {  // c increases with i: strict > keeps the lower index
            best = s;
            besti = c;
          }
        }
      }
    }
    if (amax) {
      wave_arg_xor<true>(best, besti);
      if (lane == 0) amax[r] = besti < m ? besti : 0;
    }
  }
}

long grid_for_waves(long n) {
  long blocks = (n + 3) / 4;
  return blocks > 65536 ? 65536 : (blocks < 1 ? 1 : blocks);
}

}  // namespace

HARP_EXPORT int harp_csr_gram_tile() { return CSR_GRAM_TILE; }
HARP_EXPORT int harp_csr_mom_lds_max_d() { return CSR_MOM_LDS_MAX_D; }

// blkT [nb + 1][n] int32, nb = ceil(d / T): per-row offsets of the feature blocks
HARP_EXPORT int harp_csr_block_offsets(const long* rowptr, const int* col, long n, int d, int* blkT,
                                       hipStream_t s) {
  if (n <= 0) return HARP_OK;
  if (d <= 0) return HARP_EBADARG;
  const int nb = (d + T - 1) / T;
  long blocks = (n * (long)(nb + 1) + 255) / 256;
  if (blocks > 65536) blocks = 65536;
  csr_block_offsets_kernel<<<dim3((unsigned)blocks), dim3(256), 0, s>>>(rowptr, col, n, nb, blkT);
  return harp_launch_status();
}

// ADDS the upper triangle of X^T X into G [d][d]. path 0: tiled (needs blkT and
// rows_per_split > 0, a multiple of 64), path 1: direct (lanes_per_row 8 or 64).
HARP_EXPORT int harp_csr_gram(const long* rowptr, const int* col, const double* val, long n, int d,
                              const int* blkT, int path, long rows_per_split, int lanes_per_row, double* G,
                              hipStream_t s) {
  if (n <= 0) return HARP_OK;
  if (d <= 0) return HARP_EBADARG;
  if (path == 1) {
    if (lanes_per_row == 8) {
      long blocks = (n + 31) / 32;
      if (blocks > 65536) blocks = 65536;
      csr_gram_direct_kernel<8><<<dim3((unsigned)blocks), dim3(256), 0, s>>>(rowptr, col, val, n, d, G);
    } else if (lanes_per_row == 64) {
      csr_gram_direct_kernel<64><<<dim3((unsigned)grid_for_waves(n)), dim3(256), 0, s>>>(rowptr, col, val, n, d, G);
    } else {
      return HARP_EBADARG;
    }
    return harp_launch_status();
  }
  if (path != 0 || !blkT || rows_per_split <= 0 || (rows_per_split & 63)) return HARP_EBADARG;
  const long nb = (d + T - 1) / T;
  const long npairs = nb * (nb + 1) / 2;
  const long nsplit = (n + rows_per_split - 1) / rows_per_split;
  if (npairs > 0x7fffffffL || nsplit > 65535) return HARP_EUNSUPPORTED;
  const int lds = T * T * (int)sizeof(double);
  if (hipFuncSetAttribute((const void*)csr_gram_tiled_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, lds) !=
      hipSuccess)
    return HARP_ELAUNCH;
  // 1024 threads: with two workgroups per CU that is 8 waves per SIMD to hide the row loads
  csr_gram_tiled_kernel<<<dim3((unsigned)npairs, (unsigned)nsplit), dim3(1024), lds, s>>>(
      rowptr, col, val, n, d, (int)nb, blkT, rows_per_split, G);
  return harp_launch_status();
}

// ACCUMULATES into out [5][d] = count, sum (v - c), sum (v - c)^2, min v, max v per column
// over the stored values; the caller starts it at (0, 0, 0, +inf, -inf).
HARP_EXPORT int harp_csr_col_moments(const int* col, const double* val, long nnz, int d, const double* center,
                                     double* out, hipStream_t s) {
  if (nnz <= 0) return HARP_OK;
  if (d <= 0) return HARP_EBADARG;
  long blocks = (nnz + 256 * 16 - 1) / (256 * 16);
  if (blocks > 1024) blocks = 1024;
  if (d <= CSR_MOM_LDS_MAX_D)
    csr_col_moments_kernel<true><<<dim3((unsigned)blocks), dim3(256), 0, s>>>(col, val, nnz, d, center, out);
  else
    csr_col_moments_kernel<false><<<dim3((unsigned)blocks), dim3(256), 0, s>>>(col, val, nnz, d, center, out);
  return harp_launch_status();
}

// sums [C][d] += rows by class y (int32 [n]), counts [C] += 1; err[0] = 1 if a label is
// outside [0, C) (that row is skipped)
HARP_EXPORT int harp_csr_class_sums(const long* rowptr, const int* col, const double* val, long n, int d,
                                    const int* y, int C, double* sums, double* counts, int* err, hipStream_t s) {
  if (n <= 0) return HARP_OK;
  if (d <= 0 || C <= 0) return HARP_EBADARG;
  csr_class_sums_kernel<<<dim3((unsigned)grid_for_waves(n)), dim3(256), 0, s>>>(rowptr, col, val, n, d, y, C, sums,
                                                                              counts, err);
  return harp_launch_status();
}

// out [n][m] (may be null) = X BP[:, :m] + bias (may be null), BP [d][mp] (mp >= m, a
// multiple of 64); amax [n] (may be null) = per-row argmax, ties to the lowest column
HARP_EXPORT int harp_csr_spmm(const long* rowptr, const int* col, const double* val, long n, const double* BP,
                              int m, int mp, const double* bias, double* out, int* amax, hipStream_t s) {
  if (n <= 0) return HARP_OK;
  if (m <= 0 || mp < m || (mp & 63) || (!out && !amax)) return HARP_EBADARG;
  const dim3 g((unsigned)grid_for_waves(n)), bl(256);
  if (mp <= 64) csr_spmm_kernel<1><<<g, bl, 0, s>>>(rowptr, col, val, n, BP, m, mp, bias, out, amax);
  else if (mp <= 128) csr_spmm_kernel<2><<<g, bl, 0, s>>>(rowptr, col, val, n, BP, m, mp, bias, out, amax);
  else if (mp <= 256) csr_spmm_kernel<4><<<g, bl, 0, s>>>(rowptr, col, val, n, BP, m, mp, bias, out, amax);
  else if (mp <= 512) csr_spmm_kernel<8><<<g, bl, 0, s>>>(rowptr, col, val, n, BP, m, mp, bias, out, amax);
  else csr_spmm_kernel<16><<<g, bl, 0, s>>>(rowptr, col, val, n, BP, m, mp, bias, out, amax);
  return harp_launch_status();
}
