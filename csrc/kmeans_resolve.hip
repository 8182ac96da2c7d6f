// K-means: index resolve fused into the bucketed gather-sum (the second half of the keyless
// assign, kmeans.hip variant 16).
//
// The keyless sweep leaves labels[p] = the winning 32-row centroid group of point p.
// harp_bucket_labels_spans sorts the points by (span, group id): a span is a range of
// consecutive point indices, and bucket q = span * NG + group. Spans are an ordering of the
// sort, not launches: one launch walks the whole sorted permutation. It writes no label: a
// 4-byte store to labels[perm[j]] leaves the L2 as a 32-byte write of its own (97 M of them per
// 1e8 points, 1.6 ms; profiles/kmeans_tail_onepass). The row found goes to rowof[j] in sorted
// order instead, and kmeans_finish_labels_kernel streams over the points afterwards:
// labels[p] = 32 labels[p] + rowof[rank[p]], rank being the inverse permutation the sort
// writes on its way. That byte gather stays inside the point's span of rowof. Per window of
// 32 sorted points the resolve pass does everything that needs the point's row:
//  * lane (c, h) loads 16-B chunks 2s + h of point perm[j + c]: the MFMA B fragment, and the
//    same two 128-B lines per row that the plain gather-sum fetches;
//  * one KS-MFMA chain from a zero accumulator against the group's 32 centroid rows (A
//    fragment straight from Cm2, reloaded only when the group changes) re-computes the 32
//    candidate distances of every point of the window: the bits the sweep saw (same
//    operands, same k order);
//  * a plain first-occurrence argmin over the 16 registers and the lane <-> lane + 32
//    exchange give the row (ties: the lowest row), stored as one byte per point;
//  * the (x, 1) sums of the group's 32 rows are a second small GEMM on the same window,
//    S[row][col] += onehot[row][point] * X[point][col]: the one-hot A fragment is built from
//    the rows just found, the B fragment is the window's rows read back transposed from a
//    per-wave LDS copy, and S (32 rows x dp columns, fp32) lives in MFMA accumulators. No
//    atomics and no read-modify-write chains inside the run (a per-wave LDS table updated
//    with ds_add_f32 from the point lanes measured 57 ms for this pass, profiles/r7_keyless);
//  * S is flushed to sums with fp32 atomic row segments when the bucket changes and at the
//    end of the wave's run, as the plain gather-sum does at bucket boundaries.
// Every wave owns a fixed run of the sorted permutation, so the work is balanced for any
// skew; windows are fixed 32-entry pieces of the run, and a bucket boundary inside a window
// (a change of group, or of span with the group unchanged) is handled by one masked pass per
// bucket present. The next window's rows and the one after's permutation entries are in
// flight under the current window's work; only that prefetch and S stay in registers (the
// window and the group's A fragments sit in LDS), which keeps the pass at three waves per SIMD.
#include "common.h"

namespace {

constexpr int KR_RUN = 2048;  // sorted entries per wave (one wave per workgroup)

template <int KS>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(3))) void kmeans_resolve_rowsum_kernel(
    const __bf16* __restrict__ X, long ldx, const __bf16* __restrict__ Cm2, const int* __restrict__ perm,
    const int* __restrict__ start, int NG, int NB, long n, unsigned char* __restrict__ rowof,
    float* __restrict__ sums, int ld) {
  constexpr int DP = KS * 16;
  constexpr int NCB = (DP + 31) / 32;   // 32-column blocks of the sums GEMM
  // LDS copy of the window, [32 points][NCB * 32 columns] bf16 at a row stride of an odd
  // number of 16-B slots: the 16 rows of a ds_write_b128 lane group fall on 16 distinct slots
  constexpr int STRE = NCB * 32 + 8;    // row stride in elements
  __shared__ __attribute__((aligned(16))) __bf16 tile[32 * STRE];
  __shared__ bf16x8 atile[KS * 64];
  const int lane = threadIdx.x;
  const int c = lane & 31, h = lane >> 5;
  const long j0 = (long)blockIdx.x * KR_RUN;
  if (j0 >= n) return;
  const long j1 = j0 + KR_RUN < n ? j0 + KR_RUN : n;

  // columns past DP are never written by the windows: zero them once (they only feed the
  // unused columns of the last block, which are never flushed)
  for (int i = lane; i < 32 * STRE; i += 64) tile[i] = (__bf16)0.f;
  // bucket containing j0: last k with start[k] <= j0; its group is k % NG
  int lo = 0, hi = NB;
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (start[mid] <= j0) lo = mid; else hi = mid;
  }
  int k = lo;
  long kend = start[k + 1];
  int g = k % NG;
  int gloaded = -1;
  bool dirty = false;
  floatx16 S[NCB];
#pragma unroll
  for (int b = 0; b < NCB; ++b)
#pragma unroll
    for (int q = 0; q < 16; ++q) S[b][q] = 0.f;

  // sorted position of this lane's point in the window at jb, clamped into the run (masked
  // out when clamped)
  auto pos = [&](long jb) {
    const long j = jb + c;
    return j < j1 ? j : j1 - 1;
  };
  auto load_rows = [&](bf16x8 (&xf)[KS], int p) {
    const bf16x8* row = (const bf16x8*)(X + (long)p * ldx);
#pragma unroll
    for (int s = 0; s < KS; ++s) xf[s] = row[2 * s + h];
  };
  // S register q of lane half h holds row (q & 3) + 8 (q >> 2) + 4 h, column 32 b + c
  auto flush = [&](int gg) {
    float* o = sums + ((long)gg * 32 + 4 * h) * ld + c;  // the lane's part; the rest is uniform
#pragma unroll
    for (int b = 0; b < NCB; ++b) {
#pragma unroll
      for (int q = 0; q < 16; ++q) {
        const int rq = (q & 3) + 8 * (q >> 2);
        if (32 * b + c < DP && S[b][q] != 0.f) atomicAdd(o + (long)rq * ld + 32 * b, S[b][q]);
        S[b][q] = 0.f;
      }
    }
  };

  // xp: the rows of the next window, in flight from global while the current one (copied to
  // LDS on arrival) is worked on; both MFMA uses of a window read it back from that copy
  bf16x8 xp[KS];
  load_rows(xp, perm[pos(j0)]);
  int pn = perm[pos(j0 + 32)];

  for (long jb = j0; jb < j1; jb += 32) {
    const long je = jb + 32 < j1 ? jb + 32 : j1;
    const long jj = jb + c;
    __syncthreads();  // the previous window's reads of the copy are done
#pragma unroll
    for (int s = 0; s < KS; ++s) *(bf16x8*)(tile + c * STRE + (2 * s + h) * 8) = xp[s];
    // next window's rows (its permutation entries arrived during the previous window) and the
    // permutation entries of the window after it
    if (jb + 32 < j1) load_rows(xp, pn);
    pn = perm[pos(jb + 64)];
    __syncthreads();
    long cur = jb;
    while (cur < je) {
      if (cur >= kend) {  // into the next non-empty bucket
        if (dirty) {
          flush(g);
          dirty = false;
        }
        do {
          ++k;
          kend = start[k + 1];
        } while (cur >= kend);
        g = k % NG;
      }
      if (g != gloaded) {
        // the group's A fragments, parked in LDS (every lane reads back what it wrote)
        const bf16x8* arow = (const bf16x8*)(Cm2 + ((long)g * 32 + c) * DP);
#pragma unroll
        for (int s = 0; s < KS; ++s) atile[s * 64 + lane] = arow[2 * s + h];
        gloaded = g;
      }
      const long sub_end = kend < je ? kend : je;
      const bool mine = jj >= cur && jj < sub_end;
      floatx16 acc = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int s = 0; s < KS; ++s) {
        acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(atile[s * 64 + lane],
                                                      *(const bf16x8*)(tile + c * STRE + (2 * s + h) * 8), acc, 0, 0, 0);
        __builtin_amdgcn_sched_barrier(0);
      }
      // register q of lane half h is centroid row (q & 3) + 8 (q >> 2) + 4 h: ascending in q
      float m = acc[0];
      int mq = 0;
#pragma unroll
      for (int q = 1; q < 16; ++q)
        if (acc[q] < m) {
          m = acc[q];
          mq = q;
        }
      int row = (mq & 3) + 8 * (mq >> 2) + 4 * h;
      const float om = __shfl_xor(m, 32, 64);
      const int orow = __shfl_xor(row, 32, 64);
      if (om < m || (om == m && orow < row)) row = orow;
      if (mine && h == 0) rowof[jj] = (unsigned char)row;  // sorted order: one 32-byte store per window
      // sums: S[row][col] += onehot[row][point] * X[point][col], points on the MFMA k axis
      const int code = mine ? row : -1;
#pragma unroll
      for (int t = 0; t < 2; ++t) {
        bf16x8 oh;
#pragma unroll
        for (int j = 0; j < 8; ++j) {  // point 16 t + 8 h + j: both halves' codes as scalars
          const int r0 = __builtin_amdgcn_readlane(code, 16 * t + j), r1 = __builtin_amdgcn_readlane(code, 16 * t + 8 + j);
          oh[j] = (__bf16)((h ? r1 : r0) == c ? 1.f : 0.f);
        }
        const __bf16* tp = tile + (16 * t + 8 * h) * STRE + c;
#pragma unroll
        for (int b = 0; b < NCB; ++b) {
          bf16x8 xt;
#pragma unroll
          for (int j = 0; j < 8; ++j) xt[j] = tp[j * STRE + 32 * b];
          S[b] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(oh, xt, S[b], 0, 0, 0);
          __builtin_amdgcn_sched_barrier(0);
        }
      }
      dirty = true;
      cur = sub_end;
    }
  }
  if (dirty) flush(g);
}

template <int KS>
int launch_resolve(const void* X, long ldx, const void* Cm2, const int* perm, const int* start, int NG, int NB,
                   long n, unsigned char* rowof, float* sums, int ld, hipStream_t s) {
  const long nblk = (n + KR_RUN - 1) / KR_RUN;
  kmeans_resolve_rowsum_kernel<KS><<<dim3((unsigned)nblk), dim3(64), 0, s>>>(
      (const __bf16*)X, ldx, (const __bf16*)Cm2, perm, start, NG, NB, n, rowof, sums, ld);
  return harp_launch_status();
}

// labels[p] = 32 labels[p] + rowof[rank[p]], in place: the sweep's group id is still in
// labels[p] (bucketing only reads it), rank[p] is the point's sorted position and rowof the
// rows the resolve pass found, in sorted order. Four points per thread; the byte gather stays
// inside the point's span of the sort (span bytes of rowof), which the caches hold or nearly so.
template <bool VEC>
__global__ __launch_bounds__(256) void kmeans_finish_labels_kernel(int* __restrict__ labels,
                                                                   const int* __restrict__ rank,
                                                                   const unsigned char* __restrict__ rowof, long n) {
  const long p = ((long)blockIdx.x * 256 + threadIdx.x) * 4;
  if (p >= n) return;
  if (VEC && p + 4 <= n) {
    const int4 r = *(const int4*)(rank + p);
    int4 l = *(const int4*)(labels + p);
    l.x = 32 * l.x + rowof[r.x];
    l.y = 32 * l.y + rowof[r.y];
    l.z = 32 * l.z + rowof[r.z];
    l.w = 32 * l.w + rowof[r.w];
    *(int4*)(labels + p) = l;
  } else {
    const long e = p + 4 < n ? p + 4 : n;
    for (long i = p; i < e; ++i) labels[i] = 32 * labels[i] + rowof[rank[i]];
  }
}

}  // namespace

HARP_EXPORT int harp_kmeans_finish_labels(int* labels, const int* rank, const unsigned char* rowof, long n,
                                          hipStream_t s) {
  if (n <= 0) return n == 0 ? HARP_OK : HARP_EBADARG;
  if (!labels || !rank || !rowof || n >= (1L << 31)) return HARP_EBADARG;
  const dim3 grid((unsigned)((n + 1023) / 1024));
  if ((((uintptr_t)labels | (uintptr_t)rank) & 15) == 0)
    kmeans_finish_labels_kernel<true><<<grid, dim3(256), 0, s>>>(labels, rank, rowof, n);
  else
    kmeans_finish_labels_kernel<false><<<grid, dim3(256), 0, s>>>(labels, rank, rowof, n);
  return harp_launch_status();
}

// rowof[j] = argmin row (0..31) of point perm[j] inside group g = q % NG for j in [start[q],
// start[q+1]), and sums[32 g + row][0..dp) += the point's row (sums zeroed by the caller, ld >= dp).
// harp_kmeans_finish_labels turns the group ids and rowof into the final labels. X rows of dp
// elements (dp % 16 == 0, dp <= 128) at a stride of ldx; Cm2 [>= 32 NG][dp] contiguous;
// perm / start[nspans * NG + 1] from harp_bucket_labels_spans over the NG group ids (or, with
// nspans = 1, from harp_bucket_labels). One launch for all n.
HARP_EXPORT int harp_kmeans_resolve_rowsum(const void* X, long ldx, const void* Cm2, int dp, const int* perm,
                                           const int* start, int NG, int nspans, long n, unsigned char* rowof,
                                           float* sums, int ld, hipStream_t s) {
  if (n <= 0) return n == 0 ? HARP_OK : HARP_EBADARG;
  if (dp <= 0 || dp % 16 || dp > 128 || ldx < dp || ldx % 8 || ld < dp || NG <= 0 || nspans <= 0 ||
      (long)nspans * NG >= (1L << 30) || n >= (1L << 31) || !rowof || !sums)
    return HARP_EBADARG;
  const int NB = nspans * NG;
  switch (dp / 16) {
    case 1: return launch_resolve<1>(X, ldx, Cm2, perm, start, NG, NB, n, rowof, sums, ld, s);
    case 2: return launch_resolve<2>(X, ldx, Cm2, perm, start, NG, NB, n, rowof, sums, ld, s);
    case 3: return launch_resolve<3>(X, ldx, Cm2, perm, start, NG, NB, n, rowof, sums, ld, s);
    case 4: return launch_resolve<4>(X, ldx, Cm2, perm, start, NG, NB, n, rowof, sums, ld, s);
    case 5: return launch_resolve<5>(X, ldx, Cm2, perm, start, NG, NB, n, rowof, sums, ld, s);
    case 6: return launch_resolve<6>(X, ldx, Cm2, perm, start, NG, NB, n, rowof, sums, ld, s);
    case 7: return launch_resolve<7>(X, ldx, Cm2, perm, start, NG, NB, n, rowof, sums, ld, s);
    case 8: return launch_resolve<8>(X, ldx, Cm2, perm, start, NG, NB, n, rowof, sums, ld, s);
    default: return HARP_EUNSUPPORTED;
  }
}
