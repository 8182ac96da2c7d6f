// Sparse kernel matrices for gfx950, fp64: K = f(X Y^T) for two CSR operands with a dense
// output, never forming a dense n x d block.
//
// Replaces the kernel functions of the reference's csr applications (ml/daal/.../
// daal_kernel_func/{LinCSRBatch, RbfCSRBatch} in matrixMatrix mode, and the Gram matrix that
// daal_svm/MultiClassCSRBatch trains on). Operands as in csr_stats.hip: rowptr int64 [n+1],
// col int32 [nnz] (sorted within a row, no duplicates), val fp64 [nnz].
//
// A workgroup (4 waves) owns one T x T tile of outputs: lane l of every wave owns Y row
// j0 + l, wave w owns X rows ib + w * T/4 ..., so an output element has one owner lane, its
// products are added by fma in ascending column order, and a wave's store of one output
// row is 512 contiguous bytes. No atomics, no cross-workgroup sums: equal inputs give equal
// bits, and kernel_block(X, X) is bitwise symmetric (fma(a, b, c) == fma(b, a, c)).
//
// Two paths (the host picks, ops/csr_kernel.py):
//   * slab: the column range is walked in slabs of S columns. The Y tile's part of a slab is
//     scattered into LDS as a dense [S][T] block, column-major: the 64 lanes read one column
//     as 512 contiguous bytes (ds_read_b64: both 32-lane halves cover one 256-B bank row, no
//     conflict). The X rows' nonzeros inside the slab are streamed as wave-uniform values
//     (held by the lane that owns the row, handed out by readlane): one LDS read and one fp64
//     FMA per (nonzero, lane) into register accumulators. Three LDS blocks rotate: while
//     slab s is multiplied, slab s + 1 is scattered and the entries of slab s - 1 are zeroed
//     again (only the entries, not the block), one barrier per slab. Rows are walked with
//     cursors whose next entry is held in registers, so no per-row offset table is needed
//     and a slab without an entry of a row costs that row no memory access; a slab without X
//     entries costs the barrier only, one without Y entries no FMA.
//   * merge, for hyper-sparse rows (most slabs empty): the Y rows of the tile are staged in
//     LDS once (when they fit; else read from global memory); the X row's entries are
//     wave-uniform, and every lane advances a cursor through its own sorted Y row.
// The epilogue (linear, RBF, squared distance) is fused: out is written once, never re-read.
#include "common.h"

#define CSR_KERNEL_TILE 64
#define CSR_KERNEL_SLAB 32
#define CSR_KERNEL_MERGE_CAP 4096  // staged Y entries of a tile: 4096 * 12 B = 48 KB

namespace {

constexpr int T = CSR_KERNEL_TILE;
constexpr int S = CSR_KERNEL_SLAB;
constexpr int RPW = T / 4;  // X rows per wave
constexpr int CAP = CSR_KERNEL_MERGE_CAP;
constexpr int NOCOL = 0x7fffffff;

enum { GRAM = 0, LINEAR = 1, RBF = 2, SQDIST = 3 };

// RBF: the expression of rbf_from_gram_kernel (kernelmat.hip), so equal g gives equal bits
template <int MODE>
__device__ __forceinline__ double epilogue(double g, double nxi, double nyj, double p0, double p1) {
  if (MODE == GRAM) return g;
  if (MODE == LINEAR) return p0 * g + p1;
  double d2 = nxi + nyj - 2.0 * g;
  d2 = d2 > 0.0 ? d2 : 0.0;
  return MODE == RBF ? exp(-d2 * p0) : d2;
}

__global__ __launch_bounds__(256) void csr_row_sqnorm_kernel(const long* __restrict__ rowptr,
                                                             const double* __restrict__ val, long n,
                                                             double* __restrict__ out) {
  for (long r = (long)blockIdx.x * blockDim.x + threadIdx.x; r < n; r += (long)gridDim.x * blockDim.x) {
    double s = 0.0;
    for (long p = rowptr[r]; p < rowptr[r + 1]; ++p) s = fma(val[p], val[p], s);
    out[r] = s;
  }
}

template <int MODE>
__global__ __launch_bounds__(256) void csr_kernel_slab_kernel(
    const long* __restrict__ xrp, const int* __restrict__ xcol, const double* __restrict__ xval, long i0, long i1,
    const long* __restrict__ yrp, const int* __restrict__ ycol, const double* __restrict__ yval, long m, int d,
    const double* __restrict__ nx, const double* __restrict__ ny, double p0, double p1, double* __restrict__ out,
    long ld) {
  __shared__ double ys[3][S * T];  // 48 KB: three workgroups per CU
  __shared__ int yany[3];          // does the block hold an entry?
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const long j0 = (long)blockIdx.x * T, ib = i0 + (long)blockIdx.y * T;
  for (int t = threadIdx.x; t < 3 * S * T; t += 256) (&ys[0][0])[t] = 0.0;
  if (threadIdx.x < 3) yany[threadIdx.x] = 0;

  // Y row j0 + lane is scattered (and zeroed again) by the lane of wave (lane & 3): one
  // owner thread per row, so a fill and a clear never race on an address
  const bool yown = (lane & 3) == wave && j0 + lane < m;
  long yp = 0, ye = 0;
  int ync = NOCOL;  // the row's next entry, held in registers: a slab without one costs no load
  double ynv = 0.0;
  if (yown) {
    yp = yrp[j0 + lane];
    ye = yrp[j0 + lane + 1];
    if (yp < ye) {
      ync = ycol[yp];
      ynv = yval[yp];
    }
  }
  long qa = yp, qb = yp;  // start of the row's entries in slab s - 1 and s
  // X row ib + wave * RPW + r lives on lane r: cursor, end and the next entry, prefetched
  long xp = 0, xe = 0;
  int xc = NOCOL;
  double xv = 0.0;
  if (lane < RPW && ib + wave * RPW + lane < i1) {
    xp = xrp[ib + wave * RPW + lane];
    xe = xrp[ib + wave * RPW + lane + 1];
    if (xp < xe) {
      xc = xcol[xp];
      xv = xval[xp];
    }
  }
  double acc[RPW];
#pragma unroll
  for (int r = 0; r < RPW; ++r) acc[r] = 0.0;
  __syncthreads();

  const int nslab = (int)(((long)d + S - 1) / S);
  // scatter slab f of the owned Y row into block f % 3
  auto fill = [&](int f) {
    double* buf = ys[f % 3];
    const int c0 = f * S;
    bool any = false;
    while (ync < c0 + S) {  // NOCOL once the row is used up, and on the lanes that own no row
      if ((unsigned)(ync - c0) < (unsigned)S) {  // a column below c0 (unsorted input) is dropped, never out of the block
        buf[(ync - c0) * T + lane] = ynv;
        any = true;
      }
      ++yp;
      if (yp < ye) {
        ync = ycol[yp];
        ynv = yval[yp];
      } else {
        ync = NOCOL;
      }
    }
    if (any) yany[f % 3] = 1;
  };
  if (nslab > 0) fill(0);
  __syncthreads();

  for (int s = 0; s < nslab; ++s) {
    const int c0 = s * S, cend = c0 + S;
    if (s >= 1) {  // zero the entries of slab s - 1 again: positions qa .. qb
      double* buf = ys[(s + 2) % 3];
      const int cp = c0 - S;
      for (long q = qa; q < qb; ++q) {
        const unsigned cl = (unsigned)(ycol[q] - cp);
        if (cl < (unsigned)S) buf[cl * T + lane] = 0.0;
      }
      if (threadIdx.x == 0) yany[(s + 2) % 3] = 0;
    }
    qa = qb;
    qb = yp;
    if (s + 1 < nslab) fill(s + 1);

    const double* buf = ys[s % 3];
    const bool any = yany[s % 3] != 0;
#pragma unroll
    for (int r = 0; r < RPW; ++r) {
      for (;;) {
        const int c = __builtin_amdgcn_readlane(xc, r);
        if (c >= cend) break;  // wave-uniform
        const double v = readlane_d(xv, r);
        const unsigned cl = (unsigned)(c - c0);
        if (any && cl < (unsigned)S) acc[r] = fma(v, buf[cl * T + lane], acc[r]);
        if (lane == r) {
          ++xp;
          if (xp < xe) {
            xc = xcol[xp];
            xv = xval[xp];
          } else {
            xc = NOCOL;
          }
        }
      }
    }
    __syncthreads();
  }

  const long j = j0 + lane;
  if (j < m) {
    const double nyj = MODE >= RBF ? ny[j] : 0.0;
#pragma unroll
    for (int r = 0; r < RPW; ++r) {
      const long i = ib + wave * RPW + r;
      if (i < i1) out[(i - i0) * ld + j] = epilogue<MODE>(acc[r], MODE >= RBF ? nx[i] : 0.0, nyj, p0, p1);
    }
  }
}

// one X entry (c, v), wave-uniform, against the lane's Y row: cursor py .. pye into cs / vs
__device__ __forceinline__ void merge_step(int c, double v, const int* cs, const double* vs, long& py, long pye,
                                           double& acc) {
  while (py < pye && cs[py] < c) ++py;
  if (py < pye && cs[py] == c) acc = fma(v, vs[py], acc);
}

template <int MODE>
__global__ __launch_bounds__(256) void csr_kernel_merge_kernel(
    const long* __restrict__ xrp, const int* __restrict__ xcol, const double* __restrict__ xval, long i0, long i1,
    const long* __restrict__ yrp, const int* __restrict__ ycol, const double* __restrict__ yval, long m, int d,
    const double* __restrict__ nx, const double* __restrict__ ny, double p0, double p1, double* __restrict__ out,
    long ld) {
  __shared__ int sc[CAP];
  __shared__ double sv[CAP];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const long j0 = (long)blockIdx.x * T, ib = i0 + (long)blockIdx.y * T;
  const long jend = j0 + T < m ? j0 + T : m;
  const long ya = yrp[j0], yb = yrp[jend];
  const bool staged = yb - ya <= CAP;  // workgroup-uniform
  if (staged)
    for (long t = threadIdx.x; t < yb - ya; t += 256) {
      sc[t] = ycol[ya + t];
      sv[t] = yval[ya + t];
    }
  __syncthreads();
  const long j = j0 + lane;
  long pyb = 0, pye = 0;  // the lane's Y row, relative to ya
  if (j < m) {
    pyb = yrp[j] - ya;
    pye = yrp[j + 1] - ya;
  }
  const double nyj = (MODE >= RBF && j < m) ? ny[j] : 0.0;
  for (int r = 0; r < RPW; ++r) {
    const long i = ib + wave * RPW + r;
    if (i >= i1) break;  // wave-uniform
    const long xa = xrp[i], xb = xrp[i + 1];
    double acc = 0.0;
    long py = pyb;
    for (long q0 = xa; q0 < xb; q0 += 64) {  // wave-uniform trip counts: the readlanes see every lane
      const int cnt = (int)(xb - q0 < 64 ? xb - q0 : 64);
      const int cl = lane < cnt ? xcol[q0 + lane] : 0;
      const double vl = lane < cnt ? xval[q0 + lane] : 0.0;
      for (int t = 0; t < cnt; ++t) {
        const int c = __builtin_amdgcn_readlane(cl, t);
        const double v = readlane_d(vl, t);
        if (staged) merge_step(c, v, sc, sv, py, pye, acc);
        else merge_step(c, v, ycol + ya, yval + ya, py, pye, acc);
      }
    }
    if (j < m) out[(i - i0) * ld + j] = epilogue<MODE>(acc, MODE >= RBF ? nx[i] : 0.0, nyj, p0, p1);
  }
}

template <int MODE>
int launch_block(int path, dim3 grid, hipStream_t s, const long* xrp, const int* xcol, const double* xval, long i0,
                 long i1, const long* yrp, const int* ycol, const double* yval, long m, int d, const double* nx,
                 const double* ny, double p0, double p1, double* out, long ld) {
  if (path == 0)
    csr_kernel_slab_kernel<MODE><<<grid, dim3(256), 0, s>>>(xrp, xcol, xval, i0, i1, yrp, ycol, yval, m, d, nx, ny,
                                                            p0, p1, out, ld);
  else
    csr_kernel_merge_kernel<MODE><<<grid, dim3(256), 0, s>>>(xrp, xcol, xval, i0, i1, yrp, ycol, yval, m, d, nx, ny,
                                                             p0, p1, out, ld);
  return harp_launch_status();
}

}  // namespace

HARP_EXPORT int harp_csr_kernel_tile() { return CSR_KERNEL_TILE; }
HARP_EXPORT int harp_csr_kernel_slab() { return CSR_KERNEL_SLAB; }

// out [n] = |x_i|^2 (val may be null when there is no stored entry)
HARP_EXPORT int harp_csr_row_sqnorm(const long* rowptr, const int* col, const double* val, long n, double* out,
                                    hipStream_t s) {
  (void)col;
  if (n < 0) return HARP_EBADARG;
  if (n == 0) return HARP_OK;
  if (!rowptr || !out) return HARP_EBADARG;
  long blocks = (n + 255) / 256;
  if (blocks > 65536) blocks = 65536;
  csr_row_sqnorm_kernel<<<dim3((unsigned)blocks), dim3(256), 0, s>>>(rowptr, val, n, out);
  return harp_launch_status();
}

// out[(i - i0) * ld + j] = f(<x_i, y_j>) for i in [i0, i1), j in [0, m); X is n x d, Y is m x d.
// mode 0 gram: g; 1 linear: p0 * g + p1; 2 rbf: exp(-max(nx_i + ny_j - 2 g, 0) * p0), p0 =
// 1 / (2 sigma^2); 3 sqdist: the clamped distance. nx [n], ny [m]: squared row norms (modes 2,
// 3). path 0: slab, 1: merge.
HARP_EXPORT int harp_csr_kernel_block(const long* xrp, const int* xcol, const double* xval, long n, long i0, long i1,
                                      const long* yrp, const int* ycol, const double* yval, long m, int d, int mode,
                                      double p0, double p1, const double* nx, const double* ny, int path, double* out,
                                      long ld, hipStream_t s) {
  if (n < 0 || m < 0 || d < 0 || i0 < 0 || i1 < i0 || i1 > n || ld < m || mode < GRAM || mode > SQDIST ||
      (path != 0 && path != 1))
    return HARP_EBADARG;
  if (mode == RBF && !(p0 > 0)) return HARP_EBADARG;
  if (i1 == i0 || m == 0) return HARP_OK;
  if (!xrp || !yrp || !out || (mode >= RBF && (!nx || !ny))) return HARP_EBADARG;
  const long tx = (i1 - i0 + T - 1) / T, ty = (m + T - 1) / T;
  if (tx > 65535 || ty > 0x7fffffffL || d > NOCOL - S) return HARP_EUNSUPPORTED;
  const dim3 grid((unsigned)ty, (unsigned)tx);
  switch (mode) {
    case GRAM:
      return launch_block<GRAM>(path, grid, s, xrp, xcol, xval, i0, i1, yrp, ycol, yval, m, d, nx, ny, p0, p1, out, ld);
    case LINEAR:
      return launch_block<LINEAR>(path, grid, s, xrp, xcol, xval, i0, i1, yrp, ycol, yval, m, d, nx, ny, p0, p1, out,
                                  ld);
    case RBF:
      return launch_block<RBF>(path, grid, s, xrp, xcol, xval, i0, i1, yrp, ycol, yval, m, d, nx, ny, p0, p1, out, ld);
    default:
      return launch_block<SQDIST>(path, grid, s, xrp, xcol, xval, i0, i1, yrp, ycol, yval, m, d, nx, ny, p0, p1, out,
                                  ld);
  }
}
