// Everything a lane does with its wave or its workgroup (gfx950, wave64): reductions, the
// (value, index) arg-reductions, the DPP movers and what is built on them, the scan, block
// reductions through LDS, LDS-only barriers. Included by common.h. What workgroups do with
// each other is in coop.h.
//
// Two families. The xor-shuffle forms (__shfl_xor compiles to ds_bpermute: six dependent
// round trips through the LDS crossbar) leave a result in every lane, but for a sum each
// lane adds in its own order, so the lanes' bits may differ in the last place. The DPP forms
// (*_dpp, row_*, sub16_sum, the scan) stay on the VALU and end in one fixed order of steps,
// so every lane gets the same bits. Each DPP sequence keeps its own order of steps, since
// the order fixes the bits of a sum: none is expressed through another.
//
// EVERY helper here needs the whole wave active (EXEC all ones): a shuffle or DPP move that
// reads an inactive lane reads garbage or zero. Call them outside divergent branches.
#pragma once
#include <hip/hip_runtime.h>

// ---- xor-shuffle reductions: v = op(v, partner's v) over offsets 32 .. 1 -----------------
template <typename T, typename Op>
__device__ __forceinline__ T wave_reduce(T v, Op op) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = op(v, __shfl_xor(v, o, 64));
  return v;
}

__device__ __forceinline__ float wave_sum(float v) {
  return wave_reduce(v, [](float a, float b) { return a + b; });
}
__device__ __forceinline__ double wave_sum_d(double v) {
  return wave_reduce(v, [](double a, double b) { return a + b; });
}
__device__ __forceinline__ int wave_sum_i(int v) {
  return wave_reduce(v, [](int a, int b) { return a + b; });
}
__device__ __forceinline__ double wave_max_d(double v) {
  return wave_reduce(v, [](double a, double b) { return fmax(a, b); });
}
__device__ __forceinline__ double wave_min_d(double v) {
  return wave_reduce(v, [](double a, double b) { return fmin(a, b); });
}
__device__ __forceinline__ double wave_prod_d(double v) {
  return wave_reduce(v, [](double a, double b) { return a * b; });
}
__device__ __forceinline__ float wave_max_f(float v) {
  return wave_reduce(v, [](float a, float b) { return fmaxf(a, b); });
}
__device__ __forceinline__ float wave_min_f(float v) {
  return wave_reduce(v, [](float a, float b) { return fminf(a, b); });
}
__device__ __forceinline__ unsigned long long wave_min_u64(unsigned long long v) {
  return wave_reduce(v, [](unsigned long long a, unsigned long long b) { return b < a ? b : a; });
}

// ---- (value, index) arg-max / arg-min -----------------------------------------------------
// THE TIE RULE, for every arg-reduction of the project (torch.argmax / argmin order): the
// other pair replaces mine if its value is strictly better, or equal at a LOWER index, whatever
// lanes the two pairs sit in. Both tests are false when either value is NaN, so a NaN never
// replaces a number. Nor does a number replace a NaN: a lane that enters with a NaN keeps it
// and hides what it would have passed on, so callers keep NaN out of the lanes (they seed
// with -inf / +inf and admit a candidate by a strict comparison, which a NaN fails).
// The rule is a macro so that it is written once and can still stand directly in an `if`:
// as a branch condition it compiles to short-circuit branches, through the bool-returning
// arg_better to mask arithmetic, and each caller keeps the form it was measured with.
#define HARP_ARG_BETTER(MAX, ov, oi, v, i) \
  ((MAX) ? ((ov) > (v) || ((ov) == (v) && (oi) < (i))) : ((ov) < (v) || ((ov) == (v) && (oi) < (i))))
template <bool MAX>
__device__ __forceinline__ bool arg_better(double ov, int oi, double v, int i) {
  return HARP_ARG_BETTER(MAX, ov, oi, v, i);
}
template <bool MAX>
__device__ __forceinline__ void arg_take(double& v, int& i, double ov, int oi) {
  if (arg_better<MAX>(ov, oi, v, i)) {
    v = ov;
    i = oi;
  }
}

// xor-shuffle form, the result in every lane
template <bool MAX>
__device__ __forceinline__ void wave_arg_xor(double& v, int& i) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const double w = __shfl_xor(v, o, 64);
    const int wi = __shfl_xor(i, o, 64);
    if (HARP_ARG_BETTER(MAX, w, wi, v, i)) {
      v = w;
      i = wi;
    }
  }
}

// ---- DPP movers and lane reads ------------------------------------------------------------
// CTRL: 0xB1 quad_perm [1,0,3,2], 0x4E quad_perm [2,3,0,1], 0x124 / 0x128 row_ror 4 / 8,
// 0x140 row_mirror, 0x141 row_half_mirror. All rows and banks enabled, no bound control.
template <int CTRL>
__device__ __forceinline__ int dpp_mov_i(int v) {
  return __builtin_amdgcn_update_dpp(0, v, CTRL, 0xf, 0xf, false);
}
template <int CTRL>
__device__ __forceinline__ float dpp_mov_f(float v) {
  return __int_as_float(dpp_mov_i<CTRL>(__float_as_int(v)));
}
template <int CTRL>
__device__ __forceinline__ double dpp_mov_d(double v) {
  const unsigned long long u = __builtin_bit_cast(unsigned long long, v);
  const unsigned lo = (unsigned)dpp_mov_i<CTRL>((int)(unsigned)u);
  const unsigned hi = (unsigned)dpp_mov_i<CTRL>((int)(unsigned)(u >> 32));
  return __builtin_bit_cast(double, ((unsigned long long)hi << 32) | lo);
}
// lane l's value as a wave-uniform (scalar) value; l must be wave-uniform
__device__ __forceinline__ double readlane_d(double v, int l) {
  const unsigned long long u = __builtin_bit_cast(unsigned long long, v);
  const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)u, l);
  const unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(u >> 32), l);
  return __builtin_bit_cast(double, ((unsigned long long)hi << 32) | lo);
}

// wave64 fp64 sum on the DPP network: quad_perm [1,0,3,2] and [2,3,0,1], row_ror 4 and 8
// leave every lane of a 16-lane row with the row's sum; the four row sums are then read
// from lanes 0 / 16 / 32 / 48 (v_readlane) and added in one fixed order, so every lane gets
// the same bits. Six dependent ds_bpermute round trips become four DPP moves and eight
// readlanes.
__device__ __forceinline__ double wave_sum_d_dpp(double v) {
  v += dpp_mov_d<0xB1>(v);   // quad_perm [1,0,3,2]
  v += dpp_mov_d<0x4E>(v);   // quad_perm [2,3,0,1]
  v += dpp_mov_d<0x124>(v);  // row_ror:4
  v += dpp_mov_d<0x128>(v);  // row_ror:8
  return (readlane_d(v, 0) + readlane_d(v, 16)) + (readlane_d(v, 32) + readlane_d(v, 48));
}

// fp32 sum over the 16 lanes of a DPP row, the result in every lane of the row: row
// rotations by 8 and 4, then the two quad permutations.
__device__ __forceinline__ float sub16_sum(float v) {
  v += dpp_mov_f<0x128>(v);  // row_ror:8
  v += dpp_mov_f<0x124>(v);  // row_ror:4
  v += dpp_mov_f<0x4E>(v);   // quad_perm [2,3,0,1]
  v += dpp_mov_f<0xB1>(v);   // quad_perm [1,0,3,2]
  return v;
}
// fp32 wave sum: the row sums of sub16_sum, then the rows by two xor shuffles
__device__ __forceinline__ float wave_sum_rows(float v) {
  v = sub16_sum(v);
  v += __shfl_xor(v, 16);
  v += __shfl_xor(v, 32);
  return v;
}

// (value, index) arg-reduction (tie rule above) and fp64 min inside each 16-lane row, the
// row's result in every lane of the row; then over the wave through v_readlane of lanes
// 0 / 16 / 32 / 48, rows taken in ascending order: a wave-uniform result.
template <bool MAX>
__device__ __forceinline__ void row_arg(double& v, int& i) {
  arg_take<MAX>(v, i, dpp_mov_d<0x128>(v), dpp_mov_i<0x128>(i));  // row_ror:8
  arg_take<MAX>(v, i, dpp_mov_d<0x124>(v), dpp_mov_i<0x124>(i));  // row_ror:4
  arg_take<MAX>(v, i, dpp_mov_d<0x4E>(v), dpp_mov_i<0x4E>(i));    // quad_perm [2,3,0,1]
  arg_take<MAX>(v, i, dpp_mov_d<0xB1>(v), dpp_mov_i<0xB1>(i));    // quad_perm [1,0,3,2]
}
template <bool MAX>
__device__ __forceinline__ void wave_arg_dpp(double& v, int& i) {
  row_arg<MAX>(v, i);
  double r = readlane_d(v, 0);
  int ri = __builtin_amdgcn_readlane(i, 0);
#pragma unroll
  for (int q = 16; q < 64; q += 16) arg_take<MAX>(r, ri, readlane_d(v, q), __builtin_amdgcn_readlane(i, q));
  v = r;
  i = ri;
}
__device__ __forceinline__ double row_min_d(double v) {
  v = fmin(v, dpp_mov_d<0x128>(v));
  v = fmin(v, dpp_mov_d<0x124>(v));
  v = fmin(v, dpp_mov_d<0x4E>(v));
  return fmin(v, dpp_mov_d<0xB1>(v));
}
__device__ __forceinline__ double wave_min_d_dpp(double v) {
  v = row_min_d(v);
  return fmin(fmin(readlane_d(v, 0), readlane_d(v, 16)), fmin(readlane_d(v, 32), readlane_d(v, 48)));
}

// wave64 inclusive prefix sum on the DPP network (no LDS round trips): Hillis-Steele within
// each 16-lane row (row_shr 1, 2, 4, 8), then row_bcast:15 into rows 1 and 3 and
// row_bcast:31 into rows 2 and 3; lanes without a source add 0.
__device__ __forceinline__ float dpp_shift_add(float v, int sel) {
  int t;
  switch (sel) {
    case 0: t = __builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x111, 0xf, 0xf, false); break;
    case 1: t = __builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x112, 0xf, 0xf, false); break;
    case 2: t = __builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x114, 0xf, 0xf, false); break;
    case 3: t = __builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x118, 0xf, 0xf, false); break;
    case 4: t = __builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x142, 0xa, 0xf, false); break;
    default: t = __builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x143, 0xc, 0xf, false); break;
  }
  return v + __int_as_float(t);
}

__device__ __forceinline__ float wave_scan_incl(float v) {
  v = dpp_shift_add(v, 0);
  v = dpp_shift_add(v, 1);
  v = dpp_shift_add(v, 2);
  v = dpp_shift_add(v, 3);
  v = dpp_shift_add(v, 4);
  v = dpp_shift_add(v, 5);
  return v;
}

// wave-uniform total (scalar register), no LDS traffic
__device__ __forceinline__ float wave_total(float v) {
  return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(wave_scan_incl(v)), 63));
}

// ---- block reductions through LDS, the result in every thread ----------------------------
// All threads of the workgroup call them; red[] holds one double per wave. Two barrier
// placements, because the callers differ in what surrounds the call and one form cannot
// serve both without moving their code:
//  * block_sum_d<T> (eig.hip; T threads, a compile-time constant): write, barrier, read,
//    barrier. After the closing barrier the caller may write red[] again at once (eig calls
//    it from loops with nothing in between), and house_lds relies on the two barriers to
//    order its own LDS column writes before the reads that follow the call.
//  * block_sum_d_pre / block_max_d_pre (tridiag_dc.hip; wave count from blockDim): barrier,
//    write, barrier, read. The opening barrier protects red[] from the previous call, whose
//    reads have no barrier after them: the calls come back to back. block_max_d_pre starts
//    from 0 (its callers reduce magnitudes).
// tsqr.hip keeps a four-wave sum on wave_sum_d (the xor-shuffle form and its own order of
// the four partials fix its bits).
template <int T>
__device__ __forceinline__ double block_sum_d(double v, double* red) {
  v = wave_sum_d_dpp(v);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  double s = 0.0;
#pragma unroll
  for (int w = 0; w < T / 64; ++w) s += red[w];
  __syncthreads();
  return s;
}
__device__ __forceinline__ double block_sum_d_pre(double v, double* red) {
  v = wave_sum_d_dpp(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  double s = 0.0;
  for (int w = 0; w < (int)(blockDim.x >> 6); ++w) s += red[w];
  return s;
}
__device__ __forceinline__ double block_max_d_pre(double v, double* red) {
  v = wave_max_d(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  double s = 0.0;
  for (int w = 0; w < (int)(blockDim.x >> 6); ++w) s = fmax(s, red[w]);
  return s;
}

// block arg-reduction (T threads, <= 16 waves): each wave's result through LDS, then EVERY
// wave reduces the partials itself (one row of lanes), so no second barrier; the caller
// must not write sv / si again before its next barrier. Wave-uniform result.
template <bool MAX, int T>
__device__ __forceinline__ void block_arg(double& v, int& i, double* sv, int* si, int lane, int wv) {
  wave_arg_dpp<MAX>(v, i);
  if (lane == 0) {
    sv[wv] = v;
    si[wv] = i;
  }
  __syncthreads();
  const double id = MAX ? -__builtin_inf() : __builtin_inf();
  v = lane < T / 64 ? sv[lane] : id;
  i = lane < T / 64 ? si[lane] : 0x7fffffff;
  row_arg<MAX>(v, i);
  v = readlane_d(v, 0);
  i = __builtin_amdgcn_readlane(i, 0);
}

// ---- smaller pieces -------------------------------------------------------------------------
// workgroup barrier for LDS traffic only: __syncthreads() also drains vmcnt, i.e. waits for
// outstanding global loads and stores
__device__ __forceinline__ void lds_sync() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }
// LDS ordering within one wave (its lanes run in lockstep: no barrier)
__device__ __forceinline__ void lds_sync_wave() {
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  __builtin_amdgcn_wave_barrier();
}

// 1 / x by v_rcp_f64 and two Newton steps (the IEEE divide is a ~10-instruction dependent chain)
__device__ __forceinline__ double rcp_newton_d(double x) {
  double r = __builtin_amdgcn_rcp(x);
  r = fma(r, fma(-x, r, 1.0), r);
  return fma(r, fma(-x, r, 1.0), r);
}
