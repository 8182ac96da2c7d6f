// Test utilities: a bounded "CU hog" that keeps workgroups resident for a fixed wall time,
// to rehearse the cooperative kernels (one-XCD eigensolver, 16-CU SMO) under CU contention
// on one GPU, as RCCL kernels would cause at P > 1 (tests/test_coop_contention_gpu.py); and
// a kernel that applies one primitive of wave.h to caller-given lanes (tests/test_wave_gpu.py).
#include "common.h"

namespace {

// every workgroup holds `lds` bytes of LDS (dynamic) and spins until `ticks` of the 100 MHz
// realtime counter have passed since it started (bounded: the grid always drains)
__global__ __launch_bounds__(256) void spin_kernel(long long ticks, int* __restrict__ done) {
  extern __shared__ int hog_lds[];
  const long long t0 = __builtin_amdgcn_s_memrealtime();
  if (threadIdx.x == 0) hog_lds[0] = 1;
  while (__builtin_amdgcn_s_memrealtime() - t0 < ticks) __builtin_amdgcn_s_sleep(8);
  __syncthreads();
  if (threadIdx.x == 0) atomicAdd(done, hog_lds[0]);
}

// One workgroup of NW waves: thread t takes (in_d[t], in_i[t]), applies the primitive `op`
// selects (the same for all threads, so every wave is whole) and writes its own result to
// (out_d[t], out_i[t]). fp32 primitives work on (float)in_d[t] and return it widened; the
// u64 minimum works on the bits of in_d[t]. The op numbers are harp_amd/ops/testutil.py's.
template <int NW>
__global__ __launch_bounds__(NW * 64) void wave_test_kernel(int op, const double* __restrict__ in_d,
                                                            const int* __restrict__ in_i, double* __restrict__ out_d,
                                                            int* __restrict__ out_i) {
  constexpr int T = NW * 64;
  __shared__ double red[16], sv[16];
  __shared__ int si[16];
  const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
  double v = in_d[t];
  int i = in_i[t];
  const float f = (float)v;
  switch (op) {
    case 0: v = wave_sum(f); break;
    case 1: v = wave_sum_d(v); break;
    case 2: i = wave_sum_i(i); break;
    case 3: v = wave_max_d(v); break;
    case 4: v = wave_min_d(v); break;
    case 5: v = wave_prod_d(v); break;
    case 6: v = wave_max_f(f); break;
    case 7: v = wave_min_f(f); break;
    case 8: v = __longlong_as_double((long long)wave_min_u64((unsigned long long)__double_as_longlong(v))); break;
    case 9: wave_arg_xor<true>(v, i); break;
    case 10: wave_arg_xor<false>(v, i); break;
    case 11: wave_arg_dpp<true>(v, i); break;
    case 12: wave_arg_dpp<false>(v, i); break;
    case 13: v = wave_sum_d_dpp(v); break;
    case 14: v = wave_min_d_dpp(v); break;
    case 15: v = row_min_d(v); break;
    case 16: row_arg<true>(v, i); break;
    case 17: row_arg<false>(v, i); break;
    case 18: v = sub16_sum(f); break;
    case 19: v = wave_sum_rows(f); break;
    case 20: v = wave_scan_incl(f); break;
    case 21: v = wave_total(f); break;
    case 22: v = readlane_d(v, __builtin_amdgcn_readfirstlane(i) & 63); break;
    case 23: v = block_sum_d<T>(v, red); break;
    case 24: v = block_sum_d_pre(v, red); break;
    case 25: v = block_max_d_pre(v, red); break;
    case 26: block_arg<true, T>(v, i, sv, si, lane, wv); break;
    case 27: block_arg<false, T>(v, i, sv, si, lane, wv); break;
    default: break;
  }
  out_d[t] = v;
  out_i[t] = i;
}
constexpr int kWaveTestOps = 28;

}  // namespace

// blocks workgroups of 256 threads, each holding lds bytes of LDS for us microseconds;
// done (one int, zeroed) counts the workgroups that finished
HARP_EXPORT int harp_test_spin(int blocks, int lds, long long us, int* done, hipStream_t s) {
  if (blocks < 1 || lds < 4 || lds > 160 * 1024 || us < 0 || us > 10000000 || !done) return HARP_EBADARG;
  if (lds > 65536 &&
      hipFuncSetAttribute((const void*)spin_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, lds) != hipSuccess)
    return HARP_ELAUNCH;
  spin_kernel<<<dim3((unsigned)blocks), dim3(256), (size_t)lds, s>>>(us * 100, done);
  return harp_launch_status();
}

// in_f64 / in_i32 / out_f64 / out_i32: nwaves * 64 entries each; nwaves is 1, 4 or 16
HARP_EXPORT int harp_test_wave(int op, const double* in_f64, const int* in_i32, double* out_f64, int* out_i32,
                               int nwaves, hipStream_t s) {
  if (op < 0 || op >= kWaveTestOps || !in_f64 || !in_i32 || !out_f64 || !out_i32) return HARP_EBADARG;
  if (nwaves == 1) wave_test_kernel<1><<<1, 64, 0, s>>>(op, in_f64, in_i32, out_f64, out_i32);
  else if (nwaves == 4) wave_test_kernel<4><<<1, 256, 0, s>>>(op, in_f64, in_i32, out_f64, out_i32);
  else if (nwaves == 16) wave_test_kernel<16><<<1, 1024, 0, s>>>(op, in_f64, in_i32, out_f64, out_i32);
  else return HARP_EBADARG;
  return harp_launch_status();
}
