// K-means kernels for gfx950 (MI355X / CDNA4).
//
// Replaces the reference's K-means E-step + accumulate hot loop
// (ml/java/.../kmeans/regroupallgather/CenCalcTask.java:67-100: per point, argmin
// over all centroids of the squared L2 distance, then local[c] += (1, x)) and the
// thread merge (CenMergeTask.java:36-54) and the owner-side average
// (KMeansCollectiveMapper.java:170-183).
//
// Design (MI355X-first, not a translation):
//  * distances are a GEMM: X[N,dp] (bf16) x (-2C)[Kp,dp]^T on v_mfma_f32_32x32x16_bf16.
//    ||c||^2 is folded INTO the GEMM: X carries 1.0 in columns d..d+3 and -2C carries
//    0, hi, mid, lo there (||c||^2 = hi + mid + lo in three bf16 terms, ~24-bit exact), so
//    the zero-initialised accumulator IS the distance minus ||x||^2 and the epilogue is a
//    pure argmin (no row-constant registers, no norm reads from LDS). d=100 pads to 112,
//    the same K as without the fold.
//  * centroids sit on the MFMA row axis, points on the lane (column) axis: each lane
//    owns one point and 16 candidate centroids per 32x32 tile, so the argmin is
//    register-local (16 keyed fminf -> v_min3) plus one lane<->lane+32 exchange.
//    The within-tile register index is packed into the 4 low mantissa bits of the
//    distance (relative perturbation 2^-19, far below the bf16 operand rounding).
//  * X fragments stay in VGPRs for the whole centroid sweep; centroid tiles stream
//    through double-buffered LDS (three slots in the keyless sweep) filled by
//    global_load_lds (LDS-DMA, no staging VGPRs) with a per-row chunk rotation applied to
//    the DMA source so ds_read_b128 stays conflict-free; A fragments are register
//    double-buffered across 32-row groups; one barrier per stage.
//  * column d of X (1.0) meets column d of -2C (0): the accumulation adds (x, 1) =
//    (partial sum, count) in one row: the Harp centroid row layout (sum + count) falls out
//    of the data layout.
//  * accumulation: per assigned point, one 256-B contiguous f32 atomic row segment
//    per wave-instruction (the full-rate atomic shape on gfx950).
#include "common.h"

#include <atomic>
#include <type_traits>

namespace {

constexpr float KM_BIG = 1.0e38f;
constexpr int KM_ONES = 4;  // X columns d..d+3 hold 1.0: count + the 3 folded ||c||^2 terms

__device__ __forceinline__ float keyed(float v, unsigned idx) {
  return __uint_as_float((__float_as_uint(v) & ~0xFu) | idx);
}

template <int KS, int G, int WAVES_, int RG>
struct KMCfg {
  static constexpr int DP = KS * 16;                 // padded feature dim (elements)
  static constexpr int CPR = KS * 2;                 // 16-byte chunks per row
  static constexpr int TILE = RG * 32;               // centroids per stage
  static constexpr int WAVES = WAVES_;
  static constexpr int THREADS = WAVES_ * 64;
  static constexpr int TILE_BYTES = TILE * DP * 2;
  static constexpr int DMA_INSTR = TILE * CPR / 64;  // 1-KiB LDS-DMA wave-instructions per tile
  static constexpr int PTS = WAVES_ * G * 32;        // points per workgroup
  static_assert((TILE * CPR) % 64 == 0, "tile must be whole 1-KiB DMA pieces");
};

// LDS image of a centroid tile: row-major [TILE][CPR] 16-B chunks, chunk c of row r stored at
// position (c + s(r)) mod CPR with s(r) = (r >> 3) & 1. Rows r and r+8 then sit on different
// 16-B bank slots, so every ds_read_b128 lane group (16 distinct rows) is conflict-free, while
// the image stays lane-linear for global_load_lds (the swizzle is applied to the SOURCE).
template <class C>
__device__ __forceinline__ void stage_dma(const __bf16* __restrict__ cm2, int tile, char* lds, int wave, int lane) {
  // wave is a scalar at every call: the piece index, its LDS destination and the test for a
  // last partial round are scalars too, and the source is a scalar tile pointer plus one
  // 32-bit lane offset per piece (as 64-bit pointers the offsets take two VGPRs each, held
  // across the stage loop)
  const char* gsrc = (const char*)cm2 + (size_t)tile * C::TILE_BYTES;
#pragma unroll
  for (int j0 = 0; j0 < C::DMA_INSTR; j0 += C::WAVES) {
    const int j = j0 + wave;
    if (C::DMA_INSTR % C::WAVES == 0 || j < C::DMA_INSTR) {
      const int q = j * 64 + lane;
      const int row = q / C::CPR;
      int c = q - row * C::CPR - ((row >> 3) & 1);
      if (c < 0) c += C::CPR;
      unsigned lo = (unsigned)(row * C::CPR + c) * 16u;
      asm("" : "+v"(lo));  // keeps the zero-extension beside the load (kernel comment, ring sweep)
      __builtin_amdgcn_global_load_lds((const void __attribute__((address_space(1)))*)(gsrc + (size_t)lo),
                                       (void __attribute__((address_space(3)))*)(lds + j * 1024), 16, 0, 0);
    }
  }
}

// half H (0: waves 0 .. WAVES/2-1, 1: the rest) requests piece round p of the tile two stages
// ahead behind the first MFMAs of the chain issued in item i of the ring sweep, -1 for none:
// all of them behind the barrier in item 3 and inside the same stage. The two waves of a SIMD
// (w and w + WAVES/2) are in different halves, so they never request in the same item. (The
// chains issued in items 2, 6, 10, 14 carry the A-fragment reads; 6, 10 and 14 hold a request
// of one half as well, which was measured as it stands and not moved.)
constexpr int km_ring_piece_at(int H, int i) {
  constexpr int at[2][4] = {{5, 7, 10, 13}, {6, 9, 11, 14}};
  for (int p = 0; p < 4; ++p)
    if (at[H][p] == i) return p;
  return -1;
}
constexpr int KM_RING_BARRIER_ITEM = 3;

template <int KS, int G, int WAVES, int RG, int PIPE, int PRIO = 0, int KEYLESS = 0, int RING = 0>
__global__ __launch_bounds__(WAVES * 64) void kmeans_assign_kernel(
    const __bf16* __restrict__ X, long ldx, const __bf16* __restrict__ Cm2, long N, int ntiles, int tail_rg,
    int dcount, int* __restrict__ labels, float* __restrict__ sums, int ld_sums, float* __restrict__ obj_partial,
    float* __restrict__ mind, long nblk, unsigned* __restrict__ next_block) {
  using C = KMCfg<KS, G, WAVES, RG>;
  constexpr int NSLOT = RING ? 3 : 2;  // LDS slots of one centroid tile each
  static_assert(!RING || (KEYLESS && PIPE > 0 && G == 4 && RG == 4 && WAVES == 8 && KS <= 8),
                "the ring sweep is written for the keyless 4 x 4-item stage of 8 waves");
  __shared__ __attribute__((aligned(16))) char smem[NSLOT * C::TILE_BYTES + WAVES * 4 + 16];
  // PRIO (variant 15): static VALU-arbitration priority for the younger half of the
  // workgroup, set once (MI355X_MICROARCH.md, two waves per SIMD, item 4)
  if constexpr (PRIO)
    if (__builtin_amdgcn_readfirstlane((int)threadIdx.x) >= WAVES * 32) __builtin_amdgcn_s_setprio(1);

  // The grid is resident (launch_assign: at most as many workgroups as the device holds at
  // once) and each workgroup runs point blocks until none is left: its own index first, then
  // whatever *next_block (zeroed by the host in stream order) hands out, taken by one lane at
  // the head of the block's epilogue. A block starts exactly as a freshly launched workgroup
  // would (nothing of the sweep is carried over a block edge). A static stride b += gridDim.x
  // measured slower than one workgroup per block: the CUs do not run at one speed
  // (profiles/kmeans_slots).
  long b = blockIdx.x;
  while (b < nblk) {
    // The thread id is opaque per block: everything per lane below is derived again for every
    // block, as a new workgroup would. Derived once in front of the loop, the address arithmetic
    // of the block's prologue and epilogue is hoisted and held in VGPRs across the sweep (10 to 24
    // more per instantiation; the keyed 6 to 8 k-step instances then spill).
    int tid = threadIdx.x;
    long nb = N;  // (the point count too: N - 1 is otherwise kept in a VGPR pair for the clamp)
    asm volatile("" : "+v"(tid), "+s"(nb));
    const int lane = tid & 63, wave = tid >> 6;
    const int r = lane & 31, h = lane >> 5;
    const int srot = (r >> 3) & 1;
    // the block index and the wave's first point are scalars
    const int swave = __builtin_amdgcn_readfirstlane(wave);
    const long pbase = (b * WAVES + swave) * (G * 32);
    // kick off the first centroid tile before loading this wave's points
    stage_dma<C>(Cm2, 0, smem, swave, lane);
    // ring: the second tile too (with one tile, that tile again: slot 1 is then never used, but
    // the chain the last stage starts for a stage that does not exist reads written memory)
    if constexpr (RING) stage_dma<C>(Cm2, ntiles > 1 ? 1 : 0, smem + C::TILE_BYTES, swave, lane);

    // ---- this wave's points: B-operand fragments, resident for the whole sweep
    bf16x8 xf[G][KS];
#pragma unroll
    for (int g = 0; g < G; ++g) {
      long p = pbase + g * 32 + r;
      if (p > nb - 1) p = nb - 1;
      const bf16x8* row = (const bf16x8*)(X + p * ldx);
#pragma unroll
      for (int s = 0; s < KS; ++s) xf[g][s] = row[2 * s + h];
    }

    float best[G];
    int bestt[G];
#pragma unroll
    for (int g = 0; g < G; ++g) { best[g] = KM_BIG; bestt[g] = 0; }
    // argmin of one 32x32 tile into (best, bestt)[g]: the 16 candidates' register index rides
    // in the low mantissa bits (one v_and_or per candidate). A plain v_min3 with the index
    // searched only on improvement measured 5 % slower (it spills; profiles/r2_ktail).
    // KEYLESS (variant 16): the plain minimum of the 16 candidates, no index bits. The sweep then
    // knows only the winning 32-row group; the row inside it is found by the gather-sum pass,
    // which re-computes that one group's 32 distances per point (kmeans_resolve.hip). Its min
    // chain starts from best[g] itself: eight v_min3, one compare and one select per tile (10
    // VALU, 1.56 per MFMA at 7 k-steps) where the minimum of the 16 first and a compare against
    // best[g] after took 13 (profiles/r9_sweep_pipe). The keyed form stays: folded the same way
    // its RG=2 tiling (variant 13) spills at 7 k-steps.
    auto tile_argmin = [&](const floatx16& ac, int g, int tg) {
      if constexpr (KEYLESS) {
        float nb = best[g];
#pragma unroll
        for (int q = 0; q < 16; q += 2) nb = fminf(fminf(nb, ac[q]), ac[q + 1]);
        if (nb < best[g]) bestt[g] = tg;
        best[g] = nb;
      } else {
        float m = keyed(ac[0], 0u);
#pragma unroll
        for (int q = 1; q < 16; ++q) m = fminf(m, keyed(ac[q], (unsigned)q));
        if (m < best[g]) { best[g] = m; bestt[g] = tg; }
      }
    };

    // per-lane byte offsets of its A-fragment chunks inside a 32-row group
    int aoff[KS];
#pragma unroll
    for (int s = 0; s < KS; ++s) {
      int cp = 2 * s + h + srot;
      if (cp >= C::CPR) cp -= C::CPR;
      aoff[s] = (r * C::CPR + cp) * 16;
    }
    // aoff[s] = aoff[0] + 32 s except for the last chunk, which wraps in the rotated rows: two
    // per-lane bases and immediate offsets address every fragment (KS offsets held across the
    // sweep are five more VGPRs at 7 k-steps, and the keyed instances there have none to spare)
    const int aoff0 = aoff[0], aoffL = aoff[KS - 1] - 32 * (KS - 1);
    auto a_frag = [&](const char* base, int s) {
      return *(const bf16x8*)(base + (s == KS - 1 ? aoffL : aoff0) + 32 * s);
    };

    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();

    // full tiles; a last tile of only tail_rg (< RG) row groups runs after the loop
    const int nfull = tail_rg ? ntiles - 1 : ntiles;
    if constexpr (RING) {
      // The ring sweep (variant 16): the item pipeline of the two-slot body below run as ONE
      // stream over all full stages, with nothing at a stage edge that is not also inside a stage.
      //  * Three LDS slots, tile t in slot t % 3. One barrier per stage, at item 3. In front of it
      //    a wave waits for its own pieces of tile t + 1 (requested during stage t - 1; tiles 0
      //    and 1 in the prologue), so behind the barrier of stage t
      //      - tile t + 1 is visible to every wave: its first read is at item 14 of stage t;
      //      - every wave has left stage t - 1 (it passed that stage's item 15 to get here; the
      //        stage's last read of its own slot is at item 10), so slot (t - 1) % 3 = (t + 2) % 3
      //        is free:
      //        the pieces of tile t + 2 go there, one per item, behind that barrier and in front
      //        of the barrier of stage t + 1, which orders them against their first read.
      //    Past the last tile the request repeats the last tile, into a slot nothing reads again
      //    (the two live slots are t % 3 and (t + 1) % 3): no branch inside the item stream.
      //  * Row group 0 of stage t + 1 is read under the last chain of stage t like any next row
      //    group, and the chain of (stage t + 1, item 0) stands in front of the epilogue of
      //    (stage t, item 15): accumulator and A fragments are carried over the loop edge. The
      //    last stage starts such a chain for a stage that is not there (a tail tile's first
      //    items, or a copy of the last tile); its result is dropped, so the one drain is at
      //    the end of the sweep, in front of the tail tile.
      //  * Address registers: two carried per-lane LDS bases and immediate ds_read offsets
      //    (aoff[s] = aoff[0] + 32 s except the last chunk of the rotated rows, which wraps: the
      //    second base), a scalar tile pointer plus one 32-bit lane offset per piece, scalar LDS
      //    destinations.
      //  * Every item is fenced (r9's hand-over: five MFMAs of chain i + 1, a hard fence, then
      //    epilogue i over the rest): unfenced, hipcc reads the next row group's fragments in
      //    front of the chain that still uses their registers and the 7 k-step instance spills.
      // The k order of a chain and the group order of the min chain are the two-slot body's: labels
      // are bit-identical (profiles/r10_sweep_ring).
      constexpr int NI = RG * G, RGB = 32 * C::CPR * 16, HALF = WAVES / 2, HEAD = KS < 5 ? KS : 5;
      unsigned loff[4];  // byte offset of this lane's 16 B inside a tile, per piece round
#pragma unroll
      for (int p = 0; p < 4; ++p) {
        const int q = (p * WAVES + wave) * 64 + lane;
        const int row = q / C::CPR;
        int c = q - row * C::CPR - ((row >> 3) & 1);
        if (c < 0) c += C::CPR;
        loff[p] = (unsigned)(row * C::CPR + c) * 16u;
      }
      auto sweep = [&](auto htag) {
        constexpr int H = decltype(htag)::value;
        int cur = 0, nxt = C::TILE_BYTES, nn = 2 * C::TILE_BYTES;  // slot byte offsets
        // the lane's LDS read bases, carried: they move to the next slot in front of the reads
        // of item 14 (an add of a scalar), the row group inside the slot is an immediate offset
        int ab = aoff0, abL = aoffL;
        auto a_read = [&](int imm, int s) { return *(const bf16x8*)(smem + (s == KS - 1 ? abL : ab) + (imm + 32 * s)); };
        bf16x8 af[2][KS];
        floatx16 acc[2];
        // k-steps s0 .. s1 - 1 of item j's chain into acc[j & 1]. Under the last point group of a
        // row group each A fragment of the next row group (of the next stage's first, from the
        // next slot) is read right behind the MFMA of the same k-step: pinned there by the
        // fences below the fragments need no third buffer
        auto chain = [&](int j, int s0, int s1) {
          const int rgj = j / G, gj = j % G;
          floatx16& a = acc[j & 1];
          if (s0 == 0) {
#pragma unroll
            for (int q = 0; q < 16; ++q) a[q] = 0.f;
            if (gj == G - 1 && rgj + 1 == RG) {
              ab += nxt - cur;
              abL += nxt - cur;
            }
          }
#pragma unroll
          for (int s = s0; s < s1; ++s) {
            a = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[rgj & 1][s], xf[gj][s], a, 0, 0, 0);
            if (gj == G - 1) af[(rgj + 1) & 1][s] = a_read(rgj + 1 < RG ? (rgj + 1) * RGB : 0, s);
          }
        };
#pragma unroll
        for (int s = 0; s < KS; ++s) af[0][s] = a_read(0, s);
        chain(0, 0, KS);
        __builtin_amdgcn_sched_barrier(0);
        for (int t = 0; t < nfull; ++t) {
          const int tq = t + 2 < ntiles ? t + 2 : ntiles - 1;
          const char* gsrc = (const char*)Cm2 + (size_t)tq * C::TILE_BYTES;
#pragma unroll
          for (int i = 0; i < NI; ++i) {
            const int rg = i / G, g = i % G;
            // the first HEAD MFMAs of chain i + 1 stand behind a hard fence, in front of every
            // VALU of epilogue i: with five in front the hazard wait of the epilogue's head is
            // out of the stream (profiles/r9_sweep_pipe)
            chain((i + 1) % NI, 0, HEAD);
            __builtin_amdgcn_sched_barrier(0);
            if (i == KM_RING_BARRIER_ITEM) {
              asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
              __syncthreads();
            }
            constexpr int NP = (C::DMA_INSTR - H * HALF + WAVES - 1) / WAVES;  // piece rounds of this half
            const int p = km_ring_piece_at(H, i);
            if (p >= 0 && p < NP) {
              // the empty asm keeps the zero-extension of the lane offset beside the load, where
              // it folds into the scalar-base address form (hoisted out of the loop it becomes
              // a 64-bit register pair and an add per piece)
              unsigned lo = loff[p];
              asm("" : "+v"(lo));
              __builtin_amdgcn_global_load_lds(
                  (const void __attribute__((address_space(1)))*)(gsrc + (size_t)lo),
                  (void __attribute__((address_space(3)))*)(smem + nn + (p * WAVES + swave) * 1024), 16, 0, 0);
            }
            chain((i + 1) % NI, HEAD, KS);
            tile_argmin(acc[i & 1], g, t * RG + rg);
            // epilogue i (10 VALU) over the rest of chain i + 1, then a second fence
            __builtin_amdgcn_sched_group_barrier(0x002, 2, 0);
#pragma unroll
            for (int s = HEAD; s < KS; ++s) {
              __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
              __builtin_amdgcn_sched_group_barrier(0x002, 4, 0);
            }
            __builtin_amdgcn_sched_barrier(0);
          }
          const int o = cur;
          cur = nxt;
          nxt = nn;
          nn = o;
        }
      };
      if (nfull > 0) {
        if (swave < HALF) sweep(std::integral_constant<int, 0>{});
        else sweep(std::integral_constant<int, 1>{});
      }
      // the last stages' requests: none may land after the workgroup has gone
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    } else
    for (int t = 0; t < nfull; ++t) {
      if (t + 1 < ntiles) stage_dma<C>(Cm2, t + 1, smem + ((t + 1) & 1) * C::TILE_BYTES, swave, lane);
      const char* buf = smem + (t & 1) * C::TILE_BYTES;
      bf16x8 af[2][KS];
#pragma unroll
      for (int s = 0; s < KS; ++s) af[0][s] = a_frag(buf, s);
      if constexpr (PIPE > 0) {
        // software pipeline over the stage's RG*G (row group, point group) items: the MFMA
        // chain of item i+1 stands in front of the argmin epilogue of item i, so most of the
        // epilogue's VALU work sits in the next chain's MFMA gaps. hipcc still puts the head of
        // epilogue i and its hazard wait (s_nop 11) between the two chains; forcing five MFMAs of
        // chain i+1 in front of it with a scheduling fence removes the wait from the stream and
        // measured 0.6 ms of 132 (two waves share the SIMD's matrix pipe and fill each other's
        // holes), too little to keep (profiles/r9_sweep_pipe)
        constexpr int NI = RG * G;
        floatx16 acc[2];
#pragma unroll
        for (int q = 0; q < 16; ++q) acc[0][q] = 0.f;
#pragma unroll
        for (int s = 0; s < KS; ++s) acc[0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[0][s], xf[0][s], acc[0], 0, 0, 0);
#pragma unroll
        for (int i = 0; i < NI; ++i) {
          const int rg = i / G, g = i % G;
          if (g == 0 && rg + 1 < RG) {
            // no LDS read crosses this point (everything else may): read any earlier, the
            // fragments take a third buffer and the keyed 7 k-step instances spill 28 - 44 B
            __builtin_amdgcn_sched_barrier(0x7F);
            const char* nb = buf + (rg + 1) * 32 * C::CPR * 16;
#pragma unroll
            for (int s = 0; s < KS; ++s) af[(rg + 1) & 1][s] = a_frag(nb, s);
          }
          if (i + 1 < NI) {
            const int rg1 = (i + 1) / G, g1 = (i + 1) % G;
            floatx16& an = acc[(i + 1) & 1];
#pragma unroll
            for (int q = 0; q < 16; ++q) an[q] = 0.f;
#pragma unroll
            for (int s = 0; s < KS; ++s) an = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[rg1 & 1][s], xf[g1][s], an, 0, 0, 0);
          }
          tile_argmin(acc[i & 1], g, t * RG + rg);
          if constexpr (PIPE == 2) {
#pragma unroll
            for (int s = 0; s < KS; ++s) {
              __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);  // one MFMA
              __builtin_amdgcn_sched_group_barrier(0x002, 4, 0);  // then up to 4 VALU
            }
          }
        }
      } else
#pragma unroll
      for (int rg = 0; rg < RG; ++rg) {
        if (rg + 1 < RG) {
          const char* nb = buf + (rg + 1) * 32 * C::CPR * 16;
#pragma unroll
          for (int s = 0; s < KS; ++s) af[(rg + 1) & 1][s] = a_frag(nb, s);
        }
        const int tg = t * RG + rg;
#pragma unroll
        for (int g = 0; g < G; ++g) {
          floatx16 acc = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
          for (int s = 0; s < KS; ++s)
            acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[rg & 1][s], xf[g][s], acc, 0, 0, 0);
          tile_argmin(acc, g, tg);
        }
      }
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      __syncthreads();
    }
    if (tail_rg) {
      // K not a multiple of the stage: only the live 32-row groups of the last tile (its DMA
      // landed with the previous stage's wait + barrier; the rows past them are never read)
      const int t = ntiles - 1;
      const char* buf = smem + (t % NSLOT) * C::TILE_BYTES;
      for (int rg = 0; rg < tail_rg; ++rg) {
        const char* nb = buf + rg * 32 * C::CPR * 16;
        bf16x8 af[KS];
#pragma unroll
        for (int s = 0; s < KS; ++s) af[s] = a_frag(nb, s);
        const int tg = t * RG + rg;
#pragma unroll
        for (int g = 0; g < G; ++g) {
          floatx16 acc = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
          for (int s = 0; s < KS; ++s) acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[s], xf[g][s], acc, 0, 0, 0);
          tile_argmin(acc, g, tg);
        }
      }
    }

    // ---- resolve argmin across the two lane halves, write labels / objective partials (the
    // keyed half exchange and the row decode stand in both wide kernels too: change all three)
    // (the lane's ids are derived again from the thread id, so none of them is held over the sweep)
    {
      int tid = threadIdx.x;
      asm volatile("" : "+v"(tid));
      const int lane = tid & 63, wave = tid >> 6, r = lane & 31, h = lane >> 5;
      // the next block of this workgroup; the answer arrives under the epilogue
      unsigned* nextw = (unsigned*)(smem + NSLOT * C::TILE_BYTES + WAVES * 4);
      unsigned fetched = 0;
      if (tid == 0) fetched = gridDim.x + atomicAdd(next_block, 1u);
      // __shfl_xor with this lane id (its own is a hoisted VGPR as well)
      auto lane_xor = [&](auto v, int o) {
        return __builtin_bit_cast(decltype(v), __builtin_amdgcn_ds_bpermute((lane ^ o) << 2, __builtin_bit_cast(int, v)));
      };
      int lab[G];
      float local_obj = 0.f;
#pragma unroll
      for (int g = 0; g < G; ++g) {
        float xs = 0.f;
#pragma unroll
        for (int s = 0; s < KS; ++s)
#pragma unroll
          for (int j = 0; j < 8; ++j) {
            const float v = (float)xf[g][s][j];
            xs = fmaf(v, v, xs);
          }
        xs += lane_xor(xs, 32);
        xs -= (float)KM_ONES;  // the 1.0 columns of X
        const float ob = lane_xor(best[g], 32);
        const int obt = lane_xor(bestt[g], 32);
        // keyless: the smaller value, on equality the lower group (both halves agree)
        const bool take = KEYLESS ? (ob < best[g] || (ob == best[g] && obt < bestt[g]))
                                  : (h ? (ob <= best[g]) : (ob < best[g]));
        const float bv = take ? ob : best[g];
        const int bt = take ? obt : bestt[g];
        const int hw = take ? (1 - h) : h;
        const unsigned reg = __float_as_uint(bv) & 0xFu;
        // keyless: labels[p] is the winning 32-row group id, 0 .. swept_k / 32 - 1
        const int idx = KEYLESS ? bt : bt * 32 + (int)(reg & 3u) + 8 * (int)(reg >> 2) + 4 * hw;
        lab[g] = idx;
        const long p = pbase + g * 32 + r;
        if (h == 0 && p < nb) {
          labels[p] = idx;
          // keyed: the distance without the index bits in its low mantissa (exact where the
          // products are: those four bits of the candidate were cleared when the index went in)
          const float bd = KEYLESS ? bv : __uint_as_float(__float_as_uint(bv) & ~0xFu);
          local_obj += fmaxf(bd + xs, 0.f);
          if (mind) mind[p] = bd + xs;  // squared distance to the chosen centroid (rotation merge)
        }
      }
      if (obj_partial) {
        for (int o = 32; o > 0; o >>= 1) local_obj += lane_xor(local_obj, o);  // wave_sum's order
        float* red = (float*)(smem + NSLOT * C::TILE_BYTES);
        if (lane == 0) red[wave] = local_obj;
        __syncthreads();
        if (tid == 0) {
          float acc = 0.f;
#pragma unroll
          for (int w = 0; w < WAVES; ++w) acc += red[w];
          obj_partial[b] = acc;
        }
      }

      // ---- accumulate (x, 1) rows into the per-centroid partial sums
      if (!KEYLESS && sums) {
#pragma unroll
        for (int g = 0; g < G; ++g) {
          for (int i = 0; i < 32; ++i) {
            const long p = pbase + g * 32 + i;
            if (p >= nb) break;
            const int l = __shfl(lab[g], i, 64);
            const __bf16* xr = X + p * ldx;
            float* sr = sums + (long)l * ld_sums;
            for (int c = lane; c <= dcount; c += 64) atomicAdd(sr + c, (float)xr[c]);
          }
        }
      }
      // One barrier per block edge: behind it the block's last reads of the LDS slots (the tail tile
      // sits in slot (ntiles - 1) % NSLOT, which the next block's first tile overwrites) and of
      // red[] are done, and every wave sees the next block's index
      if (tid == 0) *nextw = fetched;
      __syncthreads();
      b = (long)(unsigned)__builtin_amdgcn_readfirstlane((int)*nextw);
    }
  }
}

// sums[Kr][ld] (column d = count) -> c[Kr][d]; empty clusters keep their old centroid.
__global__ void kmeans_normalize_kernel(const float* __restrict__ sums, int ld, float* __restrict__ c,
                                        int Kr, int d, float* __restrict__ counts) {
  const int row = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (row >= Kr) return;
  const float cnt = sums[(long)row * ld + d];
  if (counts && lane == 0) counts[row] = cnt;
  if (cnt > 0.f) {
    const float inv = 1.0f / cnt;
    for (int j = lane; j < d; j += 64) c[(long)row * d + j] = sums[(long)row * ld + j] * inv;
  }
}

// c[K][d] fp32 -> Cm2[Kp][dp]: cols [0,d) = -2*bf16(c), col d = 0 (count column of X),
// cols d+1..d+3 = ||bf16(c)||^2 split into three bf16 terms (hi + mid + lo ~ 24-bit exact),
// rest 0; cn[Kp] = ||bf16(c)||^2 in fp32. Padding rows: distance +BIG.
__global__ void kmeans_prepare_kernel(const float* __restrict__ c, int K, int d, int Kp, int dp,
                                      __bf16* __restrict__ Cm2, float* __restrict__ cn) {
  const int row = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (row >= Kp) return;
  float s = 0.f;
  for (int j = lane; j < d; j += 64) {
    float v = row < K ? c[(long)row * d + j] : 0.f;
    const float bf = (float)(__bf16)v;
    s = fmaf(bf, bf, s);
    Cm2[(long)row * dp + j] = (__bf16)(-2.0f * bf);
  }
  s = wave_sum(s);
  if (row >= K) s = KM_BIG;
  const __bf16 hi = (__bf16)s;
  const float r1 = s - (float)hi;
  const __bf16 mid = (__bf16)r1;
  const __bf16 lo = (__bf16)(r1 - (float)mid);
  for (int j = d + lane; j < dp; j += 64) {
    __bf16 v = (__bf16)0.f;
    if (j == d + 1) v = hi;
    else if (j == d + 2) v = mid;
    else if (j == d + 3) v = lo;
    Cm2[(long)row * dp + j] = v;
  }
  if (lane == 0) cn[row] = s;
}

// Counter-based uniform generator (splitmix64 of the element index): device-side
// synthetic points like the reference's DataGenRunnable (U[lo,hi)), no host copy.
__device__ __forceinline__ unsigned long long splitmix64(unsigned long long z) {
  z += 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

__global__ void uniform_rows_bf16_kernel(__bf16* __restrict__ X, long N, int d, int dp, float lo,
                                         float hi, unsigned long long seed, long row0, int one_col) {
  const long total = N * (long)dp;
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const long row = i / dp;
    const int col = (int)(i - row * dp);
    float v = 0.f;
    if (col < d) {
      const unsigned long long z = splitmix64(seed ^ ((unsigned long long)(row0 + row) * 0x100000001B3ull + col));
      v = lo + (hi - lo) * (float)((z >> 40) * (1.0 / 16777216.0));
    } else if (one_col && col < d + KM_ONES) {
      v = 1.0f;
    }
    X[i] = (__bf16)v;
  }
}

// ---------------------------------------------------------------------------------------
// Wide rows (dp > 256, any d up to the operand's padding): X fragments no longer fit the
// register file for a whole centroid sweep, so the reduction over features is staged:
//  * a workgroup owns 256 points (4 wave columns of G MFMA point groups of 32) and ONE block
//    of 256 centroids (8 row groups of 32); its accumulators stay live across the feature
//    stages (16 per wave at 4 waves; 8 at 8 waves, where each wave column is two waves with
//    half the row groups each);
//  * feature stage f covers dp columns [64 f, 64 f + 64): the centroid block's 256 x 64 bf16
//    slice streams through LDS by LDS-DMA (the swizzled image of the narrow kernel). The
//    register kernel (variants 1, 3) double-buffers it and loads the points' 64-column
//    slices straight from global into double-buffered registers (next stage's loads in
//    flight under this stage's MFMAs); the ring kernel (variants 5, 6) sends the points'
//    slice through LDS-DMA as well, both into one slot of an NBUF-deep ring;
//  * the epilogue is the narrow kernel's keyed argmin over the wave's candidates, the
//    result (squared distance, index) is merged across waves and centroid blocks with ONE
//    64-bit atomic min per point (distance bits above the index: non-negative floats order
//    as integers, ties go to the lower index);
//  * grid: consecutive ids of one XCD (id mod 8) take the centroid blocks of one point block
//    one after another, so that block's rows come from HBM once and from L2 after.
constexpr int KW_CB = 256, KW_RG = KW_CB / 32;  // centroids per workgroup (8 row groups of 32)

// G point groups of 32 per wave column (4 columns), DC features per stage
template <int G, int DC>
struct KWCfg {
  static constexpr int KS = DC / 16;                  // MFMA k-steps per stage
  static constexpr int CPR = DC / 8;                  // 16-B chunks per row per stage
  static constexpr int TILE_BYTES = KW_CB * DC * 2;   // centroid slice per stage
  static constexpr int DMA = KW_CB * CPR / 64;        // its 1-KiB DMA pieces
  static constexpr int PTS = 4 * G * 32;              // points per workgroup
  static constexpr int XBYTES = PTS * DC * 2;         // point slice per stage (ring kernel)
  static constexpr int XDMA = PTS * CPR / 64;         // its 1-KiB DMA pieces
};

// XCD-aware blockIdx -> (point block pb, centroid block kb): ids x, x + 8, x + 16, ... (one
// XCD) walk the nkb centroid blocks of one point block before the next. valid is false for
// the ids of a last round of 8 that name no point block: those workgroups return at once.
// row0() is the block's first centroid row, live_blk() its row groups below kswept; they are
// derived after that return (computed in front of it, the kernels' code changes).
struct KWBlock {
  long pb;
  int kb;
  bool valid;
  __device__ int row0() const { return kb * KW_CB; }
  __device__ int live_blk(int kswept) const {
    return (kswept - row0()) >= KW_CB ? KW_RG : (kswept - row0() + 31) / 32;
  }
};
template <int PTS>
__device__ __forceinline__ KWBlock wide_block(long N, int nkb) {
  const long id = blockIdx.x;
  const long xcd = id & 7, round = id >> 3;
  const long pb = (round / nkb) * 8 + xcd;
  const int kb = (int)(round % nkb);
  const long npb = (N + PTS - 1) / PTS;
  return {pb, kb, pb < npb};
}

// LDS chunk rotation of centroid row `row` for the wide tiles: ds_read_b128 serves 16 lanes
// (rows r..r+15 of one 16-B chunk column) per LDS cycle, so their 16 addresses must fall on
// 16 distinct 16-B slots of a 256-B bank row. With 128-B rows (CPR 8) rows r and r + 2
// alias, so the rotation walks r >> 1; with 256-B rows (CPR 16) every row aliases, so it
// walks r.
template <int CPR>
__device__ __forceinline__ int wide_rot(int row) {
  return CPR == 4 ? (row >> 2) & 3 : CPR == 8 ? (row >> 1) & 7 : CPR == 16 ? row & 15 : (row >> 3) & 1;
}

// stage f of the centroid block at row0 -> its rotated LDS image, by all WAVES waves
template <class C, int WAVES>
__device__ __forceinline__ void stage_dma_wide(const __bf16* __restrict__ cm2, int dp, int row0, int kp, int f,
                                               char* lds, int wave, int lane) {
  static_assert(C::DMA % WAVES == 0, "whole pieces per wave");
#pragma unroll
  for (int j0 = 0; j0 < C::DMA; j0 += WAVES) {
    const int j = j0 + wave;
    const int q = j * 64 + lane;
    const int row = q / C::CPR;
    int c = q - row * C::CPR - wide_rot<C::CPR>(row);
    if (c < 0) c += C::CPR;
    int gr = row0 + row;
    if (gr > kp - 1) gr = kp - 1;  // past the padded rows: a valid address, never read
    const __bf16* src = cm2 + (size_t)gr * dp + f * (C::CPR * 8) + c * 8;
    __builtin_amdgcn_global_load_lds((const void __attribute__((address_space(1)))*)src,
                                     (void __attribute__((address_space(3)))*)(lds + j * 1024), 16, 0, 0);
  }
}

// The register kernel: 4 waves, each all 8 row groups x G point groups; OCC waves per SIMD
template <int G, int DC, int OCC>
__global__ __launch_bounds__(256, OCC) void kmeans_assign_wide_kernel(
    const __bf16* __restrict__ X, long ldx, const __bf16* __restrict__ Cm2, long N, int dp, int kswept, int kp,
    int nkb, unsigned long long* __restrict__ keys) {
  using C = KWCfg<G, DC>;
  constexpr int KS = C::KS;
  __shared__ __attribute__((aligned(16))) char smem[2 * C::TILE_BYTES];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int r = lane & 31, h = lane >> 5;
  const KWBlock b = wide_block<C::PTS>(N, nkb);
  if (!b.valid) return;
  const int row0 = b.row0(), live_rg = b.live_blk(kswept);
  const long pbase = b.pb * C::PTS + wave * (G * 32);
  const int nst = dp / DC;

  stage_dma_wide<C, 4>(Cm2, dp, row0, kp, 0, smem, wave, lane);
  const bf16x8* xrow[G];
#pragma unroll
  for (int g = 0; g < G; ++g) {
    long p = pbase + g * 32 + r;
    if (p > N - 1) p = N - 1;
    xrow[g] = (const bf16x8*)(X + p * ldx);
  }
  bf16x8 xf[2][G][KS];  // [buffer][point group][k-step]
#pragma unroll
  for (int g = 0; g < G; ++g)
#pragma unroll
    for (int k = 0; k < KS; ++k) xf[0][g][k] = xrow[g][2 * k + h];
  floatx16 acc[KW_RG][G];
#pragma unroll
  for (int a = 0; a < KW_RG; ++a)
#pragma unroll
    for (int g = 0; g < G; ++g)
#pragma unroll
      for (int q = 0; q < 16; ++q) acc[a][g][q] = 0.f;
  int aoff[KS];
#pragma unroll
  for (int k = 0; k < KS; ++k) {
    const int cp = (2 * k + h + wide_rot<C::CPR>(r)) % C::CPR;
    aoff[k] = (r * C::CPR + cp) * 16;
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  // one feature stage; the register buffer index is a template constant (a runtime index
  // into xf would put the fragments in scratch)
  auto stage = [&](int f, auto curtag) {
    constexpr int cur = decltype(curtag)::value;
    if (f + 1 < nst) {
      stage_dma_wide<C, 4>(Cm2, dp, row0, kp, f + 1, smem + (cur ^ 1) * C::TILE_BYTES, wave, lane);
#pragma unroll
      for (int g = 0; g < G; ++g)
#pragma unroll
        for (int k = 0; k < KS; ++k) xf[cur ^ 1][g][k] = xrow[g][(f + 1) * C::CPR + 2 * k + h];
    }
    const char* buf = smem + cur * C::TILE_BYTES;
    bf16x8 af[2][KS];
#pragma unroll
    for (int k = 0; k < KS; ++k) af[0][k] = *(const bf16x8*)(buf + aoff[k]);
#pragma unroll
    for (int rg = 0; rg < KW_RG; ++rg) {
      if (rg + 1 < KW_RG) {
        const char* nb = buf + (rg + 1) * 32 * C::CPR * 16;
#pragma unroll
        for (int k = 0; k < KS; ++k) af[(rg + 1) & 1][k] = *(const bf16x8*)(nb + aoff[k]);
      }
      if (rg < live_rg) {
#pragma unroll
        for (int g = 0; g < G; ++g)
#pragma unroll
          for (int k = 0; k < KS; ++k)
            acc[rg][g] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[rg & 1][k], xf[cur][g][k], acc[rg][g], 0, 0, 0);
      }
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
  };
  for (int f = 0; f < nst; f += 2) {
    stage(f, std::integral_constant<int, 0>{});
    if (f + 1 < nst) stage(f + 1, std::integral_constant<int, 1>{});
  }
  // |x|^2 per point group, from global once after the sweep (L2-warm rows)
  float xsg[G];
#pragma unroll
  for (int g = 0; g < G; ++g) {
    float t = 0.f;
    for (int c = h; c < dp / 8; c += 2) {
      const bf16x8 v = xrow[g][c];
#pragma unroll
      for (int j = 0; j < 8; ++j) t = fmaf((float)v[j], (float)v[j], t);
    }
    t += __shfl_xor(t, 32, 64);
    xsg[g] = t - (float)KM_ONES;
  }
  // epilogue: keyed min over the live row groups, half exchange (the lower half wins equal
  // keys), row decode, one 64-bit atomic min per point. The ring kernel below and the narrow
  // kernel above hold the same lines: as a shared function they compile to other code in every
  // kernel that calls it (profiles/r8_kwide_refactor), so a change goes into all three.
#pragma unroll
  for (int g = 0; g < G; ++g) {
    float best = KM_BIG;
    int bestt = 0;
#pragma unroll
    for (int rg = 0; rg < KW_RG; ++rg) {
      if (rg >= live_rg) break;
      float m = keyed(acc[rg][g][0], 0u);
#pragma unroll
      for (int q = 1; q < 16; ++q) m = fminf(m, keyed(acc[rg][g][q], (unsigned)q));
      if (m < best) {
        best = m;
        bestt = rg;
      }
    }
    const float ob = __shfl_xor(best, 32, 64);
    const int obt = __shfl_xor(bestt, 32, 64);
    const bool take = h ? (ob <= best) : (ob < best);
    const float bv = take ? ob : best;
    const int bt = take ? obt : bestt;
    const int hw = take ? (1 - h) : h;
    const unsigned reg = __float_as_uint(bv) & 0xFu;
    const int idx = row0 + bt * 32 + (int)(reg & 3u) + 8 * (int)(reg >> 2) + 4 * hw;
    const long p = pbase + g * 32 + r;
    if (h == 0 && p < N) {
      const float dist = fmaxf(bv + xsg[g], 0.f);
      const unsigned long long key = ((unsigned long long)__float_as_uint(dist) << 32) | (unsigned)idx;
      __hip_atomic_fetch_min(keys + p, key, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  }
}

// The ring kernel: both operands through an NBUF-deep LDS-DMA ring. WAVES = 4: wave w takes
// all 8 row groups x point column w (8 x G accumulators). WAVES = 8 (2 per SIMD) on the same
// 256 x 256 tile: wave w takes centroid half w & 1 and point column w >> 1 (4 x G
// accumulators), so each SIMD has a second wave to issue while one waits (the 4-wave form
// parks 44 % of its cycles on instruction dependencies).
template <int G, int DC, int NBUF, int WAVES>
__global__ __launch_bounds__(WAVES * 64, 1) void kmeans_assign_wide_ring_kernel(
    const __bf16* __restrict__ X, long ldx, const __bf16* __restrict__ Cm2, long N, int dp, int kswept, int kp,
    int nkb, unsigned long long* __restrict__ keys) {
  using C = KWCfg<G, DC>;
  constexpr int KS = C::KS, CPR = C::CPR;
  constexpr int CW = WAVES / 4;                       // waves per point column, one centroid share each
  constexpr int RGW = KW_RG / CW;                     // row groups per wave
  constexpr int SBYTES = C::TILE_BYTES + C::XBYTES;   // one ring slot
  constexpr int OPS = (C::DMA + C::XDMA) / WAVES;     // DMA instructions per wave per stage
  static_assert(WAVES == 4 || WAVES == 8, "4 point columns x 1 or 2 centroid shares");
  __shared__ __attribute__((aligned(16))) char smem[NBUF * SBYTES];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int r = lane & 31, h = lane >> 5;
  const int rgo = (wave % CW) * RGW;                  // first row group of this wave
  const int pw = wave / CW;                           // point column of this wave
  const KWBlock b = wide_block<C::PTS>(N, nkb);
  if (!b.valid) return;
  const int row0 = b.row0();
  // this wave's share of the block's live row groups (one wave per column: all of them)
  const int live_blk = b.live_blk(kswept);
  const int live_rg = CW == 1 ? live_blk : (live_blk - rgo < 0 ? 0 : (live_blk - rgo > RGW ? RGW : live_blk - rgo));
  const long p0 = b.pb * C::PTS;  // first point of the workgroup
  const long pbase = p0 + pw * (G * 32);
  const int nst = dp / DC;
  auto issue = [&](int f, int slot) {
    char* buf = smem + slot * SBYTES;
    stage_dma_wide<C, WAVES>(Cm2, dp, row0, kp, f, buf, wave, lane);
    char* xb = buf + C::TILE_BYTES;
#pragma unroll
    for (int j0 = 0; j0 < C::XDMA; j0 += WAVES) {
      const int j = j0 + wave;
      const int q = j * 64 + lane;
      const int row = q / CPR;
      int c = q - row * CPR - wide_rot<CPR>(row);
      if (c < 0) c += CPR;
      long pr = p0 + row;
      if (pr > N - 1) pr = N - 1;
      const __bf16* src = X + pr * ldx + f * DC + c * 8;
      __builtin_amdgcn_global_load_lds((const void __attribute__((address_space(1)))*)src,
                                       (void __attribute__((address_space(3)))*)(xb + j * 1024), 16, 0, 0);
    }
  };
  floatx16 acc[RGW][G];
#pragma unroll
  for (int a = 0; a < RGW; ++a)
#pragma unroll
    for (int g = 0; g < G; ++g)
#pragma unroll
      for (int q = 0; q < 16; ++q) acc[a][g][q] = 0.f;
  int aoff[KS];
#pragma unroll
  for (int k = 0; k < KS; ++k) aoff[k] = (r * CPR + (2 * k + h + wide_rot<CPR>(r)) % CPR) * 16;
#pragma unroll
  for (int q = 0; q < NBUF - 1; ++q)
    if (q < nst) issue(q, q);
  float xs[G];
#pragma unroll
  for (int g = 0; g < G; ++g) xs[g] = 0.f;
  for (int f = 0; f < nst; ++f) {
    // stage f landed when at most the younger stages' pieces are outstanding
    const int younger = (nst - 1 - f) < (NBUF - 2) ? (nst - 1 - f) : (NBUF - 2);
    if (younger >= 2) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(2 * OPS) : "memory");
    else if (younger == 1) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(OPS) : "memory");
    else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (f + NBUF - 1 < nst) issue(f + NBUF - 1, (f + NBUF - 1) % NBUF);
    const char* buf = smem + (f % NBUF) * SBYTES;
    const char* xb = buf + C::TILE_BYTES + pw * (G * 32) * CPR * 16;
    const char* cb = buf + rgo * 32 * CPR * 16;
    bf16x8 xf[G][KS];
#pragma unroll
    for (int g = 0; g < G; ++g)
#pragma unroll
      for (int k = 0; k < KS; ++k) xf[g][k] = *(const bf16x8*)(xb + g * 32 * CPR * 16 + aoff[k]);
    // |x|^2 from the staged fragments (VALU work under the stage's MFMAs)
#pragma unroll
    for (int g = 0; g < G; ++g)
#pragma unroll
      for (int k = 0; k < KS; ++k)
#pragma unroll
        for (int j = 0; j < 8; ++j) xs[g] = fmaf((float)xf[g][k][j], (float)xf[g][k][j], xs[g]);
    bf16x8 af[2][KS];
#pragma unroll
    for (int k = 0; k < KS; ++k) af[0][k] = *(const bf16x8*)(cb + aoff[k]);
#pragma unroll
    for (int rg = 0; rg < RGW; ++rg) {
      if (rg + 1 < RGW) {
        const char* nb = cb + (rg + 1) * 32 * CPR * 16;
#pragma unroll
        for (int k = 0; k < KS; ++k) af[(rg + 1) & 1][k] = *(const bf16x8*)(nb + aoff[k]);
      }
      if (rg < live_rg) {
#pragma unroll
        for (int g = 0; g < G; ++g)
#pragma unroll
          for (int k = 0; k < KS; ++k)
            acc[rg][g] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[rg & 1][k], xf[g][k], acc[rg][g], 0, 0, 0);
      }
    }
  }
  float xsg[G];
#pragma unroll
  for (int g = 0; g < G; ++g) xsg[g] = xs[g] + __shfl_xor(xs[g], 32, 64) - (float)KM_ONES;
  // epilogue: the register kernel's, over this wave's row groups rgo .. rgo + RGW - 1; with two
  // waves per column a wave without a live row group posts no key
#pragma unroll
  for (int g = 0; g < G; ++g) {
    float best = KM_BIG;
    int bestt = 0;
#pragma unroll
    for (int rg = 0; rg < RGW; ++rg) {
      if (rg >= live_rg) break;
      float m = keyed(acc[rg][g][0], 0u);
#pragma unroll
      for (int q = 1; q < 16; ++q) m = fminf(m, keyed(acc[rg][g][q], (unsigned)q));
      if (m < best) {
        best = m;
        bestt = rg;
      }
    }
    const float ob = __shfl_xor(best, 32, 64);
    const int obt = __shfl_xor(bestt, 32, 64);
    const bool take = h ? (ob <= best) : (ob < best);
    const float bv = take ? ob : best;
    const int bt = take ? obt : bestt;
    const int hw = take ? (1 - h) : h;
    const unsigned reg = __float_as_uint(bv) & 0xFu;
    const int idx = row0 + (rgo + bt) * 32 + (int)(reg & 3u) + 8 * (int)(reg >> 2) + 4 * hw;
    const long p = pbase + g * 32 + r;
    if (h == 0 && p < N && (CW == 1 || live_rg > 0)) {
      const float dist = fmaxf(bv + xsg[g], 0.f);
      const unsigned long long key = ((unsigned long long)__float_as_uint(dist) << 32) | (unsigned)idx;
      __hip_atomic_fetch_min(keys + p, key, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  }
}

// a wide tiling's entry point with the shape it is launched at, named together so that the
// two cannot be paired wrongly at the call
struct WideTiling {
  void (*kernel)(const __bf16*, long, const __bf16*, long, int, int, int, int, unsigned long long*);
  int waves, pts, dc;  // waves and points per workgroup, features per stage
};
template <int G, int DC, int OCC>
constexpr WideTiling wide_reg{kmeans_assign_wide_kernel<G, DC, OCC>, 4, KWCfg<G, DC>::PTS, DC};
template <int G, int DC, int NBUF, int WAVES>
constexpr WideTiling wide_ring{kmeans_assign_wide_ring_kernel<G, DC, NBUF, WAVES>, WAVES, KWCfg<G, DC>::PTS, DC};

// one launcher for every wide tiling
int launch_wide(const WideTiling& t, const void* X, long ldx, const void* Cm2, long N, int dp, int kswept, int kp,
                unsigned long long* keys, hipStream_t s) {
  if (dp % t.dc) return HARP_EBADARG;
  const long npb = (N + t.pts - 1) / t.pts;
  const int nkb = (kswept + KW_CB - 1) / KW_CB;
  const long rounds = (npb + 7) / 8 * nkb;
  t.kernel<<<dim3((unsigned)(rounds * 8)), dim3(t.waves * 64), 0, s>>>((const __bf16*)X, ldx, (const __bf16*)Cm2, N,
                                                                      dp, kswept, kp, nkb, keys);
  return harp_launch_status();
}

// keys -> labels, squared distances, per-block objective partials (256 points per block)
__global__ __launch_bounds__(256) void kmeans_wide_finish_kernel(const unsigned long long* __restrict__ keys, long N,
                                                                 int* __restrict__ labels, float* __restrict__ obj_partial,
                                                                 float* __restrict__ mind) {
  __shared__ float red[4];
  const long p = blockIdx.x * 256L + threadIdx.x;
  float v = 0.f;
  if (p < N) {
    const unsigned long long k = keys[p];
    labels[p] = (int)(k & 0xffffffffull);
    v = __uint_as_float((unsigned)(k >> 32));
    if (mind) mind[p] = v;
  }
  v = wave_sum(v);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  if (threadIdx.x == 0 && obj_partial) obj_partial[blockIdx.x] = red[0] + red[1] + red[2] + red[3];
}

// harp_kmeans_set_resident_blocks: 0 = every instantiation's own resident grid
std::atomic<int> km_resident_override{0};

// The words the resident grids take their next point block from, one per launch in flight:
// launches take them round robin and zero theirs in stream order in front of the kernel, so a
// word is shared only by launches KM_NEXT_WORDS apart, which would have to overlap on two streams.
constexpr int KM_NEXT_WORDS = 1024;
__device__ unsigned km_next_block_words[KM_NEXT_WORDS];
std::atomic<unsigned> km_next_word{0};

// this launch's word, zeroed on the stream; nullptr if the runtime refuses
unsigned* next_block_word(hipStream_t stream) {
  unsigned* base = nullptr;
  if (hipGetSymbolAddress((void**)&base, HIP_SYMBOL(km_next_block_words)) != hipSuccess || !base) return nullptr;
  unsigned* w = base + km_next_word.fetch_add(1, std::memory_order_relaxed) % KM_NEXT_WORDS;
  return hipMemsetAsync(w, 0, sizeof(unsigned), stream) == hipSuccess ? w : nullptr;
}

// Workgroups of one assign instantiation the current device holds at once: CUs x the
// occupancy of that kernel (1 at 7 k-steps: 256 VGPRs and 86 KB of LDS), asked for once per
// instantiation and device. 0 if the runtime cannot say.
template <int KS, int G, int WAVES, int RG, int PIPE, int PRIO, int KEYLESS, int RINGK>
int assign_resident_blocks() {
  constexpr int MAXDEV = 64;
  static std::atomic<int> cache[MAXDEV];
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= MAXDEV) return 0;
  int res = cache[dev].load(std::memory_order_relaxed);
  if (res > 0) return res;
  int per = 0, cus = 0;
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per, kmeans_assign_kernel<KS, G, WAVES, RG, PIPE, PRIO, KEYLESS, RINGK>,
                                                   WAVES * 64, 0) != hipSuccess ||
      hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || per <= 0 || cus <= 0)
    return 0;
  res = per * cus;
  cache[dev].store(res, std::memory_order_relaxed);
  return res;
}

// the ring sweep spills at 8 k-steps (660 B): that instance keeps the two-slot body
template <int KS, int RING>
constexpr int km_ring_at = RING && KS <= 7;

template <int KS, int G, int WAVES, int RG, int PIPE = 0, int PRIO = 0, int KEYLESS = 0, int RING = 0>
int launch_assign(const void* X, long ldx, const void* Cm2, long N, int Kp, int d, int* labels, float* sums,
                  int ld_sums, float* obj_partial, float* mind, hipStream_t stream) {
  using C = KMCfg<KS, G, WAVES, RG>;
  if (Kp % 32 || (KEYLESS && sums)) return HARP_EBADARG;  // no fused atomics in the keyless sweep
  const long nblk = (N + C::PTS - 1) / C::PTS;
  const int ntiles = (Kp + C::TILE - 1) / C::TILE, tail_rg = (Kp % C::TILE) / 32;
  constexpr int RINGK = km_ring_at<KS, RING>;
  // a resident grid: the workgroups loop over the point blocks (kernel comment)
  int resident = km_resident_override.load(std::memory_order_relaxed);
  if (resident <= 0) resident = assign_resident_blocks<KS, G, WAVES, RG, PIPE, PRIO, KEYLESS, RINGK>();
  if (resident <= 0) return HARP_ELAUNCH;
  const long grid = nblk < resident ? nblk : resident;
  if (nblk + grid >= (1L << 32)) return HARP_EUNSUPPORTED;  // block indices are handed out as 32-bit words
  unsigned* next = next_block_word(stream);
  if (!next) return HARP_ELAUNCH;
  kmeans_assign_kernel<KS, G, WAVES, RG, PIPE, PRIO, KEYLESS, RINGK><<<dim3((unsigned)grid), dim3(C::THREADS), 0, stream>>>(
      (const __bf16*)X, ldx, (const __bf16*)Cm2, N, ntiles, tail_rg, d, labels, sums, ld_sums, obj_partial, mind, nblk, next);
  return harp_launch_status();
}

// variant -> (G, WAVES, RG, PIPE, PRIO, KEYLESS, RING), the one table both the launch and
// harp_kmeans_points_per_block read. Kp (the rows swept) must be a multiple of 32; Cm2 must
// hold round_up(Kp, 128) rows (the last stage's DMA reads the whole tile).
// Only the measured frontier ships (profiles/r1_kmeans_*): 15 (= 14 + static priority for the
// younger half, profiles/r3_setprio) is the default for d <= 124, 13 the RG=2 neighbour of 14,
// 4 the one-group shape wide rows (9..16 k-steps) use. 16 is 15 without index keys: it writes
// the winning 32-row group id (0 .. Kp / 32 - 1) to labels and takes no fused sums; the
// caller finishes the labels with harp_kmeans_resolve_rowsum (kmeans_resolve.hip). The
// default for rows of <= 128 padded columns with bucketed sums (profiles/r7_keyless). Its
// sweep is the ring form (three LDS slots, the item pipeline carried over the stage edge;
// profiles/r10_sweep_ring) at 1..7 k-steps; at 8 that form spills, and the instance keeps the
// two-slot body the keyed variants run.
#define KM_VARIANT_TABLE(ROW, KS)       \
  ROW(KS, 4, 1, 16, 2, 0, 0, 0, 0)      \
  ROW(KS, 13, 4, 8, 2, 2, 0, 0, 0)      \
  ROW(KS, 14, 4, 8, 4, 2, 0, 0, 0)      \
  ROW(KS, 15, 4, 8, 4, 2, 1, 0, 0)      \
  ROW(KS, 16, 4, 8, 4, 2, 1, 1, 1)
#define KM_LAUNCH_ROW(KS, V, G, WAVES, RG, PIPE, PRIO, KEYLESS, RING) \
  case V: return launch_assign<KS, G, WAVES, RG, PIPE, PRIO, KEYLESS, RING>(X, ldx, Cm2, N, Kp, d, labels, sums, ld, op, md, s);
#define KM_PTS_ROW(KS, V, G, WAVES, RG, PIPE, PRIO, KEYLESS, RING) \
  case V: return KMCfg<KS, G, WAVES, RG>::PTS;
#define KM_RESIDENT_ROW(KS, V, G, WAVES, RG, PIPE, PRIO, KEYLESS, RING) \
  case V: return assign_resident_blocks<KS, G, WAVES, RG, PIPE, PRIO, KEYLESS, km_ring_at<KS, RING>>();
#define KM_RESIDENT(KS)                      \
  switch (variant) {                         \
    KM_VARIANT_TABLE(KM_RESIDENT_ROW, KS)    \
    default: return -1;                      \
  }
#define KM_VARIANTS(KS)                      \
  switch (variant) {                         \
    KM_VARIANT_TABLE(KM_LAUNCH_ROW, KS)      \
    default: return HARP_EBADARG;            \
  }

}  // namespace

HARP_EXPORT int harp_kmeans_points_per_block(int variant) {
  switch (variant) {
    KM_VARIANT_TABLE(KM_PTS_ROW, 1)  // PTS does not depend on the k-steps
    default: return -1;
  }
}

// Workgroups harp_kmeans_assign launches at most for (variant, ksteps = dp / 16 in 1..8) on the
// current device: the resident grid, which loops over the point blocks. 0 if the runtime
// cannot say, -1 for a pair that is not in the table.
HARP_EXPORT int harp_kmeans_resident_blocks(int variant, int ksteps) {
  switch (ksteps) {
    case 1: KM_RESIDENT(1)
    case 2: KM_RESIDENT(2)
    case 3: KM_RESIDENT(3)
    case 4: KM_RESIDENT(4)
    case 5: KM_RESIDENT(5)
    case 6: KM_RESIDENT(6)
    case 7: KM_RESIDENT(7)
    case 8: KM_RESIDENT(8)
    default: return -1;
  }
}

// n > 0: every assign launch takes min(point blocks, n) workgroups (tests force 1, 2, 3);
// 0: back to the resident grid. Process-wide.
HARP_EXPORT int harp_kmeans_set_resident_blocks(int n) {
  if (n < 0) return HARP_EBADARG;
  km_resident_override.store(n, std::memory_order_relaxed);
  return HARP_OK;
}

// X rows of dp (MFMA k) elements at a row stride of ldx >= dp elements (ldx % 8 == 0: 16-B
// aligned rows; a 256-B multiple makes every row whole 128-B lines for the gather-sum).
HARP_EXPORT int harp_kmeans_assign(const void* X, long ldx, const void* Cm2, long N, int dp, int Kp, int d,
                                   int* labels, float* sums, int ld, float* op, float* md, int variant,
                                   hipStream_t s) {
  if (N <= 0 || d + KM_ONES > dp || dp % 16 || Kp <= 0 || Kp % 32 || ldx < dp || ldx % 8) return HARP_EBADARG;
  switch (dp / 16) {
    case 1: KM_VARIANTS(1)
    case 2: KM_VARIANTS(2)
    case 3: KM_VARIANTS(3)
    case 4: KM_VARIANTS(4)
    case 5: KM_VARIANTS(5)
    case 6: KM_VARIANTS(6)
    case 7: KM_VARIANTS(7)
    case 8: KM_VARIANTS(8)
    // wide rows: one 32-point group per wave keeps the X fragments within budget
#define KM_WIDE(KSV) case KSV: return launch_assign<KSV, 1, 16, 2>(X, ldx, Cm2, N, Kp, d, labels, sums, ld, op, md, s);
    KM_WIDE(9) KM_WIDE(10) KM_WIDE(11) KM_WIDE(12) KM_WIDE(13) KM_WIDE(14) KM_WIDE(15) KM_WIDE(16)
#undef KM_WIDE
    default: return HARP_EUNSUPPORTED;
  }
}

// Wide rows (dp > 256, dp % 64 == 0): keys (N uint64, filled with ~0 by the caller) take the
// per-point (distance, index) minimum over all centroid blocks; harp_kmeans_wide_finish then
// writes labels / distances / objective partials (one per 256 points). variant: 0 = 6 (the
// ring kernel: both operands through LDS-DMA into a 256 x 256 tile, 8 waves = 2 per SIMD,
// each 128 centroids x 64 points); 5 = the same kernel with 4 waves (256 centroids x 64
// points each); 1 / 3 = the register kernel, point fragments loaded straight into registers
// (2 groups at 1 wave / SIMD, 1 group at 2).
// Measured at N = 1e7, K = 1e3 (profiles/r4_kwide): d = 1000 6 and 5 both 0.98 PF useful,
// d = 512 6 at 0.86 vs 5 at 0.81 PF; 1 / 3 at 0.56 / 0.61 (waves parked 52-66 % of their
// cycles on 32-row-per-instruction point loads); 128-feature stages, a 3-deep register
// pipeline, 32-feature stages with 3- and 4-deep LDS rings, one group per wave with a 3-deep
// ring, a persistent stage stream across tiles and square 128 x 128 per-wave tiles all
// measured 0.44-0.93 PF and were removed.
HARP_EXPORT int harp_kmeans_assign_wide(const void* X, long ldx, const void* Cm2, long N, int dp, int kswept, int kp,
                                        int d, unsigned long long* keys, int variant, hipStream_t s) {
  if (N <= 0 || d + KM_ONES > dp || dp % 64 || dp <= 0 || kswept <= 0 || kswept % 32 || kp < kswept ||
      ldx < dp || ldx % 8 || !keys)
    return HARP_EBADARG;
  if (variant == 0) variant = 6;
  switch (variant) {
    case 1: return launch_wide(wide_reg<2, 64, 1>, X, ldx, Cm2, N, dp, kswept, kp, keys, s);
    case 3: return launch_wide(wide_reg<1, 64, 2>, X, ldx, Cm2, N, dp, kswept, kp, keys, s);
    case 5: return launch_wide(wide_ring<2, 64, 2, 4>, X, ldx, Cm2, N, dp, kswept, kp, keys, s);
    case 6: return launch_wide(wide_ring<2, 64, 2, 8>, X, ldx, Cm2, N, dp, kswept, kp, keys, s);
    default: return HARP_EBADARG;
  }
}

HARP_EXPORT int harp_kmeans_wide_finish(const unsigned long long* keys, long N, int* labels, float* obj_partial,
                                        float* mind, hipStream_t s) {
  if (N <= 0) return HARP_OK;
  kmeans_wide_finish_kernel<<<dim3((unsigned)((N + 255) / 256)), dim3(256), 0, s>>>(keys, N, labels, obj_partial, mind);
  return harp_launch_status();
}

HARP_EXPORT int harp_kmeans_normalize(const float* sums, int ld, float* c, int Kr, int d, float* counts,
                                      hipStream_t s) {
  if (Kr <= 0) return HARP_OK;
  const int wpb = 4;
  kmeans_normalize_kernel<<<dim3((Kr + wpb - 1) / wpb), dim3(64 * wpb), 0, s>>>(sums, ld, c, Kr, d, counts);
  return harp_launch_status();
}

HARP_EXPORT int harp_kmeans_prepare(const float* c, int K, int d, int Kp, int dp, void* Cm2, float* cn,
                                    hipStream_t s) {
  if (Kp < K || dp < d) return HARP_EBADARG;
  const int wpb = 4;
  kmeans_prepare_kernel<<<dim3((Kp + wpb - 1) / wpb), dim3(64 * wpb), 0, s>>>(c, K, d, Kp, dp, (__bf16*)Cm2, cn);
  return harp_launch_status();
}

HARP_EXPORT int harp_uniform_rows_bf16(void* X, long N, int d, int dp, float lo, float hi,
                                       unsigned long long seed, long row0, int one_col, hipStream_t s) {
  if (N <= 0) return HARP_OK;
  long blocks = (N * (long)dp + 255) / 256;
  if (blocks > 65536) blocks = 65536;
  uniform_rows_bf16_kernel<<<dim3((unsigned)blocks), dim3(256), 0, s>>>((__bf16*)X, N, d, dp, lo, hi, seed, row0,
                                                                       one_col);
  return harp_launch_status();
}
