// Parameter-server row slots (device only): the wire format of the sparse push / pull of count
// rows, written by the row codec (rowcodec.hip) and read / written in place by the fused LDA
// samplers (lda.hip).
//
// Payload of one peer = a sequence of per-row SLOTS at static byte offsets. A slot's
// capacity comes from token totals that never change during sampling (pull: min(K, global
// tokens of the word); push delta: min(K, 2 x local tokens)), so both ends derive the same
// layout once and every call is a fixed-size all-to-all with no size exchange and no host
// sync. A slot is
//   sparse (cap >= 0): [int32 nnz][int32 counts cap][uint16 topics cap]   (4 + 6 cap bytes, 4-aligned)
//   dense  (cap <  0): [int32 row K]                      (16-aligned; when 4 + 6 cap >= 4 K)
// Entries past nnz are never read; topic order within a slot is free.
#pragma once

namespace ps_slot {

__device__ __forceinline__ const int* nnz_word(const unsigned char* slot) { return (const int*)slot; }
__device__ __forceinline__ int* nnz_word(unsigned char* slot) { return (int*)slot; }
__device__ __forceinline__ const int* counts(const unsigned char* slot) { return (const int*)(slot + 4); }
__device__ __forceinline__ int* counts(unsigned char* slot) { return (int*)(slot + 4); }
__device__ __forceinline__ const unsigned short* topics(const unsigned char* slot, int cap) {
  return (const unsigned short*)(slot + 4 + 4 * (long)cap);
}
__device__ __forceinline__ unsigned short* topics(unsigned char* slot, int cap) {
  return (unsigned short*)(slot + 4 + 4 * (long)cap);
}

// entries of a received slot: the nnz word clamped to the slot (payloads are bounds-checked)
__device__ __forceinline__ int nnz(const unsigned char* slot, int cap) {
  const int n = *nnz_word(slot);
  return n < 0 ? 0 : (n > cap ? cap : n);
}
// the nnz word of a slot whose writer placed `total` entries (those past cap were dropped)
__device__ __forceinline__ void set_nnz(unsigned char* slot, int cap, int total) {
  *nnz_word(slot) = total < cap ? total : cap;
}

// entry pos := (topic, value); true (nothing written) when pos is past the capacity: the slot
// overflowed, the caller raises its overflow flag
__device__ __forceinline__ bool put(unsigned char* slot, int cap, int pos, int topic, int value) {
  if (pos >= cap) return true;
  counts(slot)[pos] = value;
  topics(slot, cap)[pos] = (unsigned short)topic;
  return false;
}

}  // namespace ps_slot
