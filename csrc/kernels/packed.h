// The two packed 64-bit formats of the histogram hot path (seg.hip, hist5.hip), defined once.  This comment is
// the layout's only prose description; cdnaml/ops/kernels.py names the same numbers (REC_* / PACK_*).
//
// Quantised label: qb = clamp(rint(v1 * qs1), +-2^23) + 2^23, in [0, 2^24] (25 bits, never negative).
//
// Item record (one per (row, tree) item of a built node; codes_compact / node_compact / codes_scatter_* and the
// root kernels' rings write it, the record histograms read it):
//     bits  0..30  row      (the record paths need n < 2^31 rows per rank)
//     bits 31..38  weight   (bootstrap weight, <= 255)
//     bits 39..63  qb       (the top value 2^24 sets bit 63: as int64 the word is negative)
//
// LDS cell (one ds_add_u64 per update): bits 0..43 the sum of w * qb over the cell's items, bits 44..63 their
// count = sum of w.  An item adds  w << 44 | w * qb : no carry between the fields while the host keeps a cell's
// items x max weight below 2^20 (then the sum stays below 2^20 * 2^24 = 2^44 as well).  Unpacking gives
// (count, sum - 2^23 * count), the signed sum of w * q.
//
// 3-class records (kClsSplit): the label code is 0 / 1 / 2^22, so a cell's signed sum is W1 + 2^22 W2 with
// W1 < 2^22 inside a block; the flush splits it into two int64 columns.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace cdna {

constexpr int kPackShift = 44, kPackCountBits = 64 - kPackShift;
constexpr int kPackQ = 1 << 23;
constexpr int kClsSplit = 22;
constexpr int kRecRowBits = 31, kRecWBits = 8;
constexpr int kRecWShift = kRecRowBits, kRecQShift = kRecWShift + kRecWBits;
static_assert(kRecQShift > 32 && kRecWShift < 32, "the decoders read the weight across the dword boundary");

// qb of a float label
__device__ __forceinline__ int pack_quant(float v1, float qs1) {
  int q1 = (int)rintf(v1 * qs1);
  q1 = q1 > kPackQ ? kPackQ : (q1 < -kPackQ ? -kPackQ : q1);
  return q1 + kPackQ;
}

// what an item of weight w and quantised label qb adds to its cells
__device__ __forceinline__ unsigned long long cell_addend(uint32_t w, unsigned long long qb) {
  return ((unsigned long long)w << kPackShift) + (unsigned long long)w * qb;
}

struct PackedCell {
  unsigned long long cnt;
  long long sum;  // signed: sum of w * q
};

// One cell, or the copies of one cell that a kernel keeps apart in LDS.  The copies are unpacked field by field,
// not added as words: their counts together may exceed the 20-bit field.
__device__ __forceinline__ PackedCell cell_unpack(unsigned long long v0, unsigned long long v1 = 0ull,
                                                  unsigned long long v2 = 0ull) {
  constexpr unsigned long long m = (1ull << kPackShift) - 1ull;
  const unsigned long long cnt = (v0 >> kPackShift) + (v1 >> kPackShift) + (v2 >> kPackShift);
  return PackedCell{cnt, (long long)((v0 & m) + (v1 & m) + (v2 & m)) - (long long)kPackQ * (long long)cnt};
}

__device__ __forceinline__ uint64_t rec_encode(uint64_t row, uint32_t w, float v1, float qs1) {
  return row | ((uint64_t)w << kRecWShift) | ((uint64_t)(uint32_t)pack_quant(v1, qs1) << kRecQShift);
}

__device__ __forceinline__ uint32_t rec_row(uint64_t rc) { return (uint32_t)rc & ((1u << kRecRowBits) - 1u); }

// the weight straddles the two dwords: one v_alignbit_b32
__device__ __forceinline__ uint32_t rec_weight(uint64_t rc) {
  return __builtin_amdgcn_alignbit((uint32_t)(rc >> 32), (uint32_t)rc, kRecWShift) & ((1u << kRecWBits) - 1u);
}

__device__ __forceinline__ uint32_t rec_qb(uint64_t rc) { return (uint32_t)(rc >> 32) >> (kRecQShift - 32); }

// cell_addend with the count's shift done in the high dword: the same value, but the compiler schedules the two
// forms differently, and this is the one the lane kernels' instruction streams were measured with
__device__ __forceinline__ unsigned long long cell_addend_hi(uint32_t w, uint32_t qb) {
  return ((unsigned long long)(w << (kPackShift - 32)) << 32) + (unsigned long long)w * (unsigned long long)qb;
}

// the record's cell addend (record 0: weight 0, adds nothing)
__device__ __forceinline__ unsigned long long rec_addend(uint64_t rc) {
  return cell_addend_hi(rec_weight(rc), rec_qb(rc));
}

}  // namespace cdna
