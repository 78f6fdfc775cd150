// Digit form of the shared-key MSM (msm_shared.hip): plain signed 8-bit digits of the FULL scalar,
//     s = sum_{w < 32} d_w 2^(8 w),   d_w in [-127, 128],
// against the key's window table T[w][j] = 2^(8 w) G[j].  One digit per byte, low to high: a raw byte plus the carry from
// below that exceeds 128 becomes raw - 256 with a carry up (the convention of glv.h's recoder, a byte wide).  A canonical
// scalar of either curve is below 2^255, so its top byte is at most 0x7f, the top digit at most 0x80 and no carry leaves
// window 31; any other 256-bit value is first brought below r (at most 2^256 / r < 6 subtractions), which multiplies a
// point of order r by the same thing.
// Same source for the device kernels and for the host test library (tests/hosttest/hosttest_shared.cpp).
#pragma once
#include "curve_consts.h"
#include "fq.h"

namespace snarkv {

constexpr int kSharedC = 8;                              // bits of a digit
constexpr int kSharedW = 32;                             // windows = rows of the table per base
constexpr int kSharedBuckets = 1 << (kSharedC - 1);      // magnitudes 1 .. 128

// s -= r while s >= r (s: any 256-bit value, 8 little-endian words)
SNARKV_HD void shared_reduce_mod_r(uint32_t s[8]) {
  constexpr uint32_t R[8] = SNARKV_FR_R_LIMBS;
  uint32_t r[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) r[i] = R[i];
#pragma unroll 1
  for (int round = 0; round < 6; ++round) {
    uint32_t d[8];
    uint32_t borrow = 0;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const uint64_t v = (uint64_t)s[i] - r[i] - borrow;
      d[i] = (uint32_t)v;
      borrow = (uint32_t)(v >> 32) & 1u;
    }
    if (borrow) break;  // s < r
#pragma unroll
    for (int i = 0; i < 8; ++i) s[i] = d[i];
  }
}

// emit(w, d) for every window, low to high (d may be 0); returns the carry out of window 31 (0 for s < 2^255)
template <class F>
SNARKV_HD uint32_t shared_recode_each(const uint32_t s[8], F emit) {
  uint32_t carry = 0;
#pragma unroll
  for (int w = 0; w < kSharedW; ++w) {
    uint32_t raw = ((s[w >> 2] >> (8 * (w & 3))) & 0xFFu) + carry;
    carry = raw > 128u ? 1u : 0u;
    emit(w, (int)raw - (carry ? 256 : 0));
  }
  return carry;
}

}  // namespace snarkv
