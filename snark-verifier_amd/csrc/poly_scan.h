// Division of a polynomial by a linear factor as a blocked scan: the block decomposition and the arithmetic of one lane.
//   c_n = 0,  c_i = p_i + a c_{i+1}   =>   p = (X - a) quot + rem  with  quot[i-1] = c_i,  rem = c_0 = p(a)
// The recurrence is sequential; with blocks of B coefficients it splits into three phases:
//   1  in block b (indices [bB, min((b+1)B, n))):  s_i = sum_{j >= i, j in the block} p_j a^(j-i),  total T_b = s_{bB}
//   2  the totals are a polynomial in a^B:          C_b = T_b + a^B C_{b+1}  (the same recurrence, one level up)
//      and C_b = c_{bB}, so the carry into block b is C_{b+1}; the last block has none
//   3  c_i = s_i + a^((b+1)B - i) C_{b+1} = s_i + a^(B - lane) carry_b
// Phase 1 is itself a scan over the B lanes of a block: log2(B) steps at distances 1, 2, 4, ..., in step d every lane
// adds a^d times the value of the lane d to its right (none beyond the block's end).
//
// Same source for the kernels of poly.hip (B = 256, one lane per thread) and for the host (tests/hosttest/hosttest_poly.cpp,
// any B), as ipa_fold.h.
#pragma once
#include <stdint.h>
#include "fr29.h"

namespace snarkv {

template <uint32_t B>
struct PolyScan {
  static_assert(B >= 2, "a block of one coefficient does not shorten the recurrence");
  SNARKV_HD static uint32_t blocks(uint32_t n) { return (n + B - 1) / B; }
  SNARKV_HD static uint32_t block_of(uint32_t i) { return i / B; }
  SNARKV_HD static uint32_t lane_of(uint32_t i) { return i % B; }
  SNARKV_HD static uint32_t block_len(uint32_t b, uint32_t n) { return n - b * B < B ? n - b * B : B; }
  // the carry into block b is the scanned total of block b + 1
  SNARKV_HD static bool has_carry(uint32_t b, uint32_t n) { return b + 1 < blocks(n); }
  SNARKV_HD static uint32_t carry_index(uint32_t b) { return b + 1; }
  // ... and reaches the lane multiplied by a^carry_exp(lane); the level above runs with the root a^B
  SNARKV_HD static uint32_t carry_exp(uint32_t lane) { return B - lane; }
  // in step `step` lane t takes the lane t + distance(step), if the block has it
  SNARKV_HD static uint32_t steps() {
    uint32_t s = 0;
    while ((1u << s) < B) ++s;
    return s;
  }
  SNARKV_HD static uint32_t distance(uint32_t step) { return 1u << step; }
  SNARKV_HD static bool has_partner(uint32_t lane, uint32_t step, uint32_t len) { return lane + distance(step) < len; }
};

// One step of phase 1: s + a^d other.  Values: a product is within (-r/2, 3r/2) (fr29_mul), so is a coefficient fresh from
// fr29_from_canonical; four steps add four products, (-5r/2, 15r/2) at most, inside the |x| < 8r that fr29_mul and
// fr29_to_canonical take; every fourth step ends with a product by one, which brings the sum back to (-r/8, 9r/8)
// (fr_add_red of ipa_prover.hpp).  Limbs: the sum is carry-normalised, as the next step's product wants its operand.
SNARKV_HD Fr29 poly_scan_step(const Fr29& s, const Fr29& other, const Fr29& a_pow_d, uint32_t step) {
  Fr29 t = fr29_norm(fr29_add(s, fr29_mul(a_pow_d, other)));
  if ((step & 3u) == 3u) t = fr29_mul(t, fr29_one());
  return t;
}
// (a lane without a partner keeps its value: it has none in any later step either, so it stays below 8r)

// a^e from sq[j] = a^(2^j); e < 2^bits
SNARKV_HD Fr29 poly_scan_pow(const Fr29* sq, uint32_t e, uint32_t bits) {
  Fr29 acc = fr29_one();
  for (uint32_t j = 0; j < bits; ++j)
    if ((e >> j) & 1u) acc = fr29_mul(acc, sq[j]);
  return acc;
}

// phase 3: s + a^(B - lane) carry, with s and the carry fresh from fr29_from_canonical: (-r, 3r)
SNARKV_HD Fr29 poly_scan_apply(const Fr29& s, const Fr29& a_pow, const Fr29& carry) {
  return fr29_norm(fr29_add(s, fr29_mul(a_pow, carry)));
}

}  // namespace snarkv
