// The arithmetic of one tile of a transform pass (ntt_plan.h): what a lane does to an element on the way in, in a butterfly
// and on the way out, and the entries of the tables of powers.  Written over a buffer and a lane's indices, so that the
// kernel of ntt.hip (one butterfly per thread, a barrier between levels) and a host loop over the lanes
// (tests/hosttest/hosttest_ntt.cpp) run the same source.
//
// Values.  fr29_mul returns a b / 2^261 + [0, r) (fr29.h).  Every product here has one operand that is canonical, in
// [0, r), or itself such a product: a table entry, or the product of two.  With the other operand below 8r the first term is
// below 8r * 1.07r / 2^261 < 0.07r (r < 2^254.01), so such a product lies in (-0.07r, 1.07r).
//   in         raw words (< 2^256 < 8r) times a factor: (-0.07r, 1.07r)
//   butterfly  t = v w, then u + t and u - t: an element that is the top operand on every level grows by 1.07r per level,
//              and the bottom one follows it (it is made from the top one).  Entering level l without a reduction the bound
//              is 1.07 (l + 1) r.  After every sixth level (l % 6 == 5) both results are multiplied by one, which brings them
//              back to (-0.07r, 1.07r): the largest multiplier input is that reduction's, 7 * 1.07r = 7.49r < kNttBound r =
//              7.5r < 8r.  One level later it would be 8.56r.
//   out        at most five levels since the load or a reduction: below 6.42r, times a plain factor in (-0.07r, 1.07r); the
//              product is in that range too, and the conditional +r / -r of fr29_to_canonical makes it canonical.
// Limbs.  Sums and differences are carry-normalised at once: every multiplier operand has limbs 0..7 in [0, 2^29).
#pragma once
#include <stdint.h>
#include "fr29.h"

#ifndef SNARKV_NTT_PROBE  // the host model records every multiplier input here
#define SNARKV_NTT_PROBE(x)
#endif

namespace snarkv {

constexpr uint32_t kNttReduceEvery = 6;
constexpr double kNttBound = 7.5;  // |multiplier input| / r stays below this
SNARKV_HD bool ntt_reduce_after(uint32_t level) { return level % kNttReduceEvery == kNttReduceEvery - 1; }

// the constant factors: 2^522 mod r (words in -> Montgomery domain) and the integer 1 (Montgomery domain -> words out)
SNARKV_HD Fr29 ntt_factor_in() {
  constexpr int32_t r2[9] = SNARKV_FR29_R2_LIMBS;
  return fr29_limbs(r2);
}
SNARKV_HD Fr29 ntt_factor_out() { return fr29_small(1); }
// the 9 x 29-bit limbs of 8 words as they stand
SNARKV_HD Fr29 ntt_raw_limbs(const uint32_t w[8]) { return fr29_limbs_of_words(w); }

// words in: x f, with f = 2^522 f' the wanted factor f' twice in the Montgomery domain (ntt_factor_in() for f' = 1)
SNARKV_HD Fr29 ntt_load(const uint32_t w[8], const Fr29& f) { return fr29_mul(ntt_raw_limbs(w), f); }

// words out: the canonical integer of a f / 2^261, f a plain integer factor (ntt_factor_out() for 1); fr29_to_canonical with
// the factor in place of its one
SNARKV_HD void ntt_store(const Fr29& a, const Fr29& f, uint32_t w[8]) {
  const Fr29 an = fr29_norm(a);
  SNARKV_NTT_PROBE(an);
  fr29_words_of_product(an, f, w);
}

// one butterfly of level `level`, in place: the pairs of a level are disjoint
SNARKV_HD void ntt_butterfly(Fr29* buf, uint32_t top, uint32_t distance, const Fr29& w, uint32_t level) {
  const Fr29 u = buf[top], v = buf[top + distance];
  SNARKV_NTT_PROBE(v);
  const Fr29 t = fr29_mul(v, w);
  Fr29 x = fr29_norm(fr29_add(u, t)), y = fr29_norm(fr29_sub(u, t));
  if (ntt_reduce_after(level)) {
    SNARKV_NTT_PROBE(x);
    SNARKV_NTT_PROBE(y);
    x = fr29_mul(x, fr29_one());
    y = fr29_mul(y, fr29_one());
  }
  buf[top] = x;
  buf[top + distance] = y;
}

// the factor of exponent e from a two-level table: lo[e mod 2^h] hi[e >> h], one product.  hi is in the Montgomery domain;
// lo carries the form of the result (plain, or twice in the Montgomery domain for ntt_load) and any constant factor.
SNARKV_HD Fr29 ntt_factor(const Fr29* lo, const Fr29* hi, uint32_t e, uint32_t h) {
  return fr29_mul(lo[e & ((1u << h) - 1u)], hi[e >> h]);
}

// entry j of a table of powers: (base^(2^pre))^j scale / 2^261 as the canonical residue; base in the Montgomery domain.
// scale = fr29_one() keeps the power there, the integer 1 makes it plain, 2^522 mod r puts it there twice; a plain constant
// rides along.
SNARKV_HD Fr29 ntt_table_entry(const Fr29& base, uint32_t pre, uint32_t j, const Fr29& scale) {
  Fr29 x = base;
  for (uint32_t i = 0; i < pre; ++i) x = fr29_mul(x, x);
  Fr29 acc = fr29_one();
  for (; j; j >>= 1) {
    if (j & 1u) acc = fr29_mul(acc, x);
    x = fr29_mul(x, x);
  }
  return fr29_canon_residue(fr29_mul(acc, scale));
}

// the 2^S-th root of unity F::ROOT_OF_UNITY (or its inverse) squared `times` times: the generator of the domain of 2^(S - times)
SNARKV_HD Fr29 ntt_root_squared(bool inverse, uint32_t times) {
  constexpr int32_t fwd[9] = SNARKV_FR29_ROOT_OF_UNITY_LIMBS, inv[9] = SNARKV_FR29_ROOT_OF_UNITY_INV_LIMBS;
  Fr29 w = inverse ? fr29_limbs(inv) : fr29_limbs(fwd);
  for (uint32_t i = 0; i < times; ++i) w = fr29_mul(w, w);
  return w;
}

// 2^-k as a plain integer's limbs: ((r + 1) / 2)^k
SNARKV_HD Fr29 ntt_n_inverse(uint32_t k) {
  constexpr uint32_t rw[8] = SNARKV_FR_R_LIMBS;
  uint32_t half[8];  // (r >> 1) + 1, r odd
  for (int i = 0; i < 8; ++i) half[i] = (rw[i] >> 1) | (i + 1 < 8 ? rw[i + 1] << 31 : 0u);
  for (int i = 0; i < 8 && ++half[i] == 0; ++i) {
  }
  const Fr29 h = fr29_from_canonical(half);
  Fr29 acc = fr29_one();
  for (uint32_t i = 0; i < k; ++i) acc = fr29_mul(acc, h);
  uint32_t w[8];
  fr29_to_canonical(acc, w);
  return ntt_raw_limbs(w);
}

}  // namespace snarkv
