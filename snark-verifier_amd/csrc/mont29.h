// The lazy 9 x 29-bit signed-limb Montgomery layer (R = 2^261), stated ONCE for both fields that stand on it: Fq29 (fq29.h,
// the contract and the measurements are in its header) and Fr29 (fr29.h).  Everything here is a template over
//   T  the element: a plain struct with `int32_t v[9]` (Fq29 and Fr29 stay two structs: kernel signatures name them), and
//   M  the modulus: Mod29Fq / Mod29Fr below, the generated SNARKV_FQ29_* / SNARKV_FR29_* constants (gen_consts.py).
// What is here: the limb-wise operations, the product scanning loop with its two reductions (mont29_product), the
// canonical tail of a product output (mont29_canon_of_product) and the codec between 8 words and 9 limbs.
#pragma once
#include <stdint.h>
#include "fq.h"

namespace snarkv {

constexpr int32_t kMask29 = (1 << 29) - 1;

// ---- the two moduli: limbs of p, NINV = -p^-1 mod 2^29, the Montgomery one ----
struct Mod29Fq {
  static constexpr uint32_t kNinv = SNARKV_FQ29_NINV;
  SNARKV_HD static constexpr int32_t p(int i) {
    constexpr int32_t l[9] = SNARKV_FQ29_P_LIMBS;
    return l[i];
  }
  // The Montgomery-friendly multiple M = NINV * p = -1 (mod 2^29), ten limbs with limb 0 = 2^29 - 1 and limb 1 stored
  // ALREADY INCREMENTED (SNARKV_FQ29_FM_LIMBS, gen_consts.py)
  SNARKV_HD static constexpr int32_t fm(int i) {
    constexpr int32_t l[10] = SNARKV_FQ29_FM_LIMBS;
    return l[i];
  }
  SNARKV_HD static constexpr int32_t one(int i) {
    constexpr int32_t l[9] = SNARKV_FQ29_ONE_LIMBS;
    return l[i];
  }
};
static_assert(Mod29Fq::fm(0) == kMask29, "limb 0 of the friendly multiple must be 2^29 - 1: the digit is the column's low bits");

struct Mod29Fr {  // no friendly multiple: nothing on Fr asks for one
  static constexpr uint32_t kNinv = SNARKV_FR29_NINV;
  SNARKV_HD static constexpr int32_t p(int i) {
    constexpr int32_t l[9] = SNARKV_FR29_P_LIMBS;
    return l[i];
  }
  SNARKV_HD static constexpr int32_t one(int i) {
    constexpr int32_t l[9] = SNARKV_FR29_ONE_LIMBS;
    return l[i];
  }
};

// ---- limb-wise: never a carry; mont29_norm re-normalises (value unchanged) when the next product needs it ----
template <class T>
SNARKV_HD T mont29_zero() {
  T r;
#pragma unroll
  for (int i = 0; i < 9; ++i) r.v[i] = 0;
  return r;
}

template <class T>
SNARKV_HD T mont29_limbs(const int32_t (&l)[9]) {
  T r;
#pragma unroll
  for (int i = 0; i < 9; ++i) r.v[i] = l[i];
  return r;
}

template <class M, class T>
SNARKV_HD T mont29_one() {
  T r;
#pragma unroll
  for (int i = 0; i < 9; ++i) r.v[i] = M::one(i);
  return r;
}

template <class T>
SNARKV_HD T mont29_add(const T& a, const T& b) {
  T r;
#pragma unroll
  for (int i = 0; i < 9; ++i) r.v[i] = a.v[i] + b.v[i];
  return r;
}

template <class T>
SNARKV_HD T mont29_sub(const T& a, const T& b) {
  T r;
#pragma unroll
  for (int i = 0; i < 9; ++i) r.v[i] = a.v[i] - b.v[i];
  return r;
}

template <class T>
SNARKV_HD T mont29_neg(const T& a) {
  T r;
#pragma unroll
  for (int i = 0; i < 9; ++i) r.v[i] = -a.v[i];
  return r;
}

// carry-normalise: limbs 0..7 -> [0, 2^29), limb 8 keeps the sign; value unchanged
template <class T>
SNARKV_HD T mont29_norm(const T& a) {
  T r;
  int32_t c = 0;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    int32_t t = a.v[i] + c;
    r.v[i] = t & kMask29;
    c = t >> 29;  // arithmetic
  }
  r.v[8] = a.v[8] + c;
  return r;
}

// ---- the product ----
// Which operand products enter a column: a*b; a*b + c*d with ONE reduction; a*a with the cross terms as doubled limbs.
enum Mont29Shape { kMont29Mul, kMont29Mul2, kMont29Sqr };

// The Montgomery product of the given shape (times 2^-261, mod M's p), column-wise (product scanning) with a single 64-bit
// accumulator, in plain C.  FM is the number of reduction steps that use the friendly multiple: 0 is the pinned reduction
// (digit m[k] = (acc * NINV) & mask against p, one multiply per step), fq29.h's kFq29FmSteps its `_fm` one (digit
// q = acc & mask against M for k < FM: no digit multiply, no multiply-add in column k, q * fm(1 .. 9) in columns
// k + 1 .. k + 9, where fm(1) = M_1 + 1 carries the + q of column k).
// The ORDER in which partial products enter a column is part of the contract: operand products first (for mul2 all a*b,
// then all c*d), then the reduction products by ascending digit index.  tests/fq29_model.py checks the int64 column budget
// against it, and the generated asm bodies (gen_fq29_mul_asm.py) implement the same schedule, limb for limb.
// Operands a shape does not have are passed as any element and never read.
template <class M, Mont29Shape SHAPE, int FM, class T>
SNARKV_HD T mont29_product(const T& a, const T& b, const T& c, const T& d) {
  int32_t m[9], a2[9];
  T r;
  if constexpr (SHAPE == kMont29Sqr) {
#pragma unroll
    for (int i = 0; i < 9; ++i) a2[i] = a.v[i] * 2;
  }
  int64_t acc = 0;
  // the partial products of column k: operand limbs lo .. hi, then the digits below k whose multiple reaches the column
  // (always_inline like everything else here: the compiler sees the loops as if they stood in the caller)
  auto column = [&](int k) __attribute__((always_inline)) {
    const int lo = k < 9 ? 0 : k - 8, hi = k < 9 ? k : 8;
    if constexpr (SHAPE == kMont29Sqr) {
#pragma unroll
      for (int i = lo; 2 * i < k; ++i) acc += (int64_t)a2[i] * a.v[k - i];
      if ((k & 1) == 0) acc += (int64_t)a.v[k / 2] * a.v[k / 2];
    } else {
#pragma unroll
      for (int i = lo; i <= hi; ++i) acc += (int64_t)a.v[i] * b.v[k - i];
      if constexpr (SHAPE == kMont29Mul2) {
#pragma unroll
        for (int i = lo; i <= hi; ++i) acc += (int64_t)c.v[i] * d.v[k - i];
      }
    }
    if constexpr (FM > 0) {  // digits against M: ten limbs, so one column further than p
#pragma unroll
      for (int i = (k < 10 ? 0 : k - 9); i < (k < FM ? k : FM); ++i) acc += (int64_t)m[i] * M::fm(k - i);
    }
#pragma unroll
    for (int i = (lo > FM ? lo : FM); i < (k < 9 ? k : 9); ++i) acc += (int64_t)m[i] * M::p(k - i);
  };
#pragma unroll
  for (int k = 0; k < 9; ++k) {
    column(k);
    if (k < FM) {
      m[k] = (int32_t)acc & kMask29;  // acc + m[k] (2^29 - 1) = (acc >> 29) 2^29 + m[k] 2^29: the + m[k] is in fm(1)
    } else {
      m[k] = (int32_t)(((uint32_t)acc * M::kNinv) & (uint32_t)kMask29);
      acc += (int64_t)m[k] * M::p(0);
    }
    acc >>= 29;  // low 29 bits are zero
  }
#pragma unroll
  for (int k = 9; k < 17; ++k) {
    column(k);
    r.v[k - 9] = (int32_t)acc & kMask29;
    acc >>= 29;
  }
  r.v[8] = (int32_t)acc;
  return r;
}

// ---- leaving the lazy form ----
// Canonical limbs (the unique representative in [0, p), carry-normalised) of a value y in (-p, 2p) whose limbs 0..7 are
// already in [0, 2^29) -- in particular any OUTPUT of a product of operands within (-8p, 8p) (value in (-p/2, 3p/2)): one
// conditional +p, one conditional -p, no product
template <class M, class T>
SNARKV_HD T mont29_canon_of_product(const T& y) {
  T t;
  int32_t neg = y.v[8] >> 31;  // negative: all ones
#pragma unroll
  for (int i = 0; i < 9; ++i) t.v[i] = y.v[i] + (M::p(i) & neg);
  t = mont29_norm(t);
  // subtract p if t >= p
  T d;
  int32_t c = 0;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    int32_t s = t.v[i] - M::p(i) + c;
    d.v[i] = s & kMask29;
    c = s >> 29;
  }
  d.v[8] = t.v[8] - M::p(8) + c;
  int32_t keep = d.v[8] >> 31;  // negative -> t < p -> keep t
#pragma unroll
  for (int i = 0; i < 9; ++i) t.v[i] = (t.v[i] & keep) | (d.v[i] & ~keep);
  return t;
}

// the 9 x 29-bit limbs of 8 words as they stand: the integer itself (< 2^256), carry-normalised, in no domain
template <class T>
SNARKV_HD T mont29_limbs_of_words(const uint32_t w[8]) {
  T a;
#pragma unroll
  for (int i = 0; i < 9; ++i) {
    int bit = 29 * i;
    int word = bit >> 5, sh = bit & 31;
    uint64_t v = w[word];
    if (word + 1 < 8) v |= (uint64_t)w[word + 1] << 32;
    a.v[i] = (int32_t)((uint32_t)(v >> sh) & (uint32_t)kMask29);
  }
  return a;
}

// the 8 words of canonical limbs (limbs 0..7 in [0, 2^29), limb 8 below 2^24)
template <class T>
SNARKV_HD void mont29_words_of_limbs(const T& t, uint32_t w[8]) {
#pragma unroll
  for (int j = 0; j < 8; ++j) w[j] = 0;
#pragma unroll
  for (int i = 0; i < 9; ++i) {
    int bit = 29 * i;
    int word = bit >> 5, sh = bit & 31;
    uint64_t v = (uint64_t)(uint32_t)t.v[i] << sh;
    w[word] |= (uint32_t)v;
    if (word + 1 < 8) w[word + 1] |= (uint32_t)(v >> 32);
  }
}

}  // namespace snarkv
