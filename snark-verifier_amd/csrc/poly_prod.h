// Products along a column of scalars: the multiplicative prefix scan (grand product) and the batch inversion, as blocked
// scans over levels -- the block decomposition and the arithmetic of one lane.
//
// A block is T lanes of E consecutive elements each, B = T E elements.  With x the elements of one block:
//   lane        the lane's own exclusive prefix products p_j = x_0 .. x_{j-1} (p_0 = 1) and its total, E - 1 products each
//   workgroup   the inclusive scan of the T lane totals: log2(T) steps at distances 1, 2, 4, ..., in step d every lane
//               multiplies in the value of the lane d to its left (prefix) or right (suffix); none beyond the block
//   levels      the block totals are a sequence like any other, one level up, until one block remains
//
// grand product   out_i = start x_0 .. x_{i-1}: bottom up only totals are written; top down every block recomputes its
//                 prefixes from the input and multiplies them by its carry, the scanned total sequence of the level above
//                 (`start` at the top).  A block reads its elements before it writes them: out may be the input.
// batch inverse   with y = x, zeros replaced by one: bottom up the totals of y (never zero); the top block inverts its total
//                 once (prod_inv, the only inversion of a call); top down block b is handed w_b = 1 / T_b and gives
//                 1 / y_i = P_{i-1} S_{i+1} w_b from its prefix and suffix products, recomputed from the input.  On the
//                 levels above, 1 / y_i is exactly the w of block i below.  A zero is stored as zero.
//
// Values: everything here is a bare product.  A value fresh from fr29_from_canonical or fr29_mul is carry-normalised and
// within (-r/2, 3r/2), inside the |x| < 8r that fr29_mul takes on both sides; a product of two such is again.  The one sum,
// prod_affine_term, states its bound where it stands.
//
// Same source for the kernels of poly_prod.hip (T = 256, E = 4 on the data, E = 1 on the totals) and for the host
// (tests/hosttest/hosttest_poly_prod.cpp, blocks of 2, 3 and 4), as poly_scan.h.
#pragma once
#include <stdint.h>
#include "fr29.h"

namespace snarkv {

template <uint32_t T, uint32_t E>
struct ProdBlock {
  static_assert(T >= 2 && E >= 1, "a block of one lane does not shorten the product");
  static constexpr uint32_t B = T * E;
  SNARKV_HD static uint32_t blocks(uint32_t n) { return (n + B - 1) / B; }
  SNARKV_HD static uint32_t block_len(uint32_t b, uint32_t n) { return n - b * B < B ? n - b * B : B; }
  // element j of lane t of block b, and whether the sequence has it
  SNARKV_HD static uint32_t index(uint32_t b, uint32_t t, uint32_t j) { return b * B + t * E + j; }
  SNARKV_HD static bool has(uint32_t t, uint32_t j, uint32_t len) { return t * E + j < len; }
  SNARKV_HD static uint32_t steps() {
    uint32_t s = 0;
    while ((1u << s) < T) ++s;
    return s;
  }
  SNARKV_HD static uint32_t distance(uint32_t step) { return 1u << step; }
  // the partner of lane t in a step of the prefix scan (to its left) and of the suffix scan (to its right)
  SNARKV_HD static bool has_left(uint32_t t, uint32_t step) { return t >= distance(step); }
  SNARKV_HD static bool has_right(uint32_t t, uint32_t step) { return t + distance(step) < T; }
};

// zero iff the residue mod r is: the lazy forms of zero (0, r, ... as they come out of fr29_from_canonical for the words of
// 0, r, 2r, ...) all have the canonical residue 0
SNARKV_HD bool prod_is_zero(const Fr29& x) {
  const Fr29 c = fr29_canon_residue(x);
  int32_t any = 0;
#pragma unroll
  for (int i = 0; i < 9; ++i) any |= c.v[i];
  return any == 0;
}

// the E elements of a lane -> their exclusive prefix products p and the lane's total
template <uint32_t E>
SNARKV_HD void prod_lane_prefix(const Fr29* x, Fr29* p, Fr29& total) {
  p[0] = fr29_one();
  Fr29 acc = x[0];
#pragma unroll
  for (uint32_t j = 1; j < E; ++j) {
    p[j] = acc;
    acc = fr29_mul(acc, x[j]);
  }
  total = acc;
}
// ... and, for the inversion, m_j = the product of the lane's other elements: the exclusive prefix times the exclusive suffix
// q_j = x_{j+1} .. x_{E-1}.  Only m and the total stay live across the workgroup scans.
template <uint32_t E>
SNARKV_HD void prod_lane_others(const Fr29* x, Fr29* m, Fr29& total) {
  Fr29 p[E], q[E];
  prod_lane_prefix<E>(x, p, total);
  q[E - 1] = fr29_one();
#pragma unroll
  for (uint32_t j = E - 1; j > 0; --j) q[j - 1] = j == E - 1 ? x[j] : fr29_mul(q[j], x[j]);
#pragma unroll
  for (uint32_t j = 0; j < E; ++j) m[j] = j == 0 ? q[0] : (j + 1 == E ? p[j] : fr29_mul(p[j], q[j]));
}

// one step of the workgroup scan
SNARKV_HD Fr29 prod_scan_step(const Fr29& s, const Fr29& other) { return fr29_mul(s, other); }
struct ProdStep {
  SNARKV_HD Fr29 operator()(const Fr29& s, const Fr29& other) const { return prod_scan_step(s, other); }
};

#if defined(__HIPCC__)
// The inclusive scan of one value per lane over the workgroup, to the left (prefix) or to the right (suffix), for the kernels
// of poly_prod.hip (Fr29, ProdStep) and of lookup.hip (its counts and their sum): two buffers, one barrier per step, as
// k_poly_scan.  The barrier in front lets the caller have read `sh` just before.  STEP: a type whose call combines two values.
template <typename STEP, bool RIGHT, uint32_t T, typename V>
__device__ __forceinline__ V wg_scan(V (&sh)[2][T], V s, uint32_t lane) {
  typedef ProdBlock<T, 1> S;
  __syncthreads();
#pragma unroll 1
  for (uint32_t step = 0; step < S::steps(); ++step) {
    sh[step & 1u][lane] = s;
    __syncthreads();
    if (RIGHT ? S::has_right(lane, step) : S::has_left(lane, step))
      s = STEP()(s, sh[step & 1u][RIGHT ? lane + S::distance(step) : lane - S::distance(step)]);
  }
  return s;
}
// the scanned values into sh[0]: the neighbour's is the exclusive scan of a lane, the last (first) lane's the block's total
template <uint32_t T, typename V>
__device__ __forceinline__ void wg_publish(V (&sh)[2][T], const V& s, uint32_t lane) {
  __syncthreads();
  sh[0][lane] = s;
  __syncthreads();
}
#endif

// grand product, top down: `before` = the carry of the block times the totals of the lanes to the left
template <uint32_t E>
SNARKV_HD void prod_lane_outputs(const Fr29& before, const Fr29* p, Fr29* out) {
  out[0] = before;
#pragma unroll
  for (uint32_t j = 1; j < E; ++j) out[j] = fr29_mul(before, p[j]);
}

// batch inverse, top down: `around` = w_b times the totals of the lanes to the left times those of the lanes to the right;
// m from prod_lane_others of y
template <uint32_t E>
SNARKV_HD void prod_lane_inverses(const Fr29& around, const Fr29* m, const bool* zero, Fr29* out) {
#pragma unroll
  for (uint32_t j = 0; j < E; ++j) out[j] = zero[j] ? fr29_zero() : (E == 1 ? around : fr29_mul(around, m[j]));
}

// x^(r-2): 254 squarings; x != 0
SNARKV_HD Fr29 prod_inv(const Fr29& x) {
  constexpr uint32_t rw[8] = SNARKV_FR_R_LIMBS;
  uint32_t e[8];
  uint32_t borrow = 2;
  for (int i = 0; i < 8; ++i) {
    const uint32_t v = rw[i];
    e[i] = v - borrow;
    borrow = v < borrow ? 1u : 0u;
  }
  Fr29 acc = fr29_one();
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll 1
#endif
  for (int b = 255; b >= 0; --b) {
    acc = fr29_mul(acc, acc);
    if ((e[b >> 5] >> (b & 31)) & 1u) acc = fr29_mul(acc, x);
  }
  return acc;
}

// the 9 x 29-bit limbs of 8 words as they stand, not in the Montgomery domain: the integer itself, < 2^256 < 8r, normalised
SNARKV_HD Fr29 prod_raw(const uint32_t w[8]) { return fr29_limbs_of_words(w); }
// s -> s R^2 in the Montgomery domain: its product with raw limbs is the Montgomery form of the product
SNARKV_HD Fr29 prod_scalar_for_raw(const Fr29& s) {
  constexpr int32_t r2[9] = SNARKV_FR29_R2_LIMBS;
  Fr29 m;
#pragma unroll
  for (int i = 0; i < 9; ++i) m.v[i] = r2[i];
  return fr29_mul(s, m);
}

// One factor of the affine product: a + beta b + gamma, with b as raw limbs and beta from prod_scalar_for_raw.  Values: a and
// gamma are fresh from fr29_from_canonical, the middle term from fr29_mul, each within (-r/2, 3r/2): the sum is within
// (-3r/2, 9r/2), inside the |x| < 8r of fr29_mul.  Limbs: three normalised values added limb by limb reach 3 * 2^29, more
// than the 2^29.8 that both sides of a product may have, so the sum is carry-normalised before it is a factor.
SNARKV_HD Fr29 prod_affine_term(const Fr29& a, const Fr29& b_raw, const Fr29& beta_r2, const Fr29& gamma) {
  return fr29_norm(fr29_add(fr29_add(a, fr29_mul(b_raw, beta_r2)), gamma));
}
// ... without the middle term: (-r, 3r), two normalised values
SNARKV_HD Fr29 prod_affine_term(const Fr29& a, const Fr29& gamma) { return fr29_norm(fr29_add(a, gamma)); }

}  // namespace snarkv
