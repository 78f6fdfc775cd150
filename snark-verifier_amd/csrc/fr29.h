// The SCALAR field Fr on the lazy 9x29-bit signed-limb form (Montgomery, R = 2^261): the arithmetic of the Poseidon
// transcript kernel (poseidon.hip), of the transforms and of the polynomial kernels.  The algorithms are those of fq29.h
// (one 64-bit column accumulator, one mad per partial product, limb-wise add/sub with lazy carries) and are stated once
// for both fields in mont29.h; this file binds them to the modulus r (Mod29Fr).
#pragma once
#include "fq29.h"

namespace snarkv {

struct Fr29 {
  int32_t v[9];
};

SNARKV_HD constexpr int32_t fr29_r(int i) { return Mod29Fr::p(i); }
SNARKV_HD Fr29 fr29_zero() { return mont29_zero<Fr29>(); }
SNARKV_HD Fr29 fr29_one() { return mont29_one<Mod29Fr, Fr29>(); }
SNARKV_HD Fr29 fr29_limbs(const int32_t (&l)[9]) { return mont29_limbs<Fr29>(l); }
SNARKV_HD Fr29 fr29_add(const Fr29& a, const Fr29& b) { return mont29_add(a, b); }
SNARKV_HD Fr29 fr29_sub(const Fr29& a, const Fr29& b) { return mont29_sub(a, b); }
// carry-normalise: limbs 0..7 -> [0, 2^29), limb 8 keeps the sign; value unchanged
SNARKV_HD Fr29 fr29_norm(const Fr29& a) { return mont29_norm(a); }
// Montgomery product a*b*2^-261 (mod r); operand classes and column budget as for fq29_mul (fq29.h): one side with
// |limb| <= 2^29 and the other up to 2^30.6, or both up to 2^29.8 -- NOT 2^30 on both sides.  (Plain C products on purpose,
// on every build: the explicit `v_mad_i64_i32` chains of the asm bodies that pay off in the throughput-bound G1 kernels slow
// the latency-bound Poseidon kernel down -- one wavefront per SIMD, where the compiler's two interleaved chains hide
// latency.)  Result carry-normalised, value in a*b/2^261 + [0, r): (-r/2, 3r/2) for |a|, |b| < 8r.
SNARKV_HD Fr29 fr29_mul(const Fr29& a, const Fr29& b) { return mont29_product<Mod29Fr, kMont29Mul, 0>(a, b, a, a); }
// a*b + c*d, one reduction (inputs carry-normalised or the limb-wise negation of that, |limb| < 2^29): the MDS dot products
SNARKV_HD Fr29 fr29_mul2(const Fr29& a, const Fr29& b, const Fr29& c, const Fr29& d) {
  return mont29_product<Mod29Fr, kMont29Mul2, 0>(a, b, c, d);
}
// x^5
SNARKV_HD Fr29 fr29_pow5(const Fr29& x) {
  Fr29 x2 = fr29_mul(x, x);
  Fr29 x4 = fr29_mul(x2, x2);
  return fr29_mul(x4, x);
}
// canonical limbs of a product output (mont29.h): the conditional +r / -r
SNARKV_HD Fr29 fr29_canon_of_product(const Fr29& y) { return mont29_canon_of_product<Mod29Fr>(y); }
// unique representative in [0, r), carry-normalised, still in the Montgomery domain; |x| < 8r
SNARKV_HD Fr29 fr29_canon_residue(const Fr29& x) { return fr29_canon_of_product(fr29_mul(fr29_norm(x), fr29_one())); }
// the 9 x 29-bit limbs of 8 words as they stand (< 2^256 < 8r, carry-normalised, in no domain)
SNARKV_HD Fr29 fr29_limbs_of_words(const uint32_t w[8]) { return mont29_limbs_of_words<Fr29>(w); }
// 8 x u32 canonical integer (< r) -> Montgomery limbs
SNARKV_HD Fr29 fr29_from_canonical(const uint32_t w[8]) {
  constexpr int32_t r2[9] = SNARKV_FR29_R2_LIMBS;
  return fr29_mul(fr29_limbs_of_words(w), fr29_limbs(r2));
}
// the canonical integer words of y f / 2^261 for a carry-normalised y (|y| < 8r) and a plain integer factor f
SNARKV_HD void fr29_words_of_product(const Fr29& y, const Fr29& f, uint32_t w[8]) {
  mont29_words_of_limbs(fr29_canon_of_product(fr29_mul(y, f)), w);
}
// a plain small integer as a factor
SNARKV_HD Fr29 fr29_small(int32_t k) {
  Fr29 r = fr29_zero();
  r.v[0] = k;
  return r;
}
// Montgomery limbs (|a| < 8r) -> canonical integer words: a * R^-1
SNARKV_HD void fr29_to_canonical(const Fr29& a, uint32_t w[8]) { fr29_words_of_product(fr29_norm(a), fr29_small(1), w); }

// halo2curves' in-memory Fr (the four u64 limbs of a * 2^256 mod r) -> the canonical integer a: one Montgomery product by
// 2^5 (x * 32 * 2^-261 = x * 2^-256), then the conditional +r / -r of fr29_to_canonical
SNARKV_HD void fr_words_from_mont256(const uint32_t in[8], uint32_t out[8]) {
  fr29_words_of_product(fr29_limbs_of_words(in), fr29_small(32), out);
}

}  // namespace snarkv
