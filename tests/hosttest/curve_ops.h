// The field / group operations of fq29.h, fr29.h, fq.h, g1_29.h and glv.h as RAW-RECORD functions: int32 words in, int32
// words out, no canonicalisation on either side, so a test sees exactly the limbs the next formula would see.  One list,
// three builds: the host library (hosttest_curve.cpp, g++: the plain-C bodies), and the device test unit
// (tests/devtest/devtest.hip) with the asm bodies and with -DSNARKV_NO_SMAD_ASM.  Test infrastructure only.
//
// Records: Fq29 / Fr29 = 9 words; G1Affine29 = x, y (18); G1Xyzz29 = x, y, zz, zzz (36); Jacobian = x, y, z (27);
// 8 x u32 word arrays as 8 words.
#pragma once
#include "../../snark-verifier_amd/csrc/fr29.h"
#include "../../snark-verifier_amd/csrc/g1_29.h"
#include "../../snark-verifier_amd/csrc/glv.h"
#if !defined(SNARKV_CURVE_PALLAS)
#include "../../snark-verifier_amd/csrc/g2_prepare_w.h"  // the pairing decider's lane pieces (BN254 only): decide_w.h, pairing_coop29.h
#endif

namespace snarkv {
namespace rawops {

SNARKV_HD Fq29 ldq(const int32_t* p) {
  Fq29 r;
#pragma unroll
  for (int i = 0; i < 9; ++i) r.v[i] = p[i];
  return r;
}
SNARKV_HD void stq(const Fq29& a, int32_t* p) {
#pragma unroll
  for (int i = 0; i < 9; ++i) p[i] = a.v[i];
}
SNARKV_HD Fr29 ldr(const int32_t* p) {
  Fr29 r;
#pragma unroll
  for (int i = 0; i < 9; ++i) r.v[i] = p[i];
  return r;
}
SNARKV_HD void str(const Fr29& a, int32_t* p) {
#pragma unroll
  for (int i = 0; i < 9; ++i) p[i] = a.v[i];
}
SNARKV_HD void ldw(const int32_t* p, uint32_t w[8]) {
#pragma unroll
  for (int i = 0; i < 8; ++i) w[i] = (uint32_t)p[i];
}
SNARKV_HD void stw(const uint32_t w[8], int32_t* p) {
#pragma unroll
  for (int i = 0; i < 8; ++i) p[i] = (int32_t)w[i];
}
SNARKV_HD G1Affine29 lda(const int32_t* p) {
  G1Affine29 r;
  r.x = ldq(p);
  r.y = ldq(p + 9);
  return r;
}
SNARKV_HD G1Xyzz29 ldx(const int32_t* p) {
  G1Xyzz29 r;
  r.x = ldq(p);
  r.y = ldq(p + 9);
  r.zz = ldq(p + 18);
  r.zzz = ldq(p + 27);
  return r;
}
SNARKV_HD void stx(const G1Xyzz29& a, int32_t* p) {
  stq(a.x, p);
  stq(a.y, p + 9);
  stq(a.zz, p + 18);
  stq(a.zzz, p + 27);
}

// ---- field ----
SNARKV_HD void op_fq29_mul(const int32_t* in, int32_t* out) { stq(fq29_mul(ldq(in), ldq(in + 9)), out); }
SNARKV_HD void op_fq29_sqr(const int32_t* in, int32_t* out) { stq(fq29_sqr(ldq(in)), out); }
SNARKV_HD void op_fq29_mul2(const int32_t* in, int32_t* out) {
  stq(fq29_mul2(ldq(in), ldq(in + 9), ldq(in + 18), ldq(in + 27)), out);
}
SNARKV_HD void op_fq29_norm(const int32_t* in, int32_t* out) { stq(fq29_norm(ldq(in)), out); }
SNARKV_HD void op_fq29_canon_of_product(const int32_t* in, int32_t* out) { stq(fq29_canon_of_product(ldq(in)), out); }
SNARKV_HD void op_fq29_canon_residue(const int32_t* in, int32_t* out) { stq(fq29_canon_residue(ldq(in)), out); }
SNARKV_HD void op_fq29_is_zero_mod_p(const int32_t* in, int32_t* out) { out[0] = fq29_is_zero_mod_p(ldq(in)) ? 1 : 0; }
SNARKV_HD void op_fq29_from_words(const int32_t* in, int32_t* out) {
  uint32_t w[8];
  ldw(in, w);
  stq(fq29_from_words(w, false), out);
}
SNARKV_HD void op_fq29_from_words_mont(const int32_t* in, int32_t* out) {
  uint32_t w[8];
  ldw(in, w);
  stq(fq29_from_words(w, true), out);
}
SNARKV_HD void op_fq29_to_words(const int32_t* in, int32_t* out) {
  uint32_t w[8];
  fq29_to_words(ldq(in), w, false);
  stw(w, out);
}
SNARKV_HD void op_fq29_to_words_mont(const int32_t* in, int32_t* out) {
  uint32_t w[8];
  fq29_to_words(ldq(in), w, true);
  stw(w, out);
}
SNARKV_HD void op_fq29_pack256(const int32_t* in, int32_t* out) {
  uint32_t w[8];
  fq29_pack256(ldq(in), w);
  stw(w, out);
}
SNARKV_HD void op_fq29_unpack256(const int32_t* in, int32_t* out) {
  uint32_t w[8];
  ldw(in, w);
  stq(fq29_unpack256(w), out);
}
SNARKV_HD void op_fr29_mul(const int32_t* in, int32_t* out) { str(fr29_mul(ldr(in), ldr(in + 9)), out); }
SNARKV_HD void op_fr29_mul2(const int32_t* in, int32_t* out) {
  str(fr29_mul2(ldr(in), ldr(in + 9), ldr(in + 18), ldr(in + 27)), out);
}
SNARKV_HD void op_fr29_from_canonical(const int32_t* in, int32_t* out) {
  uint32_t w[8];
  ldw(in, w);
  str(fr29_from_canonical(w), out);
}
SNARKV_HD void op_fr29_to_canonical(const int32_t* in, int32_t* out) {
  uint32_t w[8];
  fr29_to_canonical(ldr(in), w);
  stw(w, out);
}
SNARKV_HD void op_fr29_pow5(const int32_t* in, int32_t* out) { str(fr29_pow5(ldr(in)), out); }
SNARKV_HD void op_fr29_canon_residue(const int32_t* in, int32_t* out) { str(fr29_canon_residue(ldr(in)), out); }
// the 8 x 32 Montgomery product of fq.h (R = 2^256; device body fq_mul_asm.inc); fq_sqr is fq_mul(a, a)
SNARKV_HD void op_fq_mul(const int32_t* in, int32_t* out) {
  Fq a, b;
  ldw(in, a.v);
  ldw(in + 8, b.v);
  Fq r = fq_mul(a, b);
  stw(r.v, out);
}

// ---- group ----
SNARKV_HD void op_xyzz29_madd_fast(const int32_t* in, int32_t* out) {
  G1Xyzz29 acc = ldx(in);
  xyzz29_madd_fast(acc, lda(in + 36));
  stx(acc, out);
}
SNARKV_HD void op_xyzz29_add_fast(const int32_t* in, int32_t* out) {
  G1Xyzz29 acc = ldx(in);
  xyzz29_add_fast(acc, ldx(in + 36));
  stx(acc, out);
}
SNARKV_HD void op_xyzz29_madd_careful(const int32_t* in, int32_t* out) {
  G1Xyzz29 acc = ldx(in);
  xyzz29_madd_careful(acc, lda(in + 36));
  stx(acc, out);
}
SNARKV_HD void op_xyzz29_add_careful(const int32_t* in, int32_t* out) {
  G1Xyzz29 acc = ldx(in);
  xyzz29_add_careful(acc, ldx(in + 36));
  stx(acc, out);
}
// in: acc, b, bad (1 word); out: acc, bad
SNARKV_HD void op_xyzz29_add_skipid_fast(const int32_t* in, int32_t* out) {
  G1Xyzz29 acc = ldx(in);
  bool bad = in[72] != 0;
  xyzz29_add_skipid_fast(acc, ldx(in + 36), bad);
  stx(acc, out);
  out[36] = bad ? 1 : 0;
}
SNARKV_HD void op_xyzz29_double(const int32_t* in, int32_t* out) { stx(xyzz29_double(ldx(in)), out); }
// in: x, y, z, n (1 word): n Jacobian doublings
SNARKV_HD void op_jac29_double(const int32_t* in, int32_t* out) {
  Fq29 x = ldq(in), y = ldq(in + 9), z = ldq(in + 18);
  for (int k = 0; k < in[27]; ++k) jac29_double(x, y, z);
  stq(x, out);
  stq(y, out + 9);
  stq(z, out + 18);
}
// in: p, n (1 word)
SNARKV_HD void op_xyzz29_double_n(const int32_t* in, int32_t* out) { stx(xyzz29_double_n(ldx(in), in[36]), out); }
SNARKV_HD void op_jac29_to_xyzz(const int32_t* in, int32_t* out) {
  stx(jac29_to_xyzz(ldq(in), ldq(in + 9), ldq(in + 18)), out);
}
SNARKV_HD void op_xyzz29_is_degenerate(const int32_t* in, int32_t* out) { out[0] = xyzz29_is_degenerate(ldx(in)) ? 1 : 0; }
SNARKV_HD void op_xyzz29_to_affine(const int32_t* in, int32_t* out) {
  G1Affine29 r = xyzz29_to_affine(ldx(in));
  stq(r.x, out);
  stq(r.y, out + 9);
}
// in: affine point, 8 scalar words
SNARKV_HD void op_g1_29_scalar_mul_fast(const int32_t* in, int32_t* out) {
  uint32_t k[8];
  ldw(in + 18, k);
  stx(g1_29_scalar_mul<false>(lda(in), k), out);
}
SNARKV_HD void op_g1_29_scalar_mul_careful(const int32_t* in, int32_t* out) {
  uint32_t k[8];
  ldw(in + 18, k);
  stx(g1_29_scalar_mul<true>(lda(in), k), out);
}
SNARKV_HD void op_glv_decompose(const int32_t* in, int32_t* out) {
  uint32_t k[8], o[8];
  ldw(in, k);
  glv_decompose(k, o);
  stw(o, out);
}
// in: a magnitude below 2^127 (4 words); out: its kWinDigits signed 3-bit digits, low to high
SNARKV_HD void op_glv_w3_digits(const int32_t* in, int32_t* out) {
  uint32_t carry = 0;
  for (int i = 0; i < kWinDigits; ++i)
    out[i] = glv_w3_digit((uint32_t)in[0], (uint32_t)in[1], (uint32_t)in[2], (uint32_t)in[3], i, carry);
}


#if !defined(SNARKV_CURVE_PALLAS)
// ---- the lane arithmetic of the pairing decider (fq29.h, pairing_coop29.h, decide_w.h, g2_prepare_w.h) ----
SNARKV_HD void op_fq29_reduce_small(const int32_t* in, int32_t* out) { stq(fq29_reduce_small(ldq(in)), out); }
// in: x, k (1 word)
SNARKV_HD void op_fq29_mul_small_norm(const int32_t* in, int32_t* out) { stq(fq29_mul_small_norm(ldq(in), in[9]), out); }
SNARKV_HD void op_wt_squeeze(const int32_t* in, int32_t* out) { stq(wt_squeeze(ldq(in)), out); }
SNARKV_HD void op_wt_xi_e0(const int32_t* in, int32_t* out) { stq(wt_xi(ldq(in), ldq(in + 9), 0), out); }
SNARKV_HD void op_wt_xi_e1(const int32_t* in, int32_t* out) { stq(wt_xi(ldq(in), ldq(in + 9), 1), out); }
// in: x, m (1 word: 0 / -1)
SNARKV_HD void op_wt_cneg(const int32_t* in, int32_t* out) { stq(wt_cneg(ldq(in), in[9]), out); }
// in: a0, a1, y0, y1
SNARKV_HD void op_coop3_product_e0(const int32_t* in, int32_t* out) {
  stq(coop3_product(0, ldq(in), ldq(in + 9), ldq(in + 18), ldq(in + 27)), out);
}
SNARKV_HD void op_coop3_product_e1(const int32_t* in, int32_t* out) {
  stq(coop3_product(1, ldq(in), ldq(in + 9), ldq(in + 18), ldq(in + 27)), out);
}
// in: lo, hi, hp
SNARKV_HD void op_coop3_finalize_e0(const int32_t* in, int32_t* out) {
  stq(coop3_finalize(0, ldq(in), ldq(in + 9), ldq(in + 18)), out);
}
SNARKV_HD void op_coop3_finalize_e1(const int32_t* in, int32_t* out) {
  stq(coop3_finalize(1, ldq(in), ldq(in + 9), ldq(in + 18)), out);
}
// in: am, bm, ap, bp; out: the fused product, then what k_g2_prepare_w writes into the line table
SNARKV_HD void op_g2w_product_e0(const int32_t* in, int32_t* out) {
  const Fq29 v = g2w_product(ldq(in), ldq(in + 9), ldq(in + 18), ldq(in + 27), 0);
  stq(v, out);
  stq(fq29_canon_of_product(v), out + 9);
}
SNARKV_HD void op_g2w_product_e1(const int32_t* in, int32_t* out) {
  const Fq29 v = g2w_product(ldq(in), ldq(in + 9), ldq(in + 18), ldq(in + 27), 1);
  stq(v, out);
  stq(fq29_canon_of_product(v), out + 9);
}
// in: x, y, g0, g1: the step coop_frob / coop_scale store
SNARKV_HD void op_fq2_scale_norm_e0(const int32_t* in, int32_t* out) {
  stq(fq2_scale_norm(ldq(in), ldq(in + 9), ldq(in + 18), ldq(in + 27), 0), out);
}
SNARKV_HD void op_fq2_scale_norm_e1(const int32_t* in, int32_t* out) {
  stq(fq2_scale_norm(ldq(in), ldq(in + 9), ldq(in + 18), ldq(in + 27), 1), out);
}
// in: d0, d1 (coefficient 0 of the operand register); out: the two values WT_FQ2INV's one lane leaves in the scalar register
SNARKV_HD void op_wt_fq2inv(const int32_t* in, int32_t* out) {
  Fq29P lds[4];
  wt_store(lds, 0, ldq(in));
  wt_store(lds, 1, ldq(in + 9));
  WtOp op{};
  op.a = 0, op.dst = 2, op.kind = WT_FQ2INV;
  wt_fq2inv(lds, op);
  stq(wt_load(lds, 2), out);
  stq(wt_load(lds, 3), out + 9);
}
#endif

}  // namespace rawops
}  // namespace snarkv

// X(name, words in, words out) -- every operation above; tests/fq29_model.py keeps the same table
#define SNARKV_RAW_OPS(X)                \
  X(fq29_mul, 18, 9)                     \
  X(fq29_sqr, 9, 9)                      \
  X(fq29_mul2, 36, 9)                    \
  X(fq29_norm, 9, 9)                     \
  X(fq29_canon_of_product, 9, 9)         \
  X(fq29_canon_residue, 9, 9)            \
  X(fq29_is_zero_mod_p, 9, 1)            \
  X(fq29_from_words, 8, 9)               \
  X(fq29_from_words_mont, 8, 9)          \
  X(fq29_to_words, 9, 8)                 \
  X(fq29_to_words_mont, 9, 8)            \
  X(fq29_pack256, 9, 8)                  \
  X(fq29_unpack256, 8, 9)                \
  X(fr29_mul, 18, 9)                     \
  X(fr29_mul2, 36, 9)                    \
  X(fr29_from_canonical, 8, 9)           \
  X(fr29_to_canonical, 9, 8)             \
  X(fr29_pow5, 9, 9)                     \
  X(fr29_canon_residue, 9, 9)            \
  X(fq_mul, 16, 8)                       \
  X(xyzz29_madd_fast, 54, 36)            \
  X(xyzz29_add_fast, 72, 36)             \
  X(xyzz29_madd_careful, 54, 36)         \
  X(xyzz29_add_careful, 72, 36)          \
  X(xyzz29_add_skipid_fast, 73, 37)      \
  X(xyzz29_double, 36, 36)               \
  X(jac29_double, 28, 27)                \
  X(xyzz29_double_n, 37, 36)             \
  X(jac29_to_xyzz, 27, 36)               \
  X(xyzz29_is_degenerate, 36, 1)         \
  X(xyzz29_to_affine, 36, 18)            \
  X(g1_29_scalar_mul_fast, 26, 36)       \
  X(g1_29_scalar_mul_careful, 26, 36)    \
  X(glv_decompose, 8, 8)                \
  X(glv_w3_digits, 4, 43)

// the pairing decider's pieces (BN254 only); tests/fq29_model.py keeps the same table as DECIDER_OPS
#if !defined(SNARKV_CURVE_PALLAS)
#define SNARKV_RAW_DECIDER_OPS(X) \
  X(fq29_reduce_small, 9, 9)      \
  X(fq29_mul_small_norm, 10, 9)   \
  X(wt_squeeze, 9, 9)             \
  X(wt_xi_e0, 18, 9)              \
  X(wt_xi_e1, 18, 9)              \
  X(wt_cneg, 10, 9)               \
  X(coop3_product_e0, 36, 9)      \
  X(coop3_product_e1, 36, 9)      \
  X(coop3_finalize_e0, 27, 9)     \
  X(coop3_finalize_e1, 27, 9)     \
  X(g2w_product_e0, 36, 18)       \
  X(g2w_product_e1, 36, 18)       \
  X(fq2_scale_norm_e0, 36, 9)     \
  X(fq2_scale_norm_e1, 36, 9)     \
  X(wt_fq2inv, 18, 18)
// records of the two whole rounds (device: k_wt_round / k_coop3_round of tests/devtest/devtest.hip, one workgroup per record;
// host: round_emul.h), in words.  wt_round: A and B as 24 values each, kind, flags -> the 24 values of dst.
// coop3_round: A and B as 12 coefficients each, mode -> 12 coefficients.
constexpr int kWtRoundIn = 48 * 9 + 2, kWtRoundOut = 24 * 9;
constexpr int kCoop3RoundIn = 24 * 9 + 1, kCoop3RoundOut = 12 * 9;
#else
#define SNARKV_RAW_DECIDER_OPS(X)
#endif
