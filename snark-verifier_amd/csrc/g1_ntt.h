// The arithmetic of one pass of the transform over group elements (include/snarkv_g1_ntt.h): which elements a butterfly reads
// and writes, what a lane does on the way to its half of w^e * b, and how two such halves and `a` become one output point.
// Written over a lane's own values and a scratch policy, so that the kernels of g1_ntt.hip (k_g1_ntt_mul: two lanes per
// butterfly, a partial each in global memory; k_g1_ntt_combine: one lane per output) and a host loop over the lanes
// (tests/hosttest/hosttest_g1_ntt.cpp) run the same source.
//
// Passes.  Stockham's radix-2 form, natural order in and out, never in place: pass s < k reads in[j] and in[j + n/2], j < n/2,
// and with kk = j mod 2^s writes  out[2 (j - kk) + kk] = a + t,  out[2 (j - kk) + kk + 2^s] = a - t,  t = w^(kk 2^(k-1-s)) * b.
// Pass 0 has kk = 0 everywhere: it multiplies nothing.  The inverse transform runs the same passes over w^-1 and then multiplies
// every element by n^-1 once (a pass of its own: n^-1 cannot ride on the twiddles, because in[0] is never a `b`).
//
// One scalar multiplication per butterfly, as k_term_scalar_mul of msm_naive.hip does a term: the GLV split  e = e1 + e2 lambda
// (glv.h), one lane per half, a signed 3-bit fixed window over |e_h| on b resp. phi(b) with the half's sign folded into y, the
// fast adders inside the window and the degenerate check + the bit-serial careful run as the net.  The text of the window is
// this file's own and not msm_naive.hip's, whose functions read threadIdx and a launch-sized table: moving them here would have
// changed the code of the MSM kernels.
//
// Every addition outside the window is a careful one: a butterfly of crafted inputs meets a = +-t and t = identity (all points
// equal: every difference is the identity and every sum a doubling).  Points cross passes as canonical affine words, so every
// pass multiplies an affine point and every lane pays one field inversion next to ~1 800 products.
#pragma once
#include <stdint.h>
#include "fr29.h"
#include "g1_29.h"
#include "glv.h"
#include "ntt_tile.h"

namespace snarkv {

constexpr uint32_t kG1NttMaxK = 22;

struct G1NttBfly {
  uint32_t a, b;    // elements read
  uint32_t lo, hi;  // elements written: a + t, a - t
  uint32_t e;       // t = w^e * b, e < n/2
};

SNARKV_HD G1NttBfly g1_ntt_bfly(uint32_t k, uint32_t s, uint32_t j) {
  const uint32_t kk = j & ((1u << s) - 1u);
  G1NttBfly r;
  r.a = j;
  r.b = j + (1u << (k - 1));
  r.lo = ((j - kk) << 1) + kk;
  r.hi = r.lo + (1u << s);
  r.e = kk << (k - 1 - s);
  return r;
}

// entry j of the table of twiddles: (w^j) as the canonical integer's words, w in the Montgomery domain
SNARKV_HD void g1_ntt_twiddle(const Fr29& w, uint32_t j, uint32_t out[8]) { fr29_to_canonical(ntt_table_entry(w, 0, j, fr29_one()), out); }

// 2^-k as the canonical integer's words
SNARKV_HD void g1_ntt_n_inverse(uint32_t k, uint32_t out[8]) {
  const Fr29 l = ntt_n_inverse(k);  // the limbs of those words
  Fq29 q;
  for (int i = 0; i < 9; ++i) q.v[i] = l.v[i];
  fq29_pack256(q, out);
}

SNARKV_HD Fq29 g1_ntt_beta() {
  constexpr int32_t bl[9] = SNARKV_GLV_BETA29_LIMBS;
  Fq29 beta;
  for (int j = 0; j < 9; ++j) beta.v[j] = bl[j];
  return beta;
}

// |k| * Q, Q affine and not the identity, 0 < |k| < 2^127 given as four words by value (glv.h: why not a pointer), through
// the lane's scratch SCR:  tab_put(e, P) / tab_get(e)  hold 2Q, 3Q, 4Q (e = 0, 1, 2),  dig_put(i, d) / dig_get(i)  the
// digits.  half_scalar_mul_w3 of msm_naive.hip has the reasoning: a fast addition can only meet P = +-Q while the accumulator
// is still the identity, which `started` covers; the caller checks the result for a degenerate ZZ.
template <class SCR>
SNARKV_HD G1Xyzz29 g1_ntt_window_mul(const G1Affine29& q, uint32_t k0, uint32_t k1, uint32_t k2, uint32_t k3, SCR& scr) {
  G1Xyzz29 t2 = xyzz29_double_affine(q), t3 = t2;
  xyzz29_madd_fast(t3, q);
  scr.tab_put(0, t2);
  scr.tab_put(1, t3);
  scr.tab_put(2, xyzz29_double(t2));
  uint32_t carry = 0;
  for (int i = 0; i < kWinDigits; ++i) scr.dig_put(i, glv_w3_digit(k0, k1, k2, k3, i, carry));
  G1Xyzz29 acc = xyzz29_identity();
  bool started = false;
#if defined(__HIPCC__)
#pragma unroll 1
#endif
  for (int i = kWinDigits - 1; i >= 0; --i) {
    acc = xyzz29_double(xyzz29_double(xyzz29_double(acc)));  // 8 acc (all-zero stays all-zero)
    const int d = scr.dig_get(i);
    const int a = d < 0 ? -d : d;
    if (a != 0) {
      G1Xyzz29 sel = a == 1 ? xyzz29_from_affine(q) : scr.tab_get(a - 2);
      if (d < 0) sel.y = fq29_neg(sel.y);
      G1Xyzz29 sum = acc;
      xyzz29_add_fast(sum, sel);
      acc = started ? sum : sel;
      started = true;
    }
  }
  return acc;
}

// lane (butterfly, half h): |e_h| * (+-phi^h(b)) with e the canonical scalar `ew`; the stored identity when the half
// contributes nothing (b the identity, or e_h = 0)
template <class SCR>
SNARKV_HD G1Xyzz29 g1_ntt_lane_mul(const uint32_t bw[16], const uint32_t ew[8], uint32_t h, SCR& scr) {
  G1Affine29 q = g1a29_from_canonical(bw);
  uint32_t halves[8], mag[4];
  glv_decompose(ew, halves);
  for (int w = 0; w < 4; ++w) mag[w] = h ? halves[4 + w] : halves[w];
  const uint32_t neg = mag[3] >> 31;
  mag[3] &= 0x7FFFFFFFu;
  if (g1a29_is_identity(q) || (mag[0] | mag[1] | mag[2] | mag[3]) == 0) return xyzz29_identity();
  if (h) q.x = fq29_canon_residue(fq29_mul(q.x, g1_ntt_beta()));
  if (neg) q.y = fq29_neg(q.y);
  G1Xyzz29 r = g1_ntt_window_mul(q, mag[0], mag[1], mag[2], mag[3], scr);
  if (xyzz29_is_degenerate(r)) {  // P = +-Q met on the way (or a true identity): bit-serial, every case spelled out
    const uint32_t m[4] = {mag[0], mag[1], mag[2], mag[3]};
    r = g1_29_scalar_mul<true, 4>(q, m);
    if (!xyzz29_is_identity(r) && xyzz29_is_degenerate(r)) r = xyzz29_identity();
  }
  return r;
}

// out = a + t or (minus) a - t, t = r0 + r1 the two halves; `aw` null: a is the identity.  Canonical affine words out.
SNARKV_HD void g1_ntt_lane_out(const uint32_t* aw, const G1Xyzz29& r0, const G1Xyzz29& r1, bool minus, uint32_t ow[16]) {
  G1Xyzz29 t = r0;
  xyzz29_add_careful(t, r1);
  if (minus) t.y = fq29_neg(t.y);
  if (aw) xyzz29_madd_careful(t, g1a29_from_canonical(aw));
  g1a29_to_canonical(xyzz29_to_affine(t), ow);
}

}  // namespace snarkv
