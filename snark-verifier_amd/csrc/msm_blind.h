// The blind term of a blinded commitment, blind * S, in the form of the shared-key MSM (msm_shared.hip): against the 32 rows
//     T[w] = 2^(8 w) S,  w < 32   (k_shared_table over the one-point key {S}: packed Montgomery affine, identity = zero row)
// and the signed 8-bit digits d_w of the blind (msm_shared.h, after its reduction mod r),
//     blind * S = sum_w d_w T[w].
// One wavefront per blind: lane w < 32 forms |d_w| T[w] by double-and-add over the 8 bits of |d_w| <= 128 (at most 7
// doublings and 7 additions after the leading bit), negated by the digit's sign; the 32 lane points are folded by a tree of
// 5 levels into ONE XYZZ partial, which the fold of the MSM's slices takes as one more slice (k_shared_blind).
//
// No carry leaves window 31: the recoded value is below r < 2^255 (msm_shared.h), so the 32 rows suffice.
//
// Lazy bounds (the sets of g1_29.h).  A row is a canonical affine point (limbs in [0, 2^29)); negating its y gives limbs in
// (-2^29, 0], which is what xyzz29_from_affine / xyzz29_madd_* take from k_shared_msm's entries as well.  The accumulator
// starts as xyzz29_from_affine (x, y canonical or negated canonical, zz = zzz = 1: inside S) and only meets xyzz29_double and
// xyzz29_madd_careful, under which S is closed; the fold only applies xyzz29_add_careful to members of S.  So every lane
// point, every level of the tree and the partial are in S, the form k_final reads.
//
// Exceptional cases.  For S of order r an accumulator j T[w], 2 <= j < 128, never equals +-T[w]; partial sums of the tree can
// still meet (sums of digits times powers of 2^8 that agree mod r), and an S off the curve or rows that repeat (the host
// test's: S and -S, S and S in one level) meet at once.  The additions are the careful ones throughout -- 32 lanes a blind is
// no hot loop -- so nothing is assumed about S or the rows.
// Same source for the device kernel and for the host test library (tests/hosttest/hosttest_blind.cpp).
#pragma once
#include "g1_29.h"
#include "msm_shared.h"

namespace snarkv {

// digit w of a value already below r (shared_reduce_mod_r)
SNARKV_HD int blind_digit(const uint32_t s[8], int w) {
  int r = 0;
  shared_recode_each(s, [&](int i, int d) {
    if (i == w) r = d;
  });
  return r;
}

// d * row, |d| <= 128: the stored identity for d = 0 or an identity row
SNARKV_HD G1Xyzz29 blind_lane_point(const G1Packed& row, int d) {
  const uint32_t mag = (uint32_t)(d < 0 ? -d : d);
  G1Affine29 p = g1a29_unpack(row);
  G1Xyzz29 acc = xyzz29_identity();
  if (mag == 0 || g1a29_is_identity(p)) return acc;
  if (d < 0) p.y = fq29_neg(p.y);
  bool started = false;
#pragma unroll 1
  for (int b = kSharedC - 1; b >= 0; --b) {
    if (started && !xyzz29_is_identity(acc)) acc = xyzz29_double(acc);
    if ((mag >> b) & 1u) {
      if (started) xyzz29_madd_careful(acc, p);
      else acc = xyzz29_from_affine(p);
      started = true;
    }
  }
  return xyzz29_sanitize(acc);
}

// lane's part of one level of the fold over sh[0 .. 2 half): sh[lane] += sh[lane + half] for lane < half.  A level reads
// only what no lane of that level writes; the caller separates the levels (a barrier on the device, a loop on the host).
SNARKV_HD void blind_fold_level(G1Xyzz29* sh, uint32_t lane, uint32_t half) {
  if (lane >= half) return;
  G1Xyzz29 a = sh[lane];
  xyzz29_add_careful(a, sh[lane + half]);
  sh[lane] = xyzz29_sanitize(a);
}

}  // namespace snarkv
