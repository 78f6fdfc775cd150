// Lane-level pieces of the workgroup-cooperative pairing on the lazy 9x29-bit
// field: the arithmetic the shipped `k_decide` uses.
//
// Why 29-bit here too: on the exact 8x32 field every signed sum of a reduction
// is a dependent carry chain, and gfx950 needs two wait states between a VALU
// writing a carry and the VALU consuming it -- the cheap-looking additions cost
// as much as the products.  In the lazy form a sum is nine independent
// `v_add_u32`, and one float-estimated quotient (`fq29_reduce_small`) squeezes
// the up-to-22-term coefficient back to within (1/2 + 2^-13) p.
//
// STORED: the invariant of a coefficient c held in LDS by k_decide: carry-normalised and
// |c| < 2.05 p (proven).  coop3_finalize leaves |c| <= (1/2 + 2^-13) p (seen: 0.50001 p), but
// coop_frob / coop_scale store fq2_scale_norm, an UNSQUEEZED sum or difference of two
// single products, proven inside (-1.025 p, 2.025 p) (seen: -0.993 p .. 1.999 p), and coop_conj
// negates such a value.  Both operands of a product stay inside the multiplier budget
// (|limb| < 2^29), and every fused two-product value -- here and in decide_w.h, whose xi
// copies reach 10.1 p -- inside (-p/8, 9p/8) (seen: -0.070 p .. 1.064 p): the ONE range
// of a fused two-product output.  tests/fq29_model.py section 4 derives these sets from
// the producers and checks every piece on raw limbs at their corners.
#pragma once
#include "fq29.h"

namespace snarkv {

struct Fq2_29 {
  Fq29 c0, c1;
};

SNARKV_HD Fq2_29 frob29_gamma(int k, int i) {
  constexpr int32_t g1[5][2][9] = BN254_FROB29_GAMMA_1;
  constexpr int32_t g2[5][2][9] = BN254_FROB29_GAMMA_2;
  constexpr int32_t g3[5][2][9] = BN254_FROB29_GAMMA_3;
  Fq2_29 r;
  for (int l = 0; l < 9; ++l) {
    r.c0.v[l] = (k == 1) ? g1[i - 1][0][l] : (k == 2) ? g2[i - 1][0][l] : g3[i - 1][0][l];
    r.c1.v[l] = (k == 1) ? g1[i - 1][1][l] : (k == 2) ? g2[i - 1][1][l] : g3[i - 1][1][l];
  }
  return r;
}

// ---------------------------------------------------------------------------
// The round `k_decide` runs ("coop3"; the first version of this round, 204 single
// products + two LDS reduction stages driven by generated tables, was 1.5x slower).
//
// A = sum_i (a[2i] + a[2i+1] u) w^i, same for B.  With V(k') = sum_{i1+i2=k'}
// a_{i1} b_{i2} (an Fq2 value, k' = 0..10) the product is
//     out(k) = V(k) + xi V(k+6)   (k = 0..4),   out(5) = V(5),   xi = 9 + u.
// Lane l = 16 k + 8 e + j  (k = output power of w, e = power of u, j < 6):
//     j <= k : the LOW pair  (i1, i2) = (j, k - j)
//     j >  k : the HIGH pair (i1, i2) = (j, k + 6 - j)       [i1 + i2 = k + 6]
// and each lane computes ONE Fq2-coefficient of its pair as a fused two-product
// Montgomery step (fq29_mul2):   e = 0: a0 b0 - a1 b1     e = 1: a0 b1 + a1 b0.
// 72 active lanes (of 96 = 1.5 wavefronts) instead of 204 products, and the
// reduction needs no LDS: low and high sums are butterflies inside the 8-lane
// group (DPP), the partner coefficient of xi V sits 8 lanes away (row_ror:8),
// and lane j = 0 of each group applies   low + 9 hi_e -/+ hi_(1-e)   in one
// 64-bit carry chain followed by the float-estimated squeeze.
// Invariant of a stored coefficient: STORED above.
struct Coop3Lane {
  int k, e, i1, i2;
  bool active, high;
};

SNARKV_HD Coop3Lane coop3_lane(int lane) {
  Coop3Lane L;
  L.k = lane >> 4;
  L.e = (lane >> 3) & 1;
  int j = lane & 7;
  L.active = L.k < 6 && j < 6;
  L.high = j > L.k;
  L.i1 = j;
  L.i2 = L.high ? L.k + 6 - j : L.k - j;
  if (!L.active) {
    L.i1 = 0;
    L.i2 = 0;
  }
  return L;
}

// the lane's fused product  a0*y0 + (+-a1)*y1  with  y0 = b[2 i2 + e],
// y1 = b[2 i2 + 1 - e] (the caller picks them by address, so both u-powers run
// the same instruction stream):   e = 0: a0 b0 - a1 b1     e = 1: a0 b1 + a1 b0
SNARKV_HD Fq29 coop3_product(int e, const Fq29& a0, const Fq29& a1, const Fq29& y0, const Fq29& y1) {
  Fq29 x1;
  int32_t m = e - 1;  // e = 0: all ones -> negate
#pragma unroll
  for (int i = 0; i < 9; ++i) x1.v[i] = (a1.v[i] ^ m) - m;
  return fq29_mul2(a0, y0, x1, y1);
}

// lo, hi, hp: limb-wise sums of <= 6 carry-normalised products (limbs 0..7
// read as UNSIGNED: up to 6 * 2^29; limb 8 signed); hp = the high sum of the
// other u-power.  Returns low + 9 hi - hp (e = 0) or low + 9 hi + hp (e = 1),
// carry-normalised and squeezed to within (1/2 + 2^-13) p (seen: 0.50001 p).  With k + 1 low
// and 5 - k high terms in (-p/8, 9p/8) the sum lies in (-11.4 p, 57.4 p) (proven; seen: -11.375 p .. 57.375 p).
SNARKV_HD Fq29 coop3_finalize(int e, const Fq29& lo, const Fq29& hi, const Fq29& hp) {
  Fq29 t;
  int64_t c = 0;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    int64_t x = (int64_t)(uint32_t)lo.v[i] + 9 * (int64_t)(uint32_t)hi.v[i];
    int64_t y = (int64_t)(uint32_t)hp.v[i];
    x += e ? y : -y;
    x += c;
    t.v[i] = (int32_t)x & kMask29;
    c = x >> 29;
  }
  {
    int64_t x = (int64_t)lo.v[8] + 9 * (int64_t)hi.v[8] + (e ? (int64_t)hp.v[8] : -(int64_t)hp.v[8]) + c;
    t.v[8] = (int32_t)x;
  }
  return fq29_reduce_small(t);
}

// (x + y u)(g0 + g1 u) = (x g0 - y g1) + (x g1 + y g0) u, component e; every product N, so the lazy sum stays < 2^30
SNARKV_HD Fq29 fq2_scale_lane(const Fq29& x, const Fq29& y, const Fq29& g0, const Fq29& g1, int e) {
  return e ? fq29_add(fq29_mul(x, g1), fq29_mul(y, g0)) : fq29_sub(fq29_mul(x, g0), fq29_mul(y, g1));
}
// what coop_frob and coop_scale (decider.hip) store: the carry-normalised sum or difference of two single products, each
// in a b / 2^261 + [0, p).  NOT squeezed: the sum (e = 1) reaches 2 p, the difference (e = 0) -p, see STORED above.
SNARKV_HD Fq29 fq2_scale_norm(const Fq29& x, const Fq29& y, const Fq29& g0, const Fq29& g1, int e) {
  return fq29_norm(fq2_scale_lane(x, y, g0, g1, e));
}

#if defined(__HIPCC__)
// ---- device only: the lane exchanges of the rounds (decider.hip; tests/devtest/devtest.hip runs the same text) ----------
// DPP lane exchange inside a 16-lane row (no LDS, no barrier)
template <int CTRL>
static __device__ __forceinline__ uint32_t dpp_u32(uint32_t x) {
  return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, CTRL, 0xF, 0xF, true);
}

// every lane of an aligned 8-lane group gets the limb-wise sum over the group
// (limbs as unsigned: <= 6 live terms of < 2^29 each)
static __device__ __forceinline__ Fq29 group8_sum(Fq29 x) {
#pragma unroll
  for (int i = 0; i < 9; ++i) x.v[i] = (int32_t)((uint32_t)x.v[i] + dpp_u32<0xB1>((uint32_t)x.v[i]));   // quad_perm [1,0,3,2]
#pragma unroll
  for (int i = 0; i < 9; ++i) x.v[i] = (int32_t)((uint32_t)x.v[i] + dpp_u32<0x4E>((uint32_t)x.v[i]));   // quad_perm [2,3,0,1]
#pragma unroll
  for (int i = 0; i < 9; ++i) x.v[i] = (int32_t)((uint32_t)x.v[i] + dpp_u32<0x141>((uint32_t)x.v[i]));  // row_half_mirror
  return x;
}
#endif

}  // namespace snarkv
