// Host build of the pass body of the transform over group elements (snark-verifier_amd/csrc/g1_ntt.h, the SNARKV_HD source the
// device compiles), driven the way k_g1_ntt_mul and k_g1_ntt_combine drive it: per butterfly the two lanes' halves of w^e * b
// first, then each output's lane from both halves and `a`; pass after pass between two buffers, and for the inverse direction the pass that
// multiplies every element by n^-1.  Points are canonical affine, 16 words each, the identity all zero.  One library per curve
// (-DSNARKV_CURVE_PALLAS), built by snark-verifier_amd/build.py.  Test infrastructure only.
#include <stdint.h>
#include <string.h>
#include <vector>
#include "../../snark-verifier_amd/csrc/g1_ntt.h"

using namespace snarkv;

namespace {

struct HostScratch {
  G1Xyzz29 tab[3];
  int8_t dig[kWinDigits];
  void tab_put(int e, const G1Xyzz29& v) { tab[e] = v; }
  G1Xyzz29 tab_get(int e) const { return tab[e]; }
  void dig_put(int i, int d) { dig[i] = (int8_t)d; }
  int dig_get(int i) const { return dig[i]; }
};

Fr29 root_of(uint32_t k, uint32_t direction) { return ntt_root_squared(direction == 1, SNARKV_FR_TWO_ADICITY - k); }

}  // namespace

extern "C" {

const char* hg_curve() {
#if defined(SNARKV_CURVE_PALLAS)
  return "pallas";
#else
  return "bn254";
#endif
}

uint32_t hg_max_k() { return kG1NttMaxK; }

// out5 = a, b, lo, hi, e of butterfly j in pass s of a transform of 2^k
void hg_bfly(uint32_t k, uint32_t s, uint32_t j, uint32_t* out5) {
  const G1NttBfly f = g1_ntt_bfly(k, s, j);
  out5[0] = f.a, out5[1] = f.b, out5[2] = f.lo, out5[3] = f.hi, out5[4] = f.e;
}

// the canonical words of w^j (direction 1: of w^-j) and of 2^-k
void hg_twiddle(uint32_t k, uint32_t direction, uint32_t j, uint32_t* out8) { g1_ntt_twiddle(root_of(k, direction), j, out8); }
void hg_n_inverse(uint32_t k, uint32_t* out8) { g1_ntt_n_inverse(k, out8); }

// pass s of a transform of 2^k: in16, out16 = 2^k x 16 words, disjoint
void hg_pass(const uint32_t* in16, uint32_t* out16, uint32_t k, uint32_t s, uint32_t direction) {
  const Fr29 w = root_of(k, direction);
  for (uint32_t j = 0; j < (1u << k) / 2; ++j) {
    const G1NttBfly f = g1_ntt_bfly(k, s, j);
    G1Xyzz29 r[2];
    if (s == 0) {  // the twiddle is 1: nothing to multiply
      r[0] = xyzz29_from_affine(g1a29_from_canonical(in16 + 16 * f.b));
      r[1] = xyzz29_identity();
    } else {
      uint32_t ew[8];
      g1_ntt_twiddle(w, f.e, ew);
      for (uint32_t h = 0; h < 2; ++h) {
        HostScratch scr;
        r[h] = g1_ntt_lane_mul(in16 + 16 * f.b, ew, h, scr);
      }
    }
    g1_ntt_lane_out(in16 + 16 * f.a, r[0], r[1], false, out16 + 16 * f.lo);
    g1_ntt_lane_out(in16 + 16 * f.a, r[0], r[1], true, out16 + 16 * f.hi);
  }
}

// out[j] = e * in[j], e = the canonical scalar ew8; `count` points
void hg_scale(const uint32_t* in16, uint32_t* out16, uint32_t count, const uint32_t* ew8) {
  for (uint32_t j = 0; j < count; ++j) {
    G1Xyzz29 r[2];
    for (uint32_t h = 0; h < 2; ++h) {
      HostScratch scr;
      r[h] = g1_ntt_lane_mul(in16 + 16 * j, ew8, h, scr);
    }
    g1_ntt_lane_out(nullptr, r[0], r[1], false, out16 + 16 * j);
  }
}

// the whole transform as the device call runs it; io16 in place
void hg_transform(uint32_t* io16, uint32_t k, uint32_t direction) {
  const size_t words = (size_t)16 << k;
  std::vector<uint32_t> a(io16, io16 + words), b(words);
  for (uint32_t s = 0; s < k; ++s) {
    hg_pass(a.data(), b.data(), k, s, direction);
    a.swap(b);
  }
  if (direction == 1 && k > 0) {
    uint32_t ninv[8];
    g1_ntt_n_inverse(k, ninv);
    hg_scale(a.data(), b.data(), 1u << k, ninv);
    a.swap(b);
  }
  memcpy(io16, a.data(), words * 4);
}

}  // extern "C"
