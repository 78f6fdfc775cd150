// The host's few scalars of the multi-open provers (ipa_multiopen.hip, kzg_multiopen_plan.h): Fr29 in the Montgomery domain,
// every result brought back to (-r/8, 9r/8), so that sums and products of any length stay in fr29_mul's range.  Host only
// and free of HIP types: plain C++ over fr29.h, which the host compiles alone (tests/hosttest/hosttest_kzg_open.cpp).
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>
#include <vector>
#include "fr29.h"

namespace snarkv {

inline Fr29 h_red(const Fr29& x) { return fr29_mul(fr29_norm(x), fr29_one()); }
inline Fr29 h_load(const uint8_t* b32) {
  uint32_t w[8];
  memcpy(w, b32, 32);
  return h_red(fr29_from_canonical(w));
}
inline void h_store(uint8_t* b32, const Fr29& v) {
  uint32_t w[8];
  fr29_to_canonical(v, w);
  memcpy(b32, w, 32);
}
inline Fr29 h_add(const Fr29& a, const Fr29& b) { return h_red(fr29_add(a, b)); }
inline Fr29 h_sub(const Fr29& a, const Fr29& b) {
  Fr29 d;
  for (int i = 0; i < 9; ++i) d.v[i] = a.v[i] - b.v[i];
  return h_red(d);
}
inline Fr29 h_mul(const Fr29& a, const Fr29& b) { return h_red(fr29_mul(a, b)); }
inline bool h_is_zero(const Fr29& v) {
  uint8_t b[32];
  h_store(b, v);
  for (int i = 0; i < 32; ++i)
    if (b[i]) return false;
  return true;
}
inline Fr29 h_inv(const Fr29& x) {  // x^(r-2)
  constexpr uint32_t rw[8] = SNARKV_FR_R_LIMBS;
  uint32_t e[8], borrow = 2;
  for (int i = 0; i < 8; ++i) {
    e[i] = rw[i] - borrow;
    borrow = rw[i] < borrow ? 1u : 0u;
  }
  Fr29 acc = fr29_one();
  for (int b = 255; b >= 0; --b) {
    acc = h_mul(acc, acc);
    if ((e[b >> 5] >> (b & 31)) & 1u) acc = h_mul(acc, x);
  }
  return acc;
}
inline std::vector<Fr29> h_powers(const Fr29& x, size_t count) {
  std::vector<Fr29> out(count, fr29_one());
  for (size_t i = 1; i < count; ++i) out[i] = h_mul(out[i - 1], x);
  return out;
}

// the coefficients of the polynomial of degree < m through (pts[j], vals[j]); false when two points coincide
inline bool h_interpolate(const std::vector<Fr29>& pts, const std::vector<Fr29>& vals, std::vector<Fr29>& out) {
  const size_t m = pts.size();
  out.assign(m, fr29_zero());
  for (size_t j = 0; j < m; ++j) {
    std::vector<Fr29> num(1, fr29_one());
    Fr29 den = fr29_one();
    for (size_t i = 0; i < m; ++i) {
      if (i == j) continue;
      std::vector<Fr29> next(num.size() + 1, fr29_zero());  // num (X - p_i)
      for (size_t t = 0; t < num.size(); ++t) {
        next[t + 1] = h_add(next[t + 1], num[t]);
        next[t] = h_sub(next[t], h_mul(pts[i], num[t]));
      }
      num.swap(next);
      den = h_mul(den, h_sub(pts[j], pts[i]));
    }
    if (h_is_zero(den)) return false;
    const Fr29 f = h_mul(vals[j], h_inv(den));
    for (size_t t = 0; t < m; ++t) out[t] = h_add(out[t], h_mul(num[t], f));
  }
  return true;
}

}  // namespace snarkv
