// Per-lane body of the folded IPA decide (ipa_fold.hip): the coefficients of
//     h[j] = sum_{i < m} rho^i prod over the set bits b of j of xi_i[k-1-b]
// with the products of the HIGH bits shared.  A lane owns the 2^T consecutive coefficients j = lane 2^T + q, q < 2^T.
// Per accumulator i it forms w = rho^i prod over the set bits of `lane` of xi_i[k-1-(T+b)] once, expands the 2^T products
// of the low bits from w (level b multiplies the 2^b values so far by xi_i[k-1-b]: 2^T - 1 products) and ADDS them into
// its 2^T running sums: (popcount(lane) + 2^T) / 2^T products per coefficient instead of popcount(j) + 1.
//
// Ranges (fr29.h): every product is carry-normalised with a value in (-r/2, 3r/2).  A running sum is carry-normalised after
// each addition and brought back to (-r/2, 3r/2) by a product with one after kFoldReduceEvery = 32 additions: a sum is then
// below 33 x 1.5 r < 64 r in magnitude -- limb 8 stays below 2^29 -- and a x one < 64 r^2, which is what fr29_mul's bound
// on its result needs.  The sums leave the function reduced, so up to 32 of them add up the same way (fold_sum_partials).
// Same source for the device kernels and for the host test library (tests/hosttest/hosttest_fold.cpp).
#pragma once
#include <stddef.h>
#include "fr29.h"

namespace snarkv {

constexpr int kFoldT = 3;                     // a lane's block: 2^3 sums x 9 limbs
constexpr uint32_t kFoldReduceEvery = 32;     // additions into a sum between two reductions

SNARKV_HD Fr29 fold_reduce(const Fr29& a) { return fr29_mul(fr29_norm(a), fr29_one()); }
SNARKV_HD Fr29 fold_add(const Fr29& a, const Fr29& b) { return fr29_norm(fr29_add(a, b)); }

template <int I>
struct FoldIdx {
  static constexpr int value = I;
};
// f(FoldIdx<I>) for I in [B, E): indices that are constants from the start keep the arrays below in registers
template <int B, int E, class F>
SNARKV_HD void fold_static_for(F&& f) {
  if constexpr (B < E) {
    f(FoldIdx<B>{});
    fold_static_for<B + 1, E>(f);
  }
}

// sums[q] = sum_{i0 <= i < i1} pw[i] prod over the set bits b of j = lane 2^T + q of xi[i k + k-1-b], q < min(2^T, 2^k);
// xi = m x k challenges and pw = the powers rho^i, both as products leave them (Montgomery, (-r/2, 3r/2)).  lane < max(1,
// 2^k >> T).  A key below a block (k < T) has the levels b >= k skipped: the sums q >= 2^k stay zero and are not part of h.
template <int T>
SNARKV_HD void ipa_fold_lane(const Fr29* xi, const Fr29* pw, uint32_t k, uint32_t lane, uint32_t i0, uint32_t i1,
                             Fr29 (&sums)[1 << T]) {
  constexpr int N = 1 << T, H = T > 0 ? (1 << (T - 1)) : 1;
  fold_static_for<0, N>([&](auto q) { sums[q.value] = fr29_zero(); });
  uint32_t since = 0;
#pragma unroll 1
  for (uint32_t i = i0; i < i1; ++i) {
    const Fr29* x = xi + (size_t)i * k;
    Fr29 e[H];  // the products of the levels below the last: those of the last level go straight into their sums
    fold_static_for<0, H>([&](auto q) { e[q.value] = fr29_zero(); });
    e[0] = pw[i];
#pragma unroll 1
    for (uint32_t b = T; b < k; ++b)
      if ((lane >> (b - T)) & 1u) e[0] = fr29_mul(e[0], x[k - 1 - b]);
    sums[0] = fold_add(sums[0], e[0]);
    fold_static_for<0, T>([&](auto lv) {
      constexpr int b = lv.value;
      if ((uint32_t)b < k) {
        const Fr29 xb = x[k - 1 - b];
        fold_static_for<0, (1 << b)>([&](auto q) {
          const Fr29 v = fr29_mul(e[q.value], xb);
          if constexpr (b + 1 < T) e[(1 << b) + q.value] = v;
          sums[(1 << b) + q.value] = fold_add(sums[(1 << b) + q.value], v);
        });
      }
    });
    if (++since == kFoldReduceEvery) {
      since = 0;
      fold_static_for<0, N>([&](auto q) { sums[q.value] = fold_reduce(sums[q.value]); });
    }
  }
  fold_static_for<0, N>([&](auto q) { sums[q.value] = fold_reduce(sums[q.value]); });
}

// the second pass: the sum of `count` reduced partials `stride` elements apart, reduced
SNARKV_HD Fr29 fold_sum_partials(const Fr29* parts, size_t stride, uint32_t count) {
  Fr29 acc = fr29_zero();
  uint32_t since = 0;
#pragma unroll 1
  for (uint32_t s = 0; s < count; ++s) {
    acc = fold_add(acc, parts[(size_t)s * stride]);
    if (++since == kFoldReduceEvery) {
      since = 0;
      acc = fold_reduce(acc);
    }
  }
  return fold_reduce(acc);
}

// accumulators [fold_slice_begin(s), fold_slice_begin(s + 1)) belong to slice s of S <= m: no slice is empty
SNARKV_HD uint32_t fold_slice_begin(uint32_t s, uint32_t S, uint32_t m) { return (uint32_t)(((uint64_t)s * m) / S); }

}  // namespace snarkv
