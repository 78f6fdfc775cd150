// The decomposition of a 2^k-point transform into passes over tiles of at most 2^T elements: index arithmetic only, the
// same source for the kernels of ntt.hip and for the host (tests/hosttest/hosttest_ntt.cpp, any T), as poly_scan.h.
//
// Cooley-Tukey with one digit per pass.  k = t_0 + ... + t_{P-1}; the input index is read most significant digit first,
//   j = j_0 2^{s_0} + j_1 2^{s_1} + ... + j_{P-1},   s_p = k - (t_0 + ... + t_p)   (s_{P-1} = 0)
// and the output index least significant digit first,
//   i = i_0 + i_1 2^{a_1} + ... + i_{P-1} 2^{a_{P-1}},   a_p = t_0 + ... + t_{p-1}.
// Pass p turns digit j_p into i_p where it stands (a 2^{t_p}-point transform over elements 2^{s_p} apart) and then multiplies
// the element by w_n^(i_p * lo * 2^{a_p}), lo = the s_p bits below the digit, which still are input digits: the four-step
// form, once per element.  Passes before the last store every element where they loaded it, so they may run in place; the
// last pass stores at i, which is the one digit reversal (out of place: it reads the working buffer and writes the output).
//
// A tile is all positions that differ in two bit fields: the digit (t_p bits at s_p, the rows) and c_p further bits (the
// columns), c_p = T - t_p clamped to what is there.  Before the last pass the columns are the lowest bits of the position, so
// a row is a run of 2^{c_p} consecutive elements; in the last pass the rows are the lowest bits (a run of 2^{t_p} consecutive
// elements on load) and the columns are the lowest bits of i_0, which are the lowest bits of the output index: a run of
// 2^{c_p} consecutive elements on store.  With more than one pass a pass takes at most T - C levels, so that every run is at
// least 2^C elements (128 bytes at C = 2); the levels are spread evenly over the passes.  A transform of k <= T is one pass
// of one tile with no columns.
//
// In LDS an element sits at (row << c) | col.  The levels are decimation in time: the load puts digit value d at row
// bitrev(d), level l pairs rows that differ in bit l, and row i_p holds output digit i_p at the end.
#pragma once
#include <stdint.h>
#include "fq29.h"  // SNARKV_HD

namespace snarkv {

constexpr uint32_t kNttMaxPasses = 32;

template <uint32_t T, uint32_t C>
struct NttPlan {
  static_assert(T >= 1 && C < T && T <= 12, "a pass of several passes takes T - C >= 1 levels");
  uint32_t k, passes;
  uint8_t t[kNttMaxPasses];  // levels of pass p
  uint8_t s[kNttMaxPasses];  // bit offset of its digit in the position
  uint8_t a[kNttMaxPasses];  // bit offset of its digit in the output index
  uint8_t c[kNttMaxPasses];  // column bits of its tiles

  SNARKV_HD explicit NttPlan(uint32_t k_) : k(k_) {
    for (uint32_t p = 0; p < kNttMaxPasses; ++p) t[p] = s[p] = a[p] = c[p] = 0;
    if (k <= T) {
      passes = 1;
      t[0] = (uint8_t)k;
      return;
    }
    passes = (k + (T - C) - 1) / (T - C);
    uint32_t done = 0;
    for (uint32_t p = 0; p < passes; ++p) {
      t[p] = (uint8_t)(k / passes + (p < k % passes ? 1u : 0u));
      a[p] = (uint8_t)done;
      done += t[p];
      s[p] = (uint8_t)(k - done);
    }
    for (uint32_t p = 0; p < passes; ++p) {
      const uint32_t room = p + 1 < passes ? s[p] : t[0];  // the bits the columns are taken from
      c[p] = (uint8_t)(T - t[p] < room ? T - t[p] : room);
    }
  }

  SNARKV_HD bool last(uint32_t p) const { return p + 1 == passes; }
  SNARKV_HD uint32_t slots(uint32_t p) const { return 1u << (t[p] + c[p]); }
  SNARKV_HD uint32_t tiles(uint32_t p) const { return 1u << (k - t[p] - c[p]); }
  // bit offset of the columns in the position
  SNARKV_HD uint32_t col_at(uint32_t p) const { return last(p) && passes > 1 ? s[0] : 0u; }

  SNARKV_HD static uint32_t spread(uint32_t x, uint32_t at, uint32_t width) {  // `width` zero bits inserted at `at`
    return ((x >> at) << (at + width)) | (x & ((1u << at) - 1u));
  }
  SNARKV_HD static uint32_t bitrev(uint32_t x, uint32_t bits) {
    uint32_t r = 0;
    for (uint32_t i = 0; i < bits; ++i) r |= ((x >> i) & 1u) << (bits - 1 - i);
    return r;
  }
  // the position of (row 0, column 0) of tile g: the lower field is opened first, the upper one in final coordinates
  SNARKV_HD uint32_t tile_base(uint32_t p, uint32_t g) const {
    if (last(p)) return passes > 1 ? spread(spread(g, 0, t[p]), s[0], c[p]) : 0u;
    return spread(spread(g, 0, c[p]), s[p], t[p]);
  }
  SNARKV_HD uint32_t position(uint32_t p, uint32_t g, uint32_t row, uint32_t col) const {
    return tile_base(p, g) | (row << s[p]) | (col << col_at(p));
  }
  // load slot -> (row, column): consecutive slots are consecutive positions, 2^c at a time (2^t in the last pass)
  SNARKV_HD uint32_t load_row(uint32_t p, uint32_t slot) const { return last(p) ? slot & ((1u << t[p]) - 1u) : slot >> c[p]; }
  SNARKV_HD uint32_t load_col(uint32_t p, uint32_t slot) const { return last(p) ? slot >> t[p] : slot & ((1u << c[p]) - 1u); }
  SNARKV_HD uint32_t load_index(uint32_t p, uint32_t g, uint32_t slot) const {
    return position(p, g, load_row(p, slot), load_col(p, slot));
  }
  SNARKV_HD uint32_t load_lds(uint32_t p, uint32_t slot) const {
    return (bitrev(load_row(p, slot), t[p]) << c[p]) | load_col(p, slot);
  }
  // store slot -> (row, column) is the LDS index itself: columns fastest
  SNARKV_HD uint32_t store_lds(uint32_t, uint32_t slot) const { return slot; }
  SNARKV_HD uint32_t store_row(uint32_t p, uint32_t slot) const { return slot >> c[p]; }
  SNARKV_HD uint32_t store_col(uint32_t p, uint32_t slot) const { return slot & ((1u << c[p]) - 1u); }
  // the output index of a position after the last pass: digit q moves from s_q to a_q
  SNARKV_HD uint32_t natural(uint32_t pos) const {
    uint32_t i = 0;
    for (uint32_t q = 0; q < passes; ++q) i |= ((pos >> s[q]) & ((1u << t[q]) - 1u)) << a[q];
    return i;
  }
  SNARKV_HD uint32_t store_index(uint32_t p, uint32_t g, uint32_t slot) const {
    const uint32_t pos = position(p, g, store_row(p, slot), store_col(p, slot));
    return last(p) ? natural(pos) : pos;
  }
  // exponent of w_n in the factor between pass p and the next: i_p * lo * 2^{a_p} < n
  SNARKV_HD uint32_t twiddle_exp(uint32_t p, uint32_t g, uint32_t slot) const {
    const uint32_t pos = position(p, g, store_row(p, slot), store_col(p, slot));
    return (store_row(p, slot) * (pos & ((1u << s[p]) - 1u))) << a[p];
  }
  // butterfly b of level l (b < slots / 2): the LDS indices of its two elements and the index of its factor in the table of
  // the 2^{T-1} powers of w_{2^T} (w_{2^{l+1}}^pos = w_{2^T}^(pos 2^{T-1-l}))
  SNARKV_HD uint32_t bfly_top(uint32_t p, uint32_t level, uint32_t b) const {
    const uint32_t col = b & ((1u << c[p]) - 1u), q = b >> c[p];
    const uint32_t row = ((q >> level) << (level + 1)) | (q & ((1u << level) - 1u));
    return (row << c[p]) | col;
  }
  SNARKV_HD uint32_t bfly_distance(uint32_t p, uint32_t level) const { return 1u << (level + c[p]); }
  SNARKV_HD uint32_t bfly_twiddle(uint32_t p, uint32_t level, uint32_t b) const {
    return ((b >> c[p]) & ((1u << level) - 1u)) << (T - 1 - level);
  }
  // the two-level table of the n powers of w_n (and of the shift): e = hi 2^h + lo
  SNARKV_HD uint32_t split_bits() const { return (k + 1) / 2; }
};

}  // namespace snarkv
