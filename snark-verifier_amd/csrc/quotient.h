// The quotient's gate program (include/snarkv_quotient.h): the decoding of an operand word, the row a rotation reads, one
// instruction step on a row's register file, and the entries of the vanishing polynomial's table.  Same source for the
// kernels of quotient.hip and for the host (tests/hosttest/hosttest_quotient.cpp), as poly_prod.h.
//
// Values.  The rule of the register file: every value written to a register is carry-normalised (limbs 0..7 in [0, 2^29),
// limb 8 signed) and lies in (-r/2, 3r/2), the range of a fresh fr29_mul result (fr29.h).  An operand is one of
//   register   by the rule
//   constant   staged as fr29_from_canonical of a canonical scalar: a fresh product
//   column     fr29_from_canonical of 8 words below 2^256 < 8r: a fresh product
// so both sides of every fr29_mul here are fresh products, inside the |x| < 8r and the 2^29.8 per limb it takes; with
// |a|, |b| < 3r/2 its result a b / 2^261 + [0, r) lies in (-0.02r, 1.02r) (r < 2^254.01).
//   MUL        a fresh product
//   ADD, SUB   a +- b limb by limb: the value in (-2r, 3r), limbs below 2^30 in size, limb 8 far below 2^31.  quot_reduce
//   FMA        a b + c, a product plus an operand: (-r, 3r), the same.               brings it to [0, r), normalised
// quot_reduce is exact integer work, no product: normalise (the sign of a normalised value is the sign of limb 8, the lower
// limbs being non-negative and below 2^232 together), add 2r to a negative value ((-2r, 0) -> (0, 2r); the others stay in
// [0, 3r)), then subtract r while the result stays non-negative, twice: [0, r).  So a sum never meets a multiplier, and the
// last register goes out through fr29_to_canonical, which takes |x| < 8r.  tests/test_quotient_model.py runs every op with
// every operand r - 1 (and with the words of r and of 2^256 - 1 in the columns).
#pragma once
#include <stddef.h>
#include <stdint.h>
#include "../../include/snarkv_quotient.h"
#include "fr29.h"
#include "ntt_tile.h"

namespace snarkv {

constexpr uint32_t kQuotKindReg = 0, kQuotKindConst = 1, kQuotKindCol = 2;  // bits 31:30 of an operand word

SNARKV_HD uint32_t quot_kind(uint32_t word) { return word >> 30; }
SNARKV_HD uint32_t quot_index(uint32_t word) { return word & 0x3FFFFFFFu; }  // of a register or a constant
SNARKV_HD uint32_t quot_col(uint32_t word) { return word & 0xFFFFFu; }
SNARKV_HD int32_t quot_rot(uint32_t word) { return (int32_t)(word << 2) >> 22; }  // bits 29:20, sign-extended
SNARKV_HD uint32_t quot_operands(uint32_t op) { return op == SNARKV_QUOT_FMA ? 3u : 2u; }

// (row + rot 2^e) mod 2^log_n, the euclidean remainder: the sum is taken mod 2^32, of which 2^log_n is a divisor
// (log_n <= 30), so a negative or a many-times-wrapping rotation needs no branch
SNARKV_HD uint32_t quot_row(uint32_t row, int32_t rot, uint32_t e, uint32_t log_n) {
  return (row + ((uint32_t)rot << e)) & ((1u << log_n) - 1u);
}

// |x| < 3r as limb-wise sums of normalised values -> the residue in [0, r), normalised (the bounds are at the top)
SNARKV_HD Fr29 quot_reduce(const Fr29& x) {
  Fr29 t = fr29_norm(x);
  const int32_t neg = t.v[8] >> 31;
#pragma unroll
  for (int i = 0; i < 9; ++i) t.v[i] += (2 * fr29_r(i)) & neg;
  t = fr29_norm(t);
#pragma unroll
  for (int pass = 0; pass < 2; ++pass) {
    Fr29 d;
    int32_t c = 0;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const int32_t s = t.v[i] - fr29_r(i) + c;
      d.v[i] = s & kMask29;
      c = s >> 29;
    }
    d.v[8] = t.v[8] - fr29_r(8) + c;
    const int32_t keep = d.v[8] >> 31;
#pragma unroll
    for (int i = 0; i < 9; ++i) t.v[i] = (t.v[i] & keep) | (d.v[i] & ~keep);
  }
  return t;
}

// Cols: load(index) -> the element at `index` of the n_cols x 2^log_n values, in the Montgomery domain
template <class Cols>
SNARKV_HD Fr29 quot_operand(uint32_t word, const Fr29* regs, const Fr29* consts, const Cols& cols, uint32_t row, uint32_t e,
                            uint32_t log_n) {
  const uint32_t kind = quot_kind(word);
  if (kind == kQuotKindReg) return regs[quot_index(word) & (SNARKV_QUOT_REGS - 1u)];
  if (kind == kQuotKindConst) return consts[quot_index(word)];
  return cols.load(((size_t)quot_col(word) << log_n) + quot_row(row, quot_rot(word), e, log_n));
}

// one instruction at one row; the program has been checked (quotient.hip: check_program).  The operands are read before dst
// is written: dst may be one of them.
template <class Cols>
SNARKV_HD void quot_step(const snarkv_quot_instr& ins, Fr29* regs, const Fr29* consts, const Cols& cols, uint32_t row, uint32_t e,
                         uint32_t log_n) {
  const Fr29 a = quot_operand(ins.a, regs, consts, cols, row, e, log_n);
  const Fr29 b = quot_operand(ins.b, regs, consts, cols, row, e, log_n);
  Fr29 v;
  if (ins.op == SNARKV_QUOT_ADD) v = quot_reduce(fr29_add(a, b));
  else if (ins.op == SNARKV_QUOT_SUB) v = quot_reduce(fr29_sub(a, b));
  else if (ins.op == SNARKV_QUOT_MUL) v = fr29_mul(a, b);
  else v = quot_reduce(fr29_add(fr29_mul(a, b), quot_operand(ins.c, regs, consts, cols, row, e, log_n)));
  regs[ins.dst & (SNARKV_QUOT_REGS - 1u)] = v;
}

// The vanishing polynomial on the extended coset: (s W^i)^n - 1 = s^n (W^n)^i - 1, and W^n generates the 2^e domain, so entry
// j = i mod 2^e of a table of 2^e serves every row.  All in the Montgomery domain.
SNARKV_HD Fr29 quot_shift_to_n(const Fr29& s, uint32_t k) {
  Fr29 x = s;
  for (uint32_t i = 0; i < k; ++i) x = fr29_mul(x, x);
  return x;
}
SNARKV_HD Fr29 quot_coset_root(uint32_t e) { return ntt_root_squared(false, SNARKV_FR_TWO_ADICITY - e); }
// products only, then one difference of two fresh products: (-2r, 2r), normalised, on its way to fr29_to_canonical
SNARKV_HD Fr29 quot_vanishing_entry(const Fr29& s_to_n, const Fr29& root, uint32_t j) {
  Fr29 x = root, acc = s_to_n;
  for (; j; j >>= 1) {
    if (j & 1u) acc = fr29_mul(acc, x);
    x = fr29_mul(x, x);
  }
  return fr29_norm(fr29_sub(acc, fr29_one()));
}

// ---------------------------------------------------------------- the join of the coset-at-a-time route
// (include/snarkv_quotient_cosets.h)  in[j][t], j < 2^e, t < n = 2^k: coefficient t of the size-k inverse transform (no shift)
// of the values on the coset (s W^j) H.  For T = t + q n
//   out[T] = s^-T 2^-e sum_j (W^n)^(-j q) (W^(-j t) g_j in[j][t])
// g_j the inverted vanishing entry, or one: the per-coset shifts the inverse transforms did not get, then the 2^e-point
// inverse transform across the cosets, then the shift of the whole.  One tile is 2^tile_bits consecutive t by all 2^e cosets
// in a buffer of Fr29, coset-major: quot_join_in on every slot, e levels of quot_join_butterfly over half the slots each (a
// barrier between levels on the device), quot_join_out on every slot.  The kernel of quotient.hip and the host loop of
// tests/hosttest/hosttest_quotient_cosets.cpp run this text.
//
// The tables (quot_join_table_entry fills them, one entry per call; canonical residues in [0, r)):
//   JT_W   4 x 256   (W^-1)^(d 2^(8 l)) in the Montgomery domain: W^-x is the product of one entry per byte of x
//   JT_S   4 x 256   the same for s^-1; level 0 is plain (out of the Montgomery domain) and carries 2^-e, so the product of
//                    the levels is the plain factor that ntt_store takes
//   JT_OM  128       (W^n)^-d, the twiddles across the cosets
//   JT_G   256       g_j in the Montgomery domain, from the canonical words of the inverted vanishing table (null: one)
// Values.  A product with one side a table entry (canonical) and the other below 8r is in (-0.07r, 1.07r), as in ntt_tile.h;
// so is a product of two such products (1.07^2 r^2 / 2^261 < 0.01r).
//   in         raw words (< 2^256 < 8r) times 2^522 mod r, times the product of the JT_W entries, times g_j (canonical, last):
//              (-0.07r, 1.07r), the bound ntt_butterfly takes at level 0
//   levels     ntt_butterfly as it is: 1.07r per level, a reduction after level 5; e <= 8 levels leave at most 6.42r (e = 5)
//   out        ntt_store with the product of the JT_S entries as its plain factor: canonical words
constexpr uint32_t kQuotJoinDigitBits = 8, kQuotJoinDigits = 4;
constexpr uint32_t JT_W = 0, JT_S = JT_W + (kQuotJoinDigits << kQuotJoinDigitBits), JT_OM = JT_S + (kQuotJoinDigits << kQuotJoinDigitBits),
                   JT_G = JT_OM + (1u << (SNARKV_QUOT_MAX_E - 1)), JT_END = JT_G + (1u << SNARKV_QUOT_MAX_E);

// the bytes of an exponent below 2^log_n that can be other than zero; one at least, so that the product has a first factor
SNARKV_HD uint32_t quot_join_levels(uint32_t log_n) {
  const uint32_t l = (log_n + kQuotJoinDigitBits - 1) / kQuotJoinDigitBits;
  return l ? l : 1u;
}

// entry `idx` of the tables.  w_inv, s_inv, om_inv: W^-1, s^-1, (W^n)^-1 in the Montgomery domain; inv_words: the 2^e
// canonical scalars g_j, or null
SNARKV_HD Fr29 quot_join_table_entry(uint32_t idx, const Fr29& w_inv, const Fr29& s_inv, const Fr29& om_inv, uint32_t e,
                                     const uint32_t* inv_words) {
  const uint32_t mask = (1u << kQuotJoinDigitBits) - 1u;
  if (idx < JT_S) return ntt_table_entry(w_inv, kQuotJoinDigitBits * ((idx - JT_W) >> kQuotJoinDigitBits), idx & mask, fr29_one());
  if (idx < JT_S + mask + 1u) return ntt_table_entry(s_inv, 0, idx & mask, ntt_n_inverse(e));
  if (idx < JT_OM) return ntt_table_entry(s_inv, kQuotJoinDigitBits * ((idx - JT_S) >> kQuotJoinDigitBits), idx & mask, fr29_one());
  if (idx < JT_G) return ntt_table_entry(om_inv, 0, idx - JT_OM, fr29_one());
  if (!inv_words || ((idx - JT_G) >> e)) return fr29_canon_residue(fr29_one());
  return fr29_canon_residue(fr29_from_canonical(inv_words + 8 * (size_t)(idx - JT_G)));
}

// base^x from the four levels at `tab`: the form of level 0 is the form of the result
SNARKV_HD Fr29 quot_join_power(const Fr29* tab, uint32_t x, uint32_t levels) {
  const uint32_t mask = (1u << kQuotJoinDigitBits) - 1u;
  Fr29 acc = tab[x & mask];
  for (uint32_t l = 1; l < levels; ++l) acc = fr29_mul(acc, tab[(l << kQuotJoinDigitBits) + ((x >> (kQuotJoinDigitBits * l)) & mask)]);
  return acc;
}

SNARKV_HD uint32_t quot_join_bitrev(uint32_t j, uint32_t e) {
  uint32_t r = 0;
  for (uint32_t i = 0; i < e; ++i) r |= ((j >> i) & 1u) << (e - 1u - i);
  return r;
}

// slot = j 2^tile_bits + dt of the tile that starts at t0: where the value of coset j at t = t0 + dt is read ...
SNARKV_HD size_t quot_join_in_index(uint32_t slot, uint32_t t0, uint32_t k, uint32_t tile_bits) {
  return ((size_t)(slot >> tile_bits) << k) + t0 + (slot & ((1u << tile_bits) - 1u));
}
// ... where it goes in the buffer (the cosets bit-reversed, for the levels to end in natural order) ...
SNARKV_HD uint32_t quot_join_in_slot(uint32_t slot, uint32_t e, uint32_t tile_bits) {
  return (quot_join_bitrev(slot >> tile_bits, e) << tile_bits) + (slot & ((1u << tile_bits) - 1u));
}
// ... and its value there: in W^(-j t) g_j.  j t is taken mod 2^32, of which 2^(k+e) is a divisor.
SNARKV_HD Fr29 quot_join_in(const uint32_t w[8], const Fr29* tab, uint32_t slot, uint32_t t0, uint32_t k, uint32_t e,
                            uint32_t tile_bits) {
  const uint32_t j = slot >> tile_bits, t = t0 + (slot & ((1u << tile_bits) - 1u));
  const uint32_t x = (j * t) & (uint32_t)((((uint64_t)1 << (k + e)) - 1u));
  const Fr29 v = fr29_mul(ntt_load(w, ntt_factor_in()), quot_join_power(tab + JT_W, x, quot_join_levels(k + e)));
  return fr29_mul(v, tab[JT_G + j]);
}

// butterfly b < 2^(e - 1 + tile_bits) of level `level` < e, decimation in time over the bit-reversed cosets
SNARKV_HD void quot_join_butterfly(Fr29* buf, const Fr29* tab, uint32_t b, uint32_t level, uint32_t e, uint32_t tile_bits) {
  const uint32_t pair = b >> tile_bits, dt = b & ((1u << tile_bits) - 1u), lo = pair & ((1u << level) - 1u);
  const uint32_t top = ((pair >> level) << (level + 1u)) | lo;
  ntt_butterfly(buf, (top << tile_bits) + dt, 1u << (level + tile_bits), tab[JT_OM + (lo << (e - 1u - level))], level);
}

// slot = q 2^tile_bits + dt after the levels: the index T = t + q n it is written to, and its canonical words
SNARKV_HD size_t quot_join_out_index(uint32_t slot, uint32_t t0, uint32_t k, uint32_t tile_bits) {
  return quot_join_in_index(slot, t0, k, tile_bits);
}
SNARKV_HD void quot_join_out(const Fr29& v, const Fr29* tab, uint32_t T, uint32_t k, uint32_t e, uint32_t w[8]) {
  ntt_store(v, quot_join_power(tab + JT_S, T, quot_join_levels(k + e)), w);
}

// the tile: as many consecutive t as 2^kQuotJoinTileBits slots hold for 2^e cosets, the whole domain if it is smaller
constexpr uint32_t kQuotJoinTileBits = 10;
SNARKV_HD uint32_t quot_join_tile_bits(uint32_t k, uint32_t e) {
  const uint32_t room = kQuotJoinTileBits - e;  // e <= 8
  return k < room ? k : room;
}

}  // namespace snarkv
