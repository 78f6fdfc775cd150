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

}  // namespace snarkv
