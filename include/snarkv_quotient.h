/* snarkv_quotient.h -- the quotient polynomial h(X) = (sum_i y^i gate_i(X)) / (X^n - 1) of a prover whose columns are in
 * device memory: coefficient columns to their values on the extended coset, a straight-line gate program run at every row,
 * the division by the vanishing polynomial, and the three with the inverse transform in one call.  The step between the
 * commitment to the permutation Z (snarkv_poly_prod.h) and the multi-open proof (snarkv_ipa_multiopen.h).
 *
 * Two families with the same shapes: snarkv_* (libsnarkv_amd.so, the BN254 scalar field) and snarkv_pallas_*
 * (libsnarkv_pallas.so).  Conventions of snarkv_amd.h: return 0 or a negative SNARKV_ERR_*.
 *
 * n = 2^k is the domain, N = 2^(k+e) the extended domain, 0 <= e <= 8, k + e <= ntt_max_k().  W is the generator of the
 * 2^(k+e) domain as snarkv_ntt.h defines it.  s is the coset shift: the 32 bytes at shift32 (host memory, little-endian,
 * canonical, not zero).  A halo2 prover passes its zeta; the calls do not care which shift it is as long as s^n is no
 * 2^e-th root of unity (see poly_div_vanishing_dev).
 *
 * An element is 32 bytes, little-endian, canonical on output (an input >= r is taken mod r as long as it is below 2^256,
 * which the calls do not check), in device memory at a 16-byte aligned address.  Every call enqueues its kernels on the
 * context's stream and returns; none waits for them.  Host arrays (the program, the constants, the shifts) are consumed before
 * the call returns; device data is read when the kernels run.  Scratch of the context: a slot of this family's own (108 KiB:
 * the staged program, the constants, the table of the vanishing polynomial's inverses), and what the transform and the batch
 * inversion take (snarkv_ntt.h, snarkv_poly_prod.h).
 *
 * poly_extend_dev          `count` polynomials of n coefficients in, `count` columns of N values out, both poly-major:
 *                          out[p][i] = f_p(s W^i), halo2's coeff_to_extended.  The coefficients are zero-padded into out and
 *                          transformed there: bit for bit what padding by hand and snarkv_ntt_dev (FORWARD, k + e, shift s)
 *                          give.  out is disjoint from coeffs.
 *
 * quotient_eval_dev        A straight-line program run at every one of the N rows.  Each row has a private file of
 *                          SNARKV_QUOT_REGS registers.  An instruction (snarkv_quot_instr, 16 bytes) is
 *                            SNARKV_QUOT_ADD  dst = a + b        SNARKV_QUOT_MUL  dst = a * b
 *                            SNARKV_QUOT_SUB  dst = a - b        SNARKV_QUOT_FMA  dst = a * b + c
 *                          with `zero` = 0, and c = 0 on the three two-operand ops.  An operand word names, by its bits 31:30,
 *                            SNARKV_QUOT_REG(i)         kind 0: register i, which an earlier instruction has written
 *                            SNARKV_QUOT_CONST(i)       kind 1: consts32[i], a host array of n_consts canonical scalars: the
 *                                                       challenges, y, and the circuit's constants
 *                            SNARKV_QUOT_COL(col, rot)  kind 2: column `col` (bits 19:0) at row (i + rot * 2^e) mod N, rot in
 *                                                       bits 29:20 as a 10-bit two's complement number, -512 .. 511.  The
 *                                                       row is the euclidean remainder, so it wraps any number of times:
 *                                                       halo2's get_rotation_idx with rot_scale = 2^e.
 *                          d_cols32 is n_cols columns of N values, poly-major.  out[i] is the destination register of the last
 *                          instruction at row i.  dst may be a register the instruction reads.  There is no operand for X: a
 *                          caller that needs X on the coset (the permutation argument's delta^j X) passes the polynomial
 *                          (0, 1, 0, ...) through poly_extend_dev as one more column.  out overlaps cols in no part.
 *                          n_instr <= SNARKV_QUOT_MAX_INSTR, n_consts <= SNARKV_QUOT_MAX_CONSTS (consts32 may be NULL when
 *                          n_consts is 0), 1 <= n_cols <= SNARKV_QUOT_MAX_COLS.
 *
 * poly_div_vanishing_dev   out[i] = in[i] / ((s W^i)^n - 1) over N values; out may be exactly in.  The divisor takes only 2^e
 *                          values, s^n (W^n)^i - 1: the table is built and inverted on the device (one field inversion per
 *                          call, no host round trip) and one pointwise pass reads it at i mod 2^e.  Precondition: s^n is no
 *                          2^e-th root of unity.  If it is, one table entry is zero and stays zero as the batch inversion
 *                          leaves it, and every row that reads it comes out zero; the call does not synchronise to detect it.
 *
 * quotient_dev             The three calls above and the inverse transform, back to back with nothing between them: the n_cols
 *                          coefficient columns at d_coeffs32 (n each) are extended into work (n_cols * N elements), the
 *                          program is evaluated over work into h, h is divided in place and brought back by the inverse
 *                          transform of size k + e with the shift s^-1, in place: the N coefficients of h(X), lowest first.
 *                          The 2^e pieces of n coefficients that halo2 commits to are its consecutive slices.  As in
 *                          snarkv_ntt.h the caller supplies s^-1 (shift_inv32) and the call inverts nothing.  Bit for bit what
 *                          the separate calls give.  work, h and coeffs are pairwise disjoint.
 *
 * Refused before any device work, with nothing enqueued, in this order:
 *   SNARKV_ERR_ARG       a null context; a null or misaligned device address; a null host array; a shift of zero; a program
 *                        fault (an unknown op, `zero` != 0, c != 0 on a two-operand op, an operand of kind 3, a register
 *                        >= SNARKV_QUOT_REGS or read before any earlier instruction wrote it, a constant index >= n_consts, a
 *                        column index >= n_cols when there are columns at all; snarkv_last_error names the instruction); any
 *                        overlap not allowed above, a partial one included ("overlap" in snarkv_last_error)
 *   SNARKV_ERR_ENCODING  a constant or a shift >= r
 *   SNARKV_ERR_EMPTY     count, n_cols or n_instr = 0
 *   SNARKV_ERR_LENGTH    e > 8, k + e > ntt_max_k(), n_instr > 4096, n_consts > 1024, n_cols > 2^20, count > 65 535          */
#ifndef SNARKV_QUOTIENT_H
#define SNARKV_QUOTIENT_H
#include "snarkv_amd.h"

#define SNARKV_QUOT_REGS 16u
#define SNARKV_QUOT_MAX_INSTR 4096u
#define SNARKV_QUOT_MAX_CONSTS 1024u
#define SNARKV_QUOT_MAX_COLS (1u << 20)
#define SNARKV_QUOT_MAX_E 8u

#define SNARKV_QUOT_ADD 0u /* dst = a + b     */
#define SNARKV_QUOT_SUB 1u /* dst = a - b     */
#define SNARKV_QUOT_MUL 2u /* dst = a * b     */
#define SNARKV_QUOT_FMA 3u /* dst = a * b + c */

/* operand words */
#define SNARKV_QUOT_REG(i) ((uint32_t)(i))
#define SNARKV_QUOT_CONST(i) ((1u << 30) | (uint32_t)(i))
#define SNARKV_QUOT_COL(col, rot) ((2u << 30) | (((uint32_t)(rot) & 0x3FFu) << 20) | ((uint32_t)(col) & 0xFFFFFu))

typedef struct {
  uint8_t op, dst;
  uint16_t zero;
  uint32_t a, b, c;
} snarkv_quot_instr;

#ifdef __cplusplus
extern "C" {
#endif

int snarkv_poly_extend_dev(snarkv_ctx* ctx, const void* d_coeffs32, uint32_t k, uint32_t e, size_t count, const uint8_t* shift32,
                           void* d_out32);
int snarkv_quotient_eval_dev(snarkv_ctx* ctx, const void* d_cols32, uint32_t k, uint32_t e, size_t n_cols,
                             const snarkv_quot_instr* prog, size_t n_instr, const uint8_t* consts32, size_t n_consts,
                             void* d_out32);
int snarkv_poly_div_vanishing_dev(snarkv_ctx* ctx, const void* d_in32, uint32_t k, uint32_t e, const uint8_t* shift32,
                                  void* d_out32);
int snarkv_quotient_dev(snarkv_ctx* ctx, const void* d_coeffs32, uint32_t k, uint32_t e, size_t n_cols,
                        const snarkv_quot_instr* prog, size_t n_instr, const uint8_t* consts32, size_t n_consts,
                        const uint8_t* shift32, const uint8_t* shift_inv32, void* d_work32, void* d_h32);

/* the same on pallas (libsnarkv_pallas.so, include/snarkv_pallas.h's context) */
int snarkv_pallas_poly_extend_dev(snarkv_ctx* ctx, const void* d_coeffs32, uint32_t k, uint32_t e, size_t count,
                                  const uint8_t* shift32, void* d_out32);
int snarkv_pallas_quotient_eval_dev(snarkv_ctx* ctx, const void* d_cols32, uint32_t k, uint32_t e, size_t n_cols,
                                    const snarkv_quot_instr* prog, size_t n_instr, const uint8_t* consts32, size_t n_consts,
                                    void* d_out32);
int snarkv_pallas_poly_div_vanishing_dev(snarkv_ctx* ctx, const void* d_in32, uint32_t k, uint32_t e, const uint8_t* shift32,
                                         void* d_out32);
int snarkv_pallas_quotient_dev(snarkv_ctx* ctx, const void* d_coeffs32, uint32_t k, uint32_t e, size_t n_cols,
                               const snarkv_quot_instr* prog, size_t n_instr, const uint8_t* consts32, size_t n_consts,
                               const uint8_t* shift32, const uint8_t* shift_inv32, void* d_work32, void* d_h32);

#ifdef __cplusplus
}
#endif
#endif /* SNARKV_QUOTIENT_H */
