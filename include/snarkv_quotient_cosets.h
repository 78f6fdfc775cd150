/* snarkv_quotient_cosets.h -- the quotient polynomial of snarkv_quotient.h computed one coset of the small domain at a time:
 * the same arguments, the same bytes out, a work buffer of n_cols * n elements where quotient_dev takes n_cols * N, and the
 * transform's scratch for columns of n where quotient_dev's is for columns of N.  The calls are declared here and not in
 * snarkv_quotient.h, whose list of names is pinned; everything that header defines (the instruction format, the operand
 * words, the limits, the conventions of an element, a shift and a refusal) holds here.
 *
 * Two families with the same shapes: snarkv_* (libsnarkv_amd.so, the BN254 scalar field) and snarkv_pallas_*
 * (libsnarkv_pallas.so).
 *
 * n = 2^k, N = 2^(k+e), W the generator of the 2^(k+e) domain, w = W^(2^e) that of the 2^k domain, s the coset shift.  Row
 * i = j + 2^e m of the extended coset is the point (s W^j) w^m: the rows i = j mod 2^e are the coset (s W^j) H of the small
 * domain.  The values of a column there come from its n coefficients by one size-k transform with the shift s W^j, without
 * padding; a rotation of rot 2^e rows of the extended coset is rot rows of the coset; X^n - 1 is the constant
 * s^n (W^n)^j - 1 on it.
 *
 * quotient_cosets_dev      h as quotient_dev writes it, bit for bit (both write canonical words): the N coefficients of h(X),
 *                          lowest first, at d_h32.  d_work32 holds n_cols * n elements.  Once per call the program and the
 *                          constants are staged and the 2^e vanishing values are built and inverted on the device; then, for
 *                          j = 0 .. 2^e - 1, the n_cols columns go through the forward transform of size k with the shift
 *                          s W^j into work (the 2^e shifts are computed on the host) and the program runs over work with
 *                          e = 0 into h + j n; then the steps of poly_cosets_join_dev below over h, in place, with the
 *                          inverted vanishing values as one more factor.  If s^n is a 2^e-th root of unity one vanishing
 *                          value is zero and stays zero, that coset counts as zero, and the result is still quotient_dev's.
 *                          work, h and coeffs are pairwise disjoint.
 *                          Launches: 2^e * (transform + program) + a constant -- at e = 8 that is 256 small transforms and
 *                          256 program launches.  The cosets are not batched, because work has one size.  Scratch: the
 *                          quotient's slot as snarkv_quotient.h states it (the join's tables reuse the room of the staged
 *                          program, which the stream has done with by then), and the transform's scratch for
 *                          max(n_cols, 2^e) polynomials of size k.
 *
 * poly_cosets_join_dev     The way back on its own, without the vanishing factor.  d_vals32: the values of a polynomial f of
 *                          degree below N on the 2^e cosets, coset-major: in[j][m] = f((s W^j) w^m).  d_out32: the N
 *                          coefficients of f.  One inverse transform of size k (no shift) over the 2^e rows, in -> out, then
 *                          the join over out in place: with c[j][t] what that transform gives,
 *                            out[t + q n] = s^-(t + q n) 2^-e sum_j W^(-j (t + q n)) c[j][t],
 *                          with s^-1 at shift_inv32.  Bit for bit snarkv_ntt_dev(INVERSE, k + e, shift s^-1) on the values
 *                          interleaved into the order of the extended coset, i = j + 2^e m.  out may be exactly in.  e = 0
 *                          is the inverse transform and the scaling by s^-t.
 *
 * Both calls enqueue their kernels on the context's stream and return; neither waits for them.
 *
 * Refused before any device work, with nothing enqueued: what quotient_dev refuses, in its order and with its codes, the
 * overlap taken with work as n_cols * n elements; for the join a null context, a null or misaligned address, a null or zero
 * shift, a partial overlap of in and out ("overlap" in snarkv_last_error): SNARKV_ERR_ARG; a shift >= r:
 * SNARKV_ERR_ENCODING; e > 8 or k + e > ntt_max_k(): SNARKV_ERR_LENGTH.                                                    */
#ifndef SNARKV_QUOTIENT_COSETS_H
#define SNARKV_QUOTIENT_COSETS_H
#include "snarkv_quotient.h"

#ifdef __cplusplus
extern "C" {
#endif

int snarkv_quotient_cosets_dev(snarkv_ctx* ctx, const void* d_coeffs32, uint32_t k, uint32_t e, size_t n_cols,
                               const snarkv_quot_instr* prog, size_t n_instr, const uint8_t* consts32, size_t n_consts,
                               const uint8_t* shift32, const uint8_t* shift_inv32, void* d_work32, void* d_h32);
int snarkv_poly_cosets_join_dev(snarkv_ctx* ctx, const void* d_vals32, uint32_t k, uint32_t e, const uint8_t* shift_inv32,
                                void* d_out32);

/* the same on pallas (libsnarkv_pallas.so, include/snarkv_pallas.h's context) */
int snarkv_pallas_quotient_cosets_dev(snarkv_ctx* ctx, const void* d_coeffs32, uint32_t k, uint32_t e, size_t n_cols,
                                      const snarkv_quot_instr* prog, size_t n_instr, const uint8_t* consts32, size_t n_consts,
                                      const uint8_t* shift32, const uint8_t* shift_inv32, void* d_work32, void* d_h32);
int snarkv_pallas_poly_cosets_join_dev(snarkv_ctx* ctx, const void* d_vals32, uint32_t k, uint32_t e,
                                       const uint8_t* shift_inv32, void* d_out32);

#ifdef __cplusplus
}
#endif
#endif /* SNARKV_QUOTIENT_COSETS_H */
