/* snarkv_poly_prod.h -- products along columns of scalars in device memory: the pointwise product, the product of affine
 * terms, the batch inversion, the grand product (multiplicative prefix scan), and the permutation argument's column Z made of
 * the four.  What a prover needs between its witness columns and the commitments to the argument columns; the columns stay
 * on the device for the one step that is sequential by nature.
 *
 * Two families with the same shapes: snarkv_poly_* (libsnarkv_amd.so, the BN254 scalar field) and snarkv_pallas_poly_*
 * (libsnarkv_pallas.so).  Conventions of snarkv_amd.h: return 0 or a negative SNARKV_ERR_*.
 *
 * A column is n elements as in snarkv_poly.h: 32 bytes each, little-endian, canonical on output (an input >= r is taken mod r
 * as long as it is below 2^256, which the calls do not check), in device memory at a 16-byte aligned address.
 * 1 <= n <= 2^30, not only powers of two.  d_polys32 is n_polys columns of n elements, column-major (poly-major, as in
 * poly_lincomb_dev); the calls name columns by index, and an index may repeat.
 *
 * Every call enqueues its kernels on the context's stream and returns; none waits for them.  (Scratch of the context, a
 * slot of this family's own, grows on the first call of a size, which waits for the stream's earlier work once: 2 KiB plus
 * 32 bytes per 1024 elements, and a little for the levels above.)  Inputs at device addresses are read when the kernels run;
 * the index arrays and betas32 / gammas32 / beta32 / gamma32 are host arrays (scalars: 32 bytes each, little-endian,
 * canonical) and are consumed before the call returns.
 *
 * Zero.  A value is zero iff its residue mod r is: the 32 bytes that spell r itself count as zero.  A zero is inverted to
 * zero, as halo2's batch_invert leaves it, and does not disturb any other element's inverse; in the grand product a zero
 * factor makes every later output and the total zero.
 *
 * poly_mul_dev            out[i] = a[i] * b[i].  out may be exactly a or exactly b.
 * poly_prod_affine_dev    out[i] = prod_{j < count} (polys[idx_a[j]][i] + betas[j] * polys[idx_b[j]][i] + gammas[j]);
 *                         idx_b[j] == SNARKV_POLY_NONE: the term has no beta part (betas[j] is still checked).  One pass per
 *                         16 terms; later passes multiply into out.  out must not overlap a column the call names.
 * poly_batch_invert_dev   out[i] = in[i]^-1, and 0 where in[i] = 0 (mod r).  out may be exactly in.  One field inversion per
 *                         call; nothing of the data's size is kept besides out.
 * poly_grand_product_dev  out[0] = start (1 when d_start32 is NULL), out[i] = out[i-1] * f[i-1] for 0 < i < n, and
 *                         total = out[n-1] * f[n-1] (d_total32 may be NULL; d_out32 may not).  d_start32 and d_total32 are 32
 *                         bytes of device memory.  out may be exactly f.  total may lie neither in out nor in f, start
 *                         neither in out nor in total; start may lie anywhere else, an earlier call's z for instance.
 * poly_perm_product_dev   z[0] = start, z[i+1] = z[i] * prod_j (v_j[i] + beta id_j[i] + gamma)
 *                                                     / prod_j (v_j[i] + beta sigma_j[i] + gamma),  total = z[n]
 *                         with v_j, id_j, sigma_j the columns idx_v[j], idx_id[j], idx_sigma[j], j < count.  The four calls
 *                         above back to back, nothing between them: the numerators into work[0, n) and the denominators
 *                         into work[n, 2n), the second half inverted in place, the first multiplied by it, its grand
 *                         product into z and total -- bit for bit what the separate calls give.  d_work32 holds 2n elements.
 *                         work, z and total are disjoint from each other and from every column named; start lies in none
 *                         of the three.  To chain a later set of columns to an earlier one (halo2's permutation sets), pass
 *                         the earlier call's d_z32 + 32 * (last usable row) as d_start32.  A denominator that is zero
 *                         contributes the factor zero, as the inversion leaves it.
 *
 * Refused before any device work, with nothing enqueued, in this order:
 *   SNARKV_ERR_ARG       a null context; a null or misaligned device address (d_start32 and d_total32 may be null); a null
 *                        host array; an index >= n_polys (when there are columns at all); any overlap not allowed above, a
 *                        partial one included ("overlap" in snarkv_last_error)
 *   SNARKV_ERR_ENCODING  a host scalar >= r
 *   SNARKV_ERR_EMPTY     n = 0, count = 0 or n_polys = 0
 *   SNARKV_ERR_LENGTH    n > 2^30                                                                                         */
#ifndef SNARKV_POLY_PROD_H
#define SNARKV_POLY_PROD_H
#include "snarkv_amd.h"

#define SNARKV_POLY_NONE 0xFFFFFFFFu /* idx_b: the term has no beta part */

#ifdef __cplusplus
extern "C" {
#endif

int snarkv_poly_mul_dev(snarkv_ctx* ctx, const void* d_a32, const void* d_b32, size_t n, void* d_out32);
int snarkv_poly_prod_affine_dev(snarkv_ctx* ctx, const void* d_polys32, size_t n, size_t n_polys, const uint32_t* idx_a,
                                const uint32_t* idx_b, const uint8_t* betas32, const uint8_t* gammas32, size_t count,
                                void* d_out32);
int snarkv_poly_batch_invert_dev(snarkv_ctx* ctx, const void* d_in32, size_t n, void* d_out32);
int snarkv_poly_grand_product_dev(snarkv_ctx* ctx, const void* d_f32, size_t n, const void* d_start32, void* d_out32,
                                  void* d_total32);
int snarkv_poly_perm_product_dev(snarkv_ctx* ctx, const void* d_polys32, size_t n, size_t n_polys, const uint32_t* idx_v,
                                 const uint32_t* idx_id, const uint32_t* idx_sigma, size_t count, const uint8_t* beta32,
                                 const uint8_t* gamma32, const void* d_start32, void* d_work32, void* d_z32, void* d_total32);

/* the same on pallas (libsnarkv_pallas.so, include/snarkv_pallas.h's context) */
int snarkv_pallas_poly_mul_dev(snarkv_ctx* ctx, const void* d_a32, const void* d_b32, size_t n, void* d_out32);
int snarkv_pallas_poly_prod_affine_dev(snarkv_ctx* ctx, const void* d_polys32, size_t n, size_t n_polys, const uint32_t* idx_a,
                                       const uint32_t* idx_b, const uint8_t* betas32, const uint8_t* gammas32, size_t count,
                                       void* d_out32);
int snarkv_pallas_poly_batch_invert_dev(snarkv_ctx* ctx, const void* d_in32, size_t n, void* d_out32);
int snarkv_pallas_poly_grand_product_dev(snarkv_ctx* ctx, const void* d_f32, size_t n, const void* d_start32, void* d_out32,
                                         void* d_total32);
int snarkv_pallas_poly_perm_product_dev(snarkv_ctx* ctx, const void* d_polys32, size_t n, size_t n_polys,
                                        const uint32_t* idx_v, const uint32_t* idx_id, const uint32_t* idx_sigma, size_t count,
                                        const uint8_t* beta32, const uint8_t* gamma32, const void* d_start32, void* d_work32,
                                        void* d_z32, void* d_total32);

#ifdef __cplusplus
}
#endif
#endif /* SNARKV_POLY_PROD_H */
