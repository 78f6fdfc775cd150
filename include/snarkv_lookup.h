/* snarkv_lookup.h -- the lookup argument of a halo2 prover whose columns are in device memory: a sort of scalars, halo2's
 * permute_expression_pair (the permuted input column A' and the permuted table column S'), and the lookup product Z.  The
 * step for which the compressed columns of a lookup otherwise leave the device; it stands between the compression of the
 * lookup's expressions (snarkv_poly.h: poly_lincomb_dev on value columns) and the quotient (snarkv_quotient.h).
 *
 * Two families with the same shapes: snarkv_* (libsnarkv_amd.so, the BN254 scalar field) and snarkv_pallas_*
 * (libsnarkv_pallas.so).  Conventions of snarkv_amd.h and snarkv_poly_prod.h: return 0 or a negative SNARKV_ERR_*; an
 * element is 32 bytes, little-endian, canonical on output (an input >= r is taken mod r as long as it is below 2^256, which
 * the calls do not check), in device memory at a 16-byte aligned address; 1 <= n, u <= 2^30, not only powers of two (the
 * usable rows of a halo2 column are n - (blinding_factors + 1)).
 *
 * Every call enqueues its kernels on the context's stream and returns; none waits for them.  Scratch of the context, a slot
 * of this family's own, grows on the first call of a size, which waits for the stream's earlier work once: 4 KiB, plus
 * 4 bytes per SNARKV_LOOKUP_TILE elements for the sort (the merge partition points), plus for lookup_permute_dev one byte
 * per row (the flags) and 8 bytes per SNARKV_LOOKUP_SCAN_BLOCK rows and a little for the levels above (the scan totals).
 * lookup_product_dev takes what snarkv_poly_prod.h's calls take.  beta32 and gamma32 are host scalars (32 bytes,
 * little-endian, canonical) and are consumed before the call returns.
 *
 * poly_sort_dev        out = in sorted ascending by the canonical integer value of the residue, the Ord of the pasta and
 *                      bn256 scalar fields (numeric, most significant word first); the words of r sort as zero.  A merge
 *                      sort whose cost does not depend on the data.  d_work32 holds n elements.  out may be exactly in;
 *                      work is disjoint from both.  Equal keys are identical after reduction, so there is no order among
 *                      them to keep.
 *
 * lookup_permute_dev   halo2's permute_expression_pair over the first u rows of the compressed input column A
 *                      (d_input32) and table column S (d_table32); u elements are written to each output and the rows
 *                      from u on are not touched (the caller's blinding rows).  perm_input = A' = A sorted.  Row i of A'
 *                      is a first row if i = 0 or A'[i] != A'[i-1], otherwise a repeated row.  perm_table[i] = A'[i] on
 *                      a first row; the table values left over once every distinct input value has taken one copy of
 *                      itself go, in ascending order with multiplicity, to the repeated rows from the LAST repeated row
 *                      down (halo2 pops its list of repeated rows).  d_work32 holds 2u elements.  The two outputs, work,
 *                      A and S are pairwise disjoint, and d_status is disjoint from the outputs and work.
 *                      d_status is 16 bytes of device memory, four uint32:
 *                        status[0]  the number of distinct input values that do not occur in the table; zero means the
 *                                   lookup is satisfiable.  halo2 returns an error otherwise; here every element of both
 *                                   outputs is still written: a first row holds its input value, and the repeated rows
 *                                   take the first leftovers there is room for
 *                        status[1]  the number of distinct input values
 *                        status[2], status[3]  zero
 *                      The call does not synchronise to look at the status; the caller reads it when it next synchronises.
 *
 * lookup_product_dev   z[0] = start, z[i+1] = z[i] (A[i] + beta)(S[i] + gamma) / ((A'[i] + beta)(S'[i] + gamma)),
 *                      total = z[n], with A, S, A', S' the columns idx_input, idx_table, idx_perm_input, idx_perm_table of
 *                      d_polys32 (n_polys columns of n elements, column-major).  poly_perm_product_dev's pattern exactly:
 *                      the numerators into work[0, n) and the denominators into work[n, 2n) (poly_prod_affine_dev with
 *                      two terms without a beta part), the second half inverted in place, the first multiplied by it,
 *                      its grand product into z and total -- bit for bit what the separate calls of snarkv_poly_prod.h
 *                      give.  d_work32 holds 2n elements.  work, z and total are disjoint from each other and from every
 *                      column named; start lies in none of the three.  d_start32 NULL: one; d_total32 may be NULL.
 *
 * Refused before any device work, with nothing enqueued, in this order:
 *   SNARKV_ERR_ARG       a null context; a null or misaligned device address (d_start32 and d_total32 may be null); a null
 *                        host scalar; an index >= n_polys (when there are columns at all); any overlap not allowed above,
 *                        a partial one included ("overlap" in snarkv_last_error)
 *   SNARKV_ERR_ENCODING  beta or gamma >= r
 *   SNARKV_ERR_EMPTY     n, u or n_polys = 0
 *   SNARKV_ERR_LENGTH    n or u > 2^30                                                                                      */
#ifndef SNARKV_LOOKUP_H
#define SNARKV_LOOKUP_H
#include "snarkv_amd.h"

#define SNARKV_LOOKUP_TILE 1024u       /* elements sorted in one workgroup's LDS, and produced by one merge workgroup */
#define SNARKV_LOOKUP_SCAN_BLOCK 1024u /* rows per workgroup of the count scans, at every level */

#ifdef __cplusplus
extern "C" {
#endif

int snarkv_poly_sort_dev(snarkv_ctx* ctx, const void* d_in32, size_t n, void* d_work32, void* d_out32);
int snarkv_lookup_permute_dev(snarkv_ctx* ctx, const void* d_input32, const void* d_table32, size_t u, void* d_work32,
                              void* d_perm_input32, void* d_perm_table32, void* d_status);
int snarkv_lookup_product_dev(snarkv_ctx* ctx, const void* d_polys32, size_t n, size_t n_polys, uint32_t idx_input,
                              uint32_t idx_table, uint32_t idx_perm_input, uint32_t idx_perm_table, const uint8_t* beta32,
                              const uint8_t* gamma32, const void* d_start32, void* d_work32, void* d_z32, void* d_total32);

/* the same on pallas (libsnarkv_pallas.so, include/snarkv_pallas.h's context) */
int snarkv_pallas_poly_sort_dev(snarkv_ctx* ctx, const void* d_in32, size_t n, void* d_work32, void* d_out32);
int snarkv_pallas_lookup_permute_dev(snarkv_ctx* ctx, const void* d_input32, const void* d_table32, size_t u, void* d_work32,
                                     void* d_perm_input32, void* d_perm_table32, void* d_status);
int snarkv_pallas_lookup_product_dev(snarkv_ctx* ctx, const void* d_polys32, size_t n, size_t n_polys, uint32_t idx_input,
                                     uint32_t idx_table, uint32_t idx_perm_input, uint32_t idx_perm_table,
                                     const uint8_t* beta32, const uint8_t* gamma32, const void* d_start32, void* d_work32,
                                     void* d_z32, void* d_total32);

#ifdef __cplusplus
}
#endif
#endif /* SNARKV_LOOKUP_H */
