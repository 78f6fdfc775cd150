/* snarkv_poly_batch.h -- many evaluations of resident polynomials in one call: the stage of a prover that evaluates every
 * committed polynomial at x and at a few rotations of x, and what turns resident polynomials into the evaluations the
 * multi-open provers take (snarkv_kzg_multiopen.h, snarkv_ipa_multiopen.h).
 *
 * Two families with the same shape: snarkv_poly_eval_many_dev (libsnarkv_amd.so, the BN254 scalar field) and
 * snarkv_pallas_poly_eval_many_dev (libsnarkv_pallas.so).  Conventions of snarkv_poly.h: a polynomial is n coefficients,
 * lowest first, 32 bytes each, little-endian and canonical, in device memory at a 16-byte aligned address; return 0 or a
 * negative SNARKV_ERR_*.
 *
 * poly_eval_many_dev   out[i] = polys[q_poly[i]](points[q_point[i]]),  i < count
 *   d_polys32    n_polys polynomials of n coefficients each, poly-major, 1 <= n <= 2^30 (not only powers of two)
 *   d_points32   n_points scalars of 32 bytes, device memory
 *   q_poly, q_point   host arrays of `count` indices, consumed before the call returns; an index may repeat
 *   d_out32      count results of 32 bytes, canonical, device memory; must not overlap the polynomials or the points
 *
 * The call enqueues on the context's stream and returns; it does not wait.  (Scratch of the context grows on the first call
 * of a size, which waits for the stream's earlier work once.)  The number of kernel launches depends on n alone -- one per
 * level of the blocked scan of snarkv_poly.h, 256 coefficients per workgroup: one up to 256 coefficients, two up to 2^16,
 * three up to 2^24, four beyond -- and not on count: the queries are the second dimension of every launch.  A count above
 * 65 535 (the grid's limit), or one whose block totals would need more than 256 MiB of scratch, runs in chunks of that many
 * queries.  The result of a query is the bytes snarkv_poly_eval_dev writes for the same polynomial and point.
 *
 * Refusals, all before any launch:
 *   SNARKV_ERR_ARG      a null context or index array; a null or misaligned device address; q_poly[i] >= n_polys or
 *                       q_point[i] >= n_points; out overlapping the polynomials or the points
 *   SNARKV_ERR_EMPTY    n = 0, count = 0, n_polys = 0 or n_points = 0
 *   SNARKV_ERR_LENGTH   n > 2^30                                                                                           */
#ifndef SNARKV_POLY_BATCH_H
#define SNARKV_POLY_BATCH_H
#include "snarkv_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

int snarkv_poly_eval_many_dev(snarkv_ctx* ctx, const void* d_polys32, size_t n, size_t n_polys, const void* d_points32,
                              size_t n_points, const uint32_t* q_poly, const uint32_t* q_point, size_t count, void* d_out32);

/* the same on pallas (libsnarkv_pallas.so, include/snarkv_pallas.h's context) */
int snarkv_pallas_poly_eval_many_dev(snarkv_ctx* ctx, const void* d_polys32, size_t n, size_t n_polys,
                                     const void* d_points32, size_t n_points, const uint32_t* q_poly,
                                     const uint32_t* q_point, size_t count, void* d_out32);

#ifdef __cplusplus
}
#endif
#endif /* SNARKV_POLY_BATCH_H */
