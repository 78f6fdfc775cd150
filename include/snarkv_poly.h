/* snarkv_poly.h -- polynomials over the scalar field in device memory: a linear combination of many, the evaluation at a
 * point and the division by a linear factor.  The pieces the IPA multi-open prover (snarkv_ipa_multiopen.h) is made of,
 * exported because they are useful alone.
 *
 * Two families with the same shapes: snarkv_poly_* (libsnarkv_amd.so, the BN254 scalar field) and snarkv_pallas_poly_*
 * (libsnarkv_pallas.so).  Conventions of snarkv_amd.h: return 0 or a negative SNARKV_ERR_*.
 *
 * A polynomial is n coefficients, lowest first, 32 bytes each, little-endian and canonical (< r; a value >= r is taken mod r
 * as long as it is below 2^256, which the calls do not check), in device memory at a 16-byte aligned address.
 * 1 <= n <= 2^30, not only powers of two; n = 0 is SNARKV_ERR_EMPTY, more SNARKV_ERR_LENGTH, a null or misaligned address
 * SNARKV_ERR_ARG.
 *
 * Every call enqueues its kernels on the context's stream and returns; none waits for them.  (Scratch of the context grows
 * on the first call of a size, which waits for the stream's earlier work once.)  Inputs at device addresses are read when
 * the kernels run; the host arrays of poly_lincomb_dev are consumed before the call returns.
 *
 * poly_lincomb_dev     out = sum_{j < count} scalars[j] * polys[idx[j]]
 *                      d_polys32: n_polys polynomials of n coefficients each, poly-major.  idx and scalars32 (count x 32
 *                      bytes) are host arrays; an index may repeat.  idx[j] >= n_polys is SNARKV_ERR_ARG before any
 *                      launch, count = 0 SNARKV_ERR_EMPTY.  One pass per 32 terms: each coefficient of out is written once
 *                      per pass.  out must not overlap a polynomial it reads: SNARKV_ERR_ARG.
 * poly_eval_dev        out = p(point); the point is 32 bytes in device memory, and so is out.
 * poly_div_linear_dev  p = (X - root) * quot + rem: quot has n - 1 coefficients, rem is 32 bytes, the root is 32 bytes in
 *                      device memory.  rem = p(root).  n = 1 gives an empty quotient (d_quot32 may be null) and rem = p_0.
 *                      quot must NOT overlap coeffs, nor rem either of them: the quotient's coefficient i - 1 is written
 *                      by the workgroup that reads coefficient i, a neighbour of the one that reads i - 1.  An overlap is
 *                      SNARKV_ERR_ARG and nothing is enqueued.                                                            */
#ifndef SNARKV_POLY_H
#define SNARKV_POLY_H
#include "snarkv_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

int snarkv_poly_lincomb_dev(snarkv_ctx* ctx, const void* d_polys32, size_t n, size_t n_polys, const uint32_t* idx,
                            const uint8_t* scalars32, size_t count, void* d_out32);
int snarkv_poly_eval_dev(snarkv_ctx* ctx, const void* d_coeffs32, size_t n, const void* d_point32, void* d_out32);
int snarkv_poly_div_linear_dev(snarkv_ctx* ctx, const void* d_coeffs32, size_t n, const void* d_root32, void* d_quot32,
                               void* d_rem32);

/* the same on pallas (libsnarkv_pallas.so, include/snarkv_pallas.h's context) */
int snarkv_pallas_poly_lincomb_dev(snarkv_ctx* ctx, const void* d_polys32, size_t n, size_t n_polys, const uint32_t* idx,
                                   const uint8_t* scalars32, size_t count, void* d_out32);
int snarkv_pallas_poly_eval_dev(snarkv_ctx* ctx, const void* d_coeffs32, size_t n, const void* d_point32, void* d_out32);
int snarkv_pallas_poly_div_linear_dev(snarkv_ctx* ctx, const void* d_coeffs32, size_t n, const void* d_root32,
                                      void* d_quot32, void* d_rem32);

#ifdef __cplusplus
}
#endif
#endif /* SNARKV_POLY_H */
