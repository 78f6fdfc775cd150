/* snarkv_g1_ntt.h -- the transform of snarkv_ntt.h over group elements: n = 2^k points in device memory in, the n linear
 * combinations of them with the powers of the domain generator out.  What turns the points g of a commitment key into its
 * Lagrange basis (halo2's g_to_lagrange, the g_lagrange of ParamsIPA and ParamsKZG): the points that commit a column held as
 * evaluations over the domain.
 *
 * Two families with the same shapes: snarkv_g1_ntt_* / snarkv_ipa_dk_lagrange_dev (libsnarkv_amd.so, BN254 G1) and
 * snarkv_pallas_g1_ntt_* / snarkv_pallas_ipa_dk_lagrange_dev (libsnarkv_pallas.so).  Conventions of snarkv_amd.h: return 0 or
 * a negative SNARKV_ERR_*.
 *
 * A point is 64 bytes, x || y, little-endian and canonical, as the Pippenger entry points take it, at a 16-byte aligned device
 * address; the identity is 64 zero bytes, accepted on input and written on output.  Points are not validated (the MSM _dev
 * calls do not validate them either): a point off the curve gives bytes without meaning, never an access outside the buffers.
 * Natural order in, natural order out.
 *
 * w and the directions are those of snarkv_ntt.h, without a shift:
 *   SNARKV_NTT_FORWARD   out[i] = sum_j w^(i j) in[j]
 *   SNARKV_NTT_INVERSE   out[i] = n^-1 sum_j w^(-i j) in[j]
 * so that for every scalar vector v   <v, inverse(g)> = <snarkv_ntt_dev(v, SNARKV_NTT_INVERSE), g>:   committing evaluations over
 * inverse(g) is committing the coefficients over g.  The forward transform undoes the inverse one.  k = 0 copies.  d_out64 may
 * be d_in64 (in place) or disjoint from it.
 *
 * The call enqueues its kernels on the context's stream and returns; it does not wait for them.  Work: k passes of n/2
 * butterflies (a + t, a - t with t = w^e b), one scalar multiplication per butterfly except in the first pass, whose
 * twiddles are all 1; the inverse direction multiplies every point by n^-1 in one more pass.  Scratch of the context:
 *   32 (2^(k-1) + 1) bytes of twiddles + 2 * 64 * 2^k bytes of working buffers + 1 152 m bytes for the multiplications of one
 *   launch, m = min(2^k, 2^16) of them (288 m of partial sums, 864 m of window tables: 72 MiB from k = 16 on),
 * 216 MiB at k = 20 and 648 MiB at k = 22.  It grows on the first call of a size, which waits for the stream's earlier work
 * once.
 *
 * snarkv_ipa_dk_lagrange_dev: the inverse transform of the points of a resident key (snarkv_ipa_dk_create), 2^k points to
 * d_out64; the key is only read.
 *
 * Refused before any device work, with nothing written: a null context or key, a null or misaligned address, direction > 1,
 * a key on another device than the context, in and out overlapping in part ("overlap" in snarkv_last_error):
 * SNARKV_ERR_ARG.  k > g1_ntt_max_k(), or a key that is a shard (snarkv_ipa_dk_create_shard: a part of the points has no
 * transform): SNARKV_ERR_LENGTH.
 *
 * g1_ntt_max_k(): 22 (the working buffers are 512 MiB there).                                                                 */
#ifndef SNARKV_G1_NTT_H
#define SNARKV_G1_NTT_H
#include "snarkv_amd.h"
#include "snarkv_ntt.h"

#ifdef __cplusplus
extern "C" {
#endif

int snarkv_g1_ntt_dev(snarkv_ctx* ctx, const void* d_in64, void* d_out64, uint32_t k, uint32_t direction);
int snarkv_ipa_dk_lagrange_dev(snarkv_ctx* ctx, const snarkv_ipa_dk* dk, void* d_out64);
uint32_t snarkv_g1_ntt_max_k(void);

/* the same on pallas (libsnarkv_pallas.so, include/snarkv_pallas.h's context and key) */
int snarkv_pallas_g1_ntt_dev(snarkv_ctx* ctx, const void* d_in64, void* d_out64, uint32_t k, uint32_t direction);
int snarkv_pallas_ipa_dk_lagrange_dev(snarkv_ctx* ctx, const snarkv_ipa_dk* dk, void* d_out64);
uint32_t snarkv_pallas_g1_ntt_max_k(void);

#ifdef __cplusplus
}
#endif
#endif /* SNARKV_G1_NTT_H */
