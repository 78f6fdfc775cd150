/* snarkv_ntt.h -- the number-theoretic transform over the scalar field on polynomials in device memory: coefficients to
 * evaluations over the 2^k domain (or a coset of it) and back.  The change of basis a prover needs before it can feed the
 * resident-polynomial calls (snarkv_poly.h) and the multi-open prover (snarkv_ipa_multiopen.h), which take coefficients,
 * from columns it holds as evaluations.
 *
 * Two families with the same shapes: snarkv_ntt_* (libsnarkv_amd.so, the BN254 scalar field) and snarkv_pallas_ntt_*
 * (libsnarkv_pallas.so).  Conventions of snarkv_amd.h: return 0 or a negative SNARKV_ERR_*.
 *
 * The data is `count` polynomials of n = 2^k elements each, poly-major; an element as in snarkv_poly.h: 32 bytes,
 * little-endian, canonical on output (an input >= r is taken mod r as long as it is below 2^256, which the call does not
 * check), at a 16-byte aligned device address.  Natural order in, natural order out.
 *
 * w = the generator of the 2^k domain that halo2 uses: F::ROOT_OF_UNITY = g^((r - 1) / 2^S) squared S - k times, with g = 7,
 * S = 28 on BN254 and g = 5, S = 32 on pallas.  s = the 32 bytes at shift32 (host memory, little-endian, canonical), or 1
 * when shift32 is NULL.
 *   SNARKV_NTT_FORWARD   out[i] = sum_j (s^j in[j]) w^(i j)          the values of the polynomial on the coset s H
 *   SNARKV_NTT_INVERSE   out[j] = s^j n^-1 sum_i in[i] w^(-i j)
 * The inverse with the shift s^-1 undoes the forward with the shift s; the caller supplies s^-1, the call inverts nothing.
 * k = 0 is the identity.  d_out32 may be d_in32 (in place) or disjoint from it.
 *
 * The call enqueues its kernels on the context's stream and returns; it does not wait for them.  shift32 is consumed before
 * it returns; the data is read when the kernels run.  Scratch of the context: tables of powers of w and of s, 72 * (2^ceil(k/2)
 * + 2^floor(k/2)) bytes + 10 KiB (under 5 MiB at k = 30), and for k > 9 a working buffer of count * 2^k * 32 bytes, the size
 * of the data.  It grows on the first call of a size, which waits for the stream's earlier work once; the tables of w are
 * filled by a kernel on the context's first use of (k, direction) and again when another (k, direction) has been used since.
 *
 * Refused before any device work, with nothing written: a null context, a null or misaligned data address, direction > 1,
 * a shift of zero, data the runtime knows to be on another device than the context, in and out overlapping in part
 * ("overlap" in snarkv_last_error): SNARKV_ERR_ARG.  A shift >= r: SNARKV_ERR_ENCODING.  count = 0: SNARKV_ERR_EMPTY.
 * k > ntt_max_k() or count > 65 535: SNARKV_ERR_LENGTH.
 *
 * ntt_max_k(): the largest k, min(S, 30): 28 on BN254, 30 on pallas.                                                       */
#ifndef SNARKV_NTT_H
#define SNARKV_NTT_H
#include "snarkv_amd.h"

#define SNARKV_NTT_FORWARD 0u /* coefficients -> evaluations */
#define SNARKV_NTT_INVERSE 1u /* evaluations  -> coefficients, 1/n included */

#ifdef __cplusplus
extern "C" {
#endif

int snarkv_ntt_dev(snarkv_ctx* ctx, const void* d_in32, void* d_out32, uint32_t k, size_t count, uint32_t direction,
                   const uint8_t* shift32);
uint32_t snarkv_ntt_max_k(void);

/* the same on pallas (libsnarkv_pallas.so, include/snarkv_pallas.h's context) */
int snarkv_pallas_ntt_dev(snarkv_ctx* ctx, const void* d_in32, void* d_out32, uint32_t k, size_t count, uint32_t direction,
                          const uint8_t* shift32);
uint32_t snarkv_pallas_ntt_max_k(void);

#ifdef __cplusplus
}
#endif
#endif /* SNARKV_NTT_H */
