/* snarkv_ipa_prover.h -- the IPA prover on the device: the rounds of `Ipa::create_proof`
 * (reference snark-verifier/src/pcs/ipa.rs:39-124) and the h-combination of
 * `IpaAs::create_proof` (pcs/ipa/accumulation.rs:149-226).
 *
 * Two families with the same shapes: snarkv_ipa_prover_* (libsnarkv_amd.so, BN254, on the
 * snarkv_amd.h context and deciding key) and snarkv_pallas_ipa_prover_* (libsnarkv_pallas.so, on
 * the snarkv_pallas.h context and key).  Same conventions as snarkv_amd.h: scalars 32-byte
 * little-endian canonical, points x || y 64 bytes little-endian canonical, identity = 64 zero
 * bytes, return 0 or a negative SNARKV_ERR_*.  The prover speaks the wire form whatever the
 * context's default flags say; SNARKV_FLAG_VALIDATE among them makes a non-canonical scalar
 * SNARKV_ERR_ENCODING.
 *
 * The session does not touch the transcript: the caller writes L, R, U and c and squeezes xi, as a
 * Rust `TranscriptWrite` would.  Call order, with k = log2 of the key size:
 *     begin; k x (round, fold); finish; destroy
 * Any other order is SNARKV_ERR_ARG (fold before round, a (k+1)-th round, finish before the k-th
 * fold).  Two refusals change nothing and leave the session usable: SNARKV_ERR_ARG for a call out
 * of order or with a null argument, and SNARKV_ERR_ENCODING for a non-canonical xi under
 * SNARKV_FLAG_VALIDATE (checked before any work).  Any other failure leaves the session failed: it
 * then accepts only destroy.
 *
 * The session owns its buffers (n coefficients, n powers of z, the n/2 folded bases and the
 * staging of the base fold), allocated at begin and freed at destroy; context scratch is used
 * only inside a call, so other calls on the same context may run between rounds.  The deciding
 * key is read until the first fold, which waits for its kernels: the key may be destroyed once
 * the first fold has returned.
 *
 * fold takes xi as the caller squeezed it and folds the coefficients with xi^-1, computed on the
 * device as xi^(r-2): xi = 0 (which the reference's `invert().unwrap()` rejects) folds with 0.     */
#ifndef SNARKV_IPA_PROVER_H
#define SNARKV_IPA_PROVER_H
#include "snarkv_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct snarkv_ipa_prover snarkv_ipa_prover;

/* `IpaProvingKey::commit` (ipa.rs:221-229) with the resident key: sum_{j<n} poly[j] G[j], plus
 * omega * s when both omega32 and s64 are given.  1 <= n <= 2^k (the first n bases).  Synchronous. */
int snarkv_ipa_commit(snarkv_ctx* ctx, const snarkv_ipa_dk* dk, const uint8_t* poly32, size_t n,
                      const uint8_t* omega32_or_null, const uint8_t* s64_or_null, uint8_t out64[64]);
/* coeffs = p' (n = 2^k canonical scalars; host memory, or device memory for _dev), z the opening
 * point, h the key's h; h' = xi_0 * h is formed on the device.  n != 2^k is SNARKV_ERR_LENGTH. */
int snarkv_ipa_prover_begin(snarkv_ctx* ctx, const snarkv_ipa_dk* dk, const uint8_t* coeffs32, size_t n,
                            const uint8_t z32[32], const uint8_t h64[64], const uint8_t xi0_32[32],
                            snarkv_ipa_prover** out);
int snarkv_ipa_prover_begin_dev(snarkv_ctx* ctx, const snarkv_ipa_dk* dk, const void* d_coeffs32, size_t n,
                                const uint8_t z32[32], const uint8_t h64[64], const uint8_t xi0_32[32],
                                snarkv_ipa_prover** out);
/* L_i and R_i of the current round (ipa.rs:80-101).  Synchronous. */
int snarkv_ipa_prover_round(snarkv_ipa_prover* p, uint8_t l64[64], uint8_t r64[64]);
/* fold bases, coefficients and powers by xi_i (ipa.rs:103-118).  Enqueued (the first fold waits). */
int snarkv_ipa_prover_fold(snarkv_ipa_prover* p, const uint8_t xi32[32]);
/* U = the last base, c = the last coefficient (ipa.rs:121-122).  Synchronous. */
int snarkv_ipa_prover_finish(snarkv_ipa_prover* p, uint8_t u64[64], uint8_t c32[32]);
void snarkv_ipa_prover_destroy(snarkv_ipa_prover* p);
/* h[j] = sum_{i<m} alpha^i h_coeffs(xi_i)[j] (+ alpha^m (b, a, 0, ...) when ab64 = a || b is given):
 * accumulation.rs:186-207.  xi32 = m x k scalars (host), d_h32 = 2^k scalars out (device memory,
 * 16-byte aligned: SNARKV_ERR_ARG otherwise).
 * Synchronous: h is written when the call returns.                                                */
int snarkv_ipa_as_combine_dev(snarkv_ctx* ctx, const uint8_t* xi32, size_t m, uint32_t k, const uint8_t alpha32[32],
                              const uint8_t* ab64_or_null, void* d_h32);

/* the same on pallas (libsnarkv_pallas.so, include/snarkv_pallas.h's context and key) */
int snarkv_pallas_ipa_commit(snarkv_ctx* ctx, const snarkv_ipa_dk* dk, const uint8_t* poly32, size_t n,
                             const uint8_t* omega32_or_null, const uint8_t* s64_or_null, uint8_t out64[64]);
int snarkv_pallas_ipa_prover_begin(snarkv_ctx* ctx, const snarkv_ipa_dk* dk, const uint8_t* coeffs32, size_t n,
                                   const uint8_t z32[32], const uint8_t h64[64], const uint8_t xi0_32[32],
                                   snarkv_ipa_prover** out);
int snarkv_pallas_ipa_prover_begin_dev(snarkv_ctx* ctx, const snarkv_ipa_dk* dk, const void* d_coeffs32, size_t n,
                                       const uint8_t z32[32], const uint8_t h64[64], const uint8_t xi0_32[32],
                                       snarkv_ipa_prover** out);
int snarkv_pallas_ipa_prover_round(snarkv_ipa_prover* p, uint8_t l64[64], uint8_t r64[64]);
int snarkv_pallas_ipa_prover_fold(snarkv_ipa_prover* p, const uint8_t xi32[32]);
int snarkv_pallas_ipa_prover_finish(snarkv_ipa_prover* p, uint8_t u64[64], uint8_t c32[32]);
void snarkv_pallas_ipa_prover_destroy(snarkv_ipa_prover* p);
int snarkv_pallas_ipa_as_combine_dev(snarkv_ctx* ctx, const uint8_t* xi32, size_t m, uint32_t k,
                                     const uint8_t alpha32[32], const uint8_t* ab64_or_null, void* d_h32);

#ifdef __cplusplus
}
#endif
#endif /* SNARKV_IPA_PROVER_H */
