/* snarkv_ipa_create.h -- `Ipa::create_proof` (reference snark-verifier/src/pcs/ipa.rs:39-124) in one call, with
 * halo2's Blake2b transcript (`Blake2bWrite`, `Challenge255`) on the device: the proof bytes a `Blake2bRead` reads, and
 * the `IpaAccumulator { xi, u }` the reference returns.
 *
 * The session of snarkv_ipa_prover.h leaves the transcript to the caller and costs a read-back, a host transcript step
 * and an upload per round.  Here the rounds, the transcript between them and the folds are enqueued on the context's
 * stream in one go; the call synchronises once, at its end.  The session is unchanged and remains the route for any other
 * transcript (Keccak, Poseidon).
 *
 * Two families with the same shapes: snarkv_ipa_create_proof* (libsnarkv_amd.so, BN254) and
 * snarkv_pallas_ipa_create_proof* (libsnarkv_pallas.so), plus the forms on a library's default context.  Conventions of
 * snarkv_amd.h: scalars 32-byte little-endian canonical, points x || y 64 bytes, return 0 or a negative SNARKV_ERR_*.
 *
 * Arguments
 *   dk            the whole key (a shard is SNARKV_ERR_LENGTH); n must be 2^k, k >= 1 (SNARKV_ERR_LENGTH otherwise)
 *   h64           the key's h
 *   coeffs32      the n coefficients of p (host memory; device memory for _dev)
 *   z32           the opening point
 *   zk            the zero-knowledge branch (ipa.rs:53-69) is taken iff s64 (the key's s), omega32, pbar32 and
 *                 omega_bar32 are ALL given; none of them is the non-zk key; a partial set is SNARKV_ERR_ARG.
 *                 pbar32 = the n scalars the reference draws for p_bar, omega_bar32 the one it draws for omega_bar: the
 *                 caller owns the randomness, as with the blind of the KZG zk call.  The device forms
 *                 p_bar[0] -= p_bar(z) itself.  For _dev, pbar32 is device memory too.
 *   absorbed      the raw bytes the transcript's hasher has taken so far (every prefix byte included), absorbed_len of
 *                 them; may be null when absorbed_len = 0.  The transcript starts from BLAKE2b-512 with the
 *                 personalisation "Halo2-Transcript" over these bytes.
 *   proof_out     proof_cap bytes; *proof_len = 64 k + 64 bytes written, + 64 with zk:
 *                 [c_bar | omega'] k x (L_i | R_i) | U | c    (points compressed to 32 bytes)
 *                 proof_cap too small is SNARKV_ERR_LENGTH with the needed length in *proof_len, before any work.
 *   xi_out32      k x 32 bytes: the challenges xi_1..xi_k of the accumulator
 *   u_out64       its U
 *
 * Under SNARKV_FLAG_VALIDATE z, omega, omega_bar, the coefficients and p_bar are checked before any other work: a
 * non-canonical one is SNARKV_ERR_ENCODING and nothing is written.
 *
 * A point at infinity among L_i, R_i, c_bar and U cannot be written to the transcript (the reference's `write_ec_point`
 * fails): the call returns SNARKV_ERR_ENCODING, snarkv_last_error() says "cannot write points at infinity to the
 * transcript", *proof_len = 0 and the outputs are not written.  The context stays usable.
 *
 * The transcript does not continue after the call -- `Ipa::create_proof` is the last writer in both of the reference's
 * callers -- so no state is exported.                                                                                   */
#ifndef SNARKV_IPA_CREATE_H
#define SNARKV_IPA_CREATE_H
#include "snarkv_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

int snarkv_ipa_create_proof(snarkv_ctx* ctx, const snarkv_ipa_dk* dk, const uint8_t h64[64], const uint8_t* s64_or_null,
                            const uint8_t* coeffs32, size_t n, const uint8_t z32[32], const uint8_t* omega32_or_null,
                            const uint8_t* pbar32_or_null, const uint8_t* omega_bar32_or_null, const uint8_t* absorbed,
                            size_t absorbed_len, uint8_t* proof_out, size_t proof_cap, size_t* proof_len,
                            uint8_t* xi_out32, uint8_t u_out64[64]);
int snarkv_ipa_create_proof_dev(snarkv_ctx* ctx, const snarkv_ipa_dk* dk, const uint8_t h64[64],
                                const uint8_t* s64_or_null, const void* d_coeffs32, size_t n, const uint8_t z32[32],
                                const uint8_t* omega32_or_null, const void* d_pbar32_or_null,
                                const uint8_t* omega_bar32_or_null, const uint8_t* absorbed, size_t absorbed_len,
                                uint8_t* proof_out, size_t proof_cap, size_t* proof_len, uint8_t* xi_out32,
                                uint8_t u_out64[64]);
/* on the library's default context */
int bn254_ipa_create_proof(const snarkv_ipa_dk* dk, const uint8_t h64[64], const uint8_t* s64_or_null,
                           const uint8_t* coeffs32, size_t n, const uint8_t z32[32], const uint8_t* omega32_or_null,
                           const uint8_t* pbar32_or_null, const uint8_t* omega_bar32_or_null, const uint8_t* absorbed,
                           size_t absorbed_len, uint8_t* proof_out, size_t proof_cap, size_t* proof_len,
                           uint8_t* xi_out32, uint8_t u_out64[64]);

/* the same on pallas (libsnarkv_pallas.so, include/snarkv_pallas.h's context and key) */
int snarkv_pallas_ipa_create_proof(snarkv_ctx* ctx, const snarkv_ipa_dk* dk, const uint8_t h64[64],
                                   const uint8_t* s64_or_null, const uint8_t* coeffs32, size_t n, const uint8_t z32[32],
                                   const uint8_t* omega32_or_null, const uint8_t* pbar32_or_null,
                                   const uint8_t* omega_bar32_or_null, const uint8_t* absorbed, size_t absorbed_len,
                                   uint8_t* proof_out, size_t proof_cap, size_t* proof_len, uint8_t* xi_out32,
                                   uint8_t u_out64[64]);
int snarkv_pallas_ipa_create_proof_dev(snarkv_ctx* ctx, const snarkv_ipa_dk* dk, const uint8_t h64[64],
                                       const uint8_t* s64_or_null, const void* d_coeffs32, size_t n,
                                       const uint8_t z32[32], const uint8_t* omega32_or_null,
                                       const void* d_pbar32_or_null, const uint8_t* omega_bar32_or_null,
                                       const uint8_t* absorbed, size_t absorbed_len, uint8_t* proof_out, size_t proof_cap,
                                       size_t* proof_len, uint8_t* xi_out32, uint8_t u_out64[64]);
int pallas_ipa_create_proof(const snarkv_ipa_dk* dk, const uint8_t h64[64], const uint8_t* s64_or_null,
                            const uint8_t* coeffs32, size_t n, const uint8_t z32[32], const uint8_t* omega32_or_null,
                            const uint8_t* pbar32_or_null, const uint8_t* omega_bar32_or_null, const uint8_t* absorbed,
                            size_t absorbed_len, uint8_t* proof_out, size_t proof_cap, size_t* proof_len,
                            uint8_t* xi_out32, uint8_t u_out64[64]);

#ifdef __cplusplus
}
#endif
#endif /* SNARKV_IPA_CREATE_H */
