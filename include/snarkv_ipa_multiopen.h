/* snarkv_ipa_multiopen.h -- the prover of the Bgh19 multi-open scheme of halo2's IPA backend (halo2's `ProverIPA`) in one
 * call: committed polynomials and a list of (polynomial, rotation, evaluation) queries in, the bytes that `Bgh19Proof::read`
 * (reference snark-verifier/src/pcs/ipa/multiopen/bgh19.rs:113-153) consumes out, with the `IpaAccumulator { xi, u }` of the
 * opening it ends in.  The transcript is halo2's Blake2b transcript (`Blake2bWrite`, `Challenge255`).  The steps are those
 * of oracle/ipa.py::bgh19_create_proof, which the tests hold the bytes against.
 *
 * Two families with the same shapes: snarkv_ipa_multiopen_create_proof* (libsnarkv_amd.so, BN254) and
 * snarkv_pallas_ipa_multiopen_create_proof* (libsnarkv_pallas.so), plus the forms on a library's default context.
 * Conventions of snarkv_amd.h: scalars 32-byte little-endian canonical, points x || y 64 bytes, return 0 or a negative
 * SNARKV_ERR_*.
 *
 * Arguments
 *   dk            the whole key (a shard is SNARKV_ERR_LENGTH); n must be 2^k, k >= 1 (SNARKV_ERR_LENGTH otherwise)
 *   h64, s64      the key's h and s.  Both are required: the scheme is always zero-knowledge (a null one is SNARKV_ERR_ARG)
 *   polys32       n_polys x n coefficients, poly-major (host memory; device memory, 16-byte aligned, for _dev).  The
 *                 polynomials never leave the device in either form.
 *   blinds32      n_polys scalars: the blind of each polynomial's commitment <poly, G> + blind s
 *   x32           the evaluation challenge
 *   q_poly, q_shift32, q_eval32    the n_queries queries as three parallel arrays: the point of query i is x * q_shift[i],
 *                 and q_eval[i] must be polys[q_poly[i]] at that point.  Queries are grouped into S sets by the rule of
 *                 bgh19.rs:155-215: per polynomial the distinct shifts in first-seen order; polynomials with equal shift
 *                 sets share a set.  A repeated (polynomial, shift) keeps its first evaluation.
 *   f_blind32, pbar32, omega_bar32   the randomness, which the caller owns, in the order the prover draws it: the blind of
 *                 f, the n scalars of p_bar (device memory for _dev; the call forms p_bar[0] -= p_bar(x_3) on a copy), the
 *                 blind of p_bar's commitment
 *   absorbed      the raw bytes the transcript's hasher has taken so far, as in snarkv_ipa_create.h; may be null when
 *                 absorbed_len = 0
 *   proof_out     proof_cap bytes; *proof_len = 64 k + 32 S + 160 bytes written, points compressed to 32 bytes:
 *                 f | q_eval_1..q_eval_S | s | k x (L_i | R_i) | c | omega' | U
 *                 proof_cap too small is SNARKV_ERR_LENGTH with the needed length in *proof_len, before any device work.
 *   xi_out32      k x 32 bytes: the challenges xi_1..xi_k of the accumulator
 *   u_out64       its U
 *
 * Refusals, all before any output is written:
 *   SNARKV_ERR_ARG       a null argument; a key of another device; q_poly[i] >= n_polys; the points of a set coincide
 *                        (x = 0); and an evaluation that does not match its polynomial: the division of step 3 leaves a
 *                        remainder, which the call notices at its first synchronisation.  snarkv_last_error() then names
 *                        the first offending set ("evaluation does not match the polynomial").  The context stays usable.
 *   SNARKV_ERR_EMPTY     n_polys = 0 or n_queries = 0
 *   SNARKV_ERR_LENGTH    the key, n or proof_cap as above
 *   SNARKV_ERR_ENCODING  under SNARKV_FLAG_VALIDATE a non-canonical scalar among x, the blinds, shifts, evaluations,
 *                        f_blind, omega_bar (checked on the host), the coefficients and p_bar (on the device); and, with
 *                        or without the flag, a point at infinity among f, s, L_i, R_i and U: "cannot write points at
 *                        infinity to the transcript", *proof_len = 0.
 *
 * The call synchronises three times (more under SNARKV_FLAG_VALIDATE, which reads its counts back): after the commitment
 * of f, which the host writes to the transcript to draw x_3; after the S + 1 evaluations at x_3, which it writes to draw
 * x_4; and at the end.  The transcript state goes to the device once, after x_4: s, the two challenges after it, the k
 * rounds and c | omega' | U are hashed there.  The transcript does not continue after the call, so no state is exported. */
#ifndef SNARKV_IPA_MULTIOPEN_H
#define SNARKV_IPA_MULTIOPEN_H
#include "snarkv_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

int snarkv_ipa_multiopen_create_proof(snarkv_ctx* ctx, const snarkv_ipa_dk* dk, const uint8_t h64[64], const uint8_t s64[64],
                                      const uint8_t* polys32, size_t n, size_t n_polys, const uint8_t* blinds32,
                                      const uint8_t x32[32], const uint32_t* q_poly, const uint8_t* q_shift32,
                                      const uint8_t* q_eval32, size_t n_queries, const uint8_t f_blind32[32],
                                      const uint8_t* pbar32, const uint8_t omega_bar32[32], const uint8_t* absorbed,
                                      size_t absorbed_len, uint8_t* proof_out, size_t proof_cap, size_t* proof_len,
                                      uint8_t* xi_out32, uint8_t u_out64[64]);
int snarkv_ipa_multiopen_create_proof_dev(snarkv_ctx* ctx, const snarkv_ipa_dk* dk, const uint8_t h64[64],
                                          const uint8_t s64[64], const void* d_polys32, size_t n, size_t n_polys,
                                          const uint8_t* blinds32, const uint8_t x32[32], const uint32_t* q_poly,
                                          const uint8_t* q_shift32, const uint8_t* q_eval32, size_t n_queries,
                                          const uint8_t f_blind32[32], const void* d_pbar32, const uint8_t omega_bar32[32],
                                          const uint8_t* absorbed, size_t absorbed_len, uint8_t* proof_out, size_t proof_cap,
                                          size_t* proof_len, uint8_t* xi_out32, uint8_t u_out64[64]);
/* on the library's default context */
int bn254_ipa_multiopen_create_proof(const snarkv_ipa_dk* dk, const uint8_t h64[64], const uint8_t s64[64],
                                     const uint8_t* polys32, size_t n, size_t n_polys, const uint8_t* blinds32,
                                     const uint8_t x32[32], const uint32_t* q_poly, const uint8_t* q_shift32,
                                     const uint8_t* q_eval32, size_t n_queries, const uint8_t f_blind32[32],
                                     const uint8_t* pbar32, const uint8_t omega_bar32[32], const uint8_t* absorbed,
                                     size_t absorbed_len, uint8_t* proof_out, size_t proof_cap, size_t* proof_len,
                                     uint8_t* xi_out32, uint8_t u_out64[64]);

/* the same on pallas (libsnarkv_pallas.so, include/snarkv_pallas.h's context and key) */
int snarkv_pallas_ipa_multiopen_create_proof(snarkv_ctx* ctx, const snarkv_ipa_dk* dk, const uint8_t h64[64],
                                             const uint8_t s64[64], const uint8_t* polys32, size_t n, size_t n_polys,
                                             const uint8_t* blinds32, const uint8_t x32[32], const uint32_t* q_poly,
                                             const uint8_t* q_shift32, const uint8_t* q_eval32, size_t n_queries,
                                             const uint8_t f_blind32[32], const uint8_t* pbar32,
                                             const uint8_t omega_bar32[32], const uint8_t* absorbed, size_t absorbed_len,
                                             uint8_t* proof_out, size_t proof_cap, size_t* proof_len, uint8_t* xi_out32,
                                             uint8_t u_out64[64]);
int snarkv_pallas_ipa_multiopen_create_proof_dev(snarkv_ctx* ctx, const snarkv_ipa_dk* dk, const uint8_t h64[64],
                                                 const uint8_t s64[64], const void* d_polys32, size_t n, size_t n_polys,
                                                 const uint8_t* blinds32, const uint8_t x32[32], const uint32_t* q_poly,
                                                 const uint8_t* q_shift32, const uint8_t* q_eval32, size_t n_queries,
                                                 const uint8_t f_blind32[32], const void* d_pbar32,
                                                 const uint8_t omega_bar32[32], const uint8_t* absorbed, size_t absorbed_len,
                                                 uint8_t* proof_out, size_t proof_cap, size_t* proof_len, uint8_t* xi_out32,
                                                 uint8_t u_out64[64]);
int pallas_ipa_multiopen_create_proof(const snarkv_ipa_dk* dk, const uint8_t h64[64], const uint8_t s64[64],
                                      const uint8_t* polys32, size_t n, size_t n_polys, const uint8_t* blinds32,
                                      const uint8_t x32[32], const uint32_t* q_poly, const uint8_t* q_shift32,
                                      const uint8_t* q_eval32, size_t n_queries, const uint8_t f_blind32[32],
                                      const uint8_t* pbar32, const uint8_t omega_bar32[32], const uint8_t* absorbed,
                                      size_t absorbed_len, uint8_t* proof_out, size_t proof_cap, size_t* proof_len,
                                      uint8_t* xi_out32, uint8_t u_out64[64]);

#ifdef __cplusplus
}
#endif
#endif /* SNARKV_IPA_MULTIOPEN_H */
