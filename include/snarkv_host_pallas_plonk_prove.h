/* snarkv_host_pallas_plonk_prove.h -- a PLONK prover on pallas for the callers of snarkv_host_pallas.h
 * (libsnarkv_host_pallas_plonk_prove.so, on top of libsnarkv_host_pallas.so and libsnarkv_pallas.so): a protocol and the
 * witness polynomials in device memory in, the bytes that `PlonkProof::read` with `IpaAs<Bgh19>` consumes out -- halo2's IPA
 * backend: blinded commitments, the Bgh19 multi-open, halo2's Blake2b transcript.  It is the session of
 * snarkv_host_plonk_prove.h (`PlonkProver` of host/plonk_prover.hpp, one session for both commitment schemes) with the IPA
 * scheme in the place of KZG; what that header says about the protocols it takes, the phases and the verdicts holds here and
 * is not repeated.  This header states what the scheme changes.
 *
 * Blinds.  Every commitment is <poly, G> + blind S.  The blinds are the caller's, as all randomness is: a proof is a
 * function of the arguments.  `begin` takes one per preprocessed polynomial -- the blinds their commitments in the protocol
 * were made with (halo2 commits fixed columns with blind 1) --, `phase` one per witness polynomial of the phase, `finish` one
 * per chunk of h.  The session keeps one blind per polynomial below the quotient (0 for the instance polynomials, which are
 * never committed or queried) and forms blind(Q) = sum (z^n)^i blind(h_i) on the host, next to Q = sum (z^n)^i h_i.  Blinds
 * are 32-byte little-endian canonical scalars in host memory; a non-canonical one is SNARKV_HOST_ERR_PANIC.
 *     A zero polynomial with a non-zero blind commits to blind S and is written.  Only a commitment that IS the identity is
 * SNARKV_HOST_ERR_TRANSCRIPT: a zero polynomial with a zero blind, or a polynomial that cancels its blind term.  So a protocol
 * with num_chunk * 2^k = 2^(k+e), whose top chunk of h is zero for every good witness, does yield proofs here when that
 * chunk's blind is not zero; over KZG it never does.
 *
 * Codes and layouts are those of snarkv_host_pallas.h (the SNARKV_HOST_ERR_* of snarkv_host.h; an accumulator = k x xi, 32
 * bytes each | u, 64 bytes); snarkv_host_pallas_plonk_prover_last_error() has the message of the last failing call of this
 * header on the calling thread.
 *
 * snarkv_host_pallas_plonk_prover_plan    needs no device: the numbers of the compiled plan, as snarkv_host_plonk_prover_plan_opts
 *                     gives them (flags: SNARKV_HOST_PLONK_QUOTIENT_COSETS or 0).  `bytes` = 32 ((n_cols' + 1) 2^k + n_cols W +
 *                     2^(k+e)) with n_cols' the columns in front of the quotient's slot (= n_cols) and W = 2^(k+e), or 2^k
 *                     under the flag.  Outputs may be null.  Returns 1, or the refusal: SNARKV_HOST_ERR_INVALID_PROTOCOL with
 *                     the cause named -- a linearization, an instance_committing_key (committed instances), chunk_degree != 1
 *                     and the rest of snarkv_host_plonk_prove.h's list.  No synchronisation.
 * snarkv_host_pallas_plonk_prover_begin   flags: those of snarkv_host_plonk_prove_opts.h.  ctx: a context of libsnarkv_pallas.so
 *                     on whose stream the inputs are ready.  dk: a resident key of libsnarkv_pallas.so
 *                     (snarkv_pallas_ipa_dk_create), the whole key of 2^k points with k the protocol's -- a key of another k
 *                     is SNARKV_HOST_ERR_ARG here; a shard of a 2^k key is refused as SNARKV_HOST_ERR_ARG by the first phase
 *                     that commits.  h64, s64: the key's h and s; both are required, the scheme is always zero-knowledge.
 *                     d_preprocessed32 and pre_blinds32: the preprocessed polynomials as coefficients, 2^k each, in device
 *                     memory (16-byte aligned; copied), and their blinds; both null when the protocol has none.  instances:
 *                     one packed block.  The key is read until the session ends.  No synchronisation.
 * snarkv_host_pallas_plonk_prover_phase   as snarkv_host_plonk_prover_phase, with blinds32: one blind per witness polynomial
 *                     of the phase (null for a phase without witnesses).  The polynomials are committed in one call of
 *                     snarkv_pallas_ipa_commit_blinded_batch_dev into the session's memory.  One synchronisation (none for a
 *                     phase without witnesses; the first commitment on a key also builds its window table, once).
 * snarkv_host_pallas_plonk_prover_finish  chunk_blinds32: one blind per chunk of h.  f_blind32, d_pbar32 (2^k scalars in
 *                     device memory, 16-byte aligned, read and never written), omega_bar32: the randomness of the opening in
 *                     the order the prover draws it (include/snarkv_ipa_multiopen.h).  Returns 1 with the proof in proof_out
 *                     and the accumulator of the opening in acc_out (32 k + 64 bytes, xi then u: what
 *                     snarkv_host_pallas_plonk_succinct_verify_batch computes for the proof, and what
 *                     snarkv_host_pallas_ipa_decide_all takes).  The proof has
 *                         32 (n_wit + num_chunk + |evaluations|) + 64 k + 32 S + 160
 *                     bytes, S the number of query sets of the protocol's queries; *proof_len is always set, and a proof_cap
 *                     below that is SNARKV_HOST_ERR_CAPACITY with the needed length in *proof_len, before any work.  0 with
 *                     "the witness does not satisfy the protocol's constraints" and *proof_len = 0 as over KZG; the opening's
 *                     own "evaluation does not match the polynomial" is the same verdict.  Five synchronisations: the chunks'
 *                     points with the status word, the evaluations, and the three of the opening.
 * snarkv_host_pallas_plonk_prover_destroy frees the session and its device memory (waits for the context's stream); null is
 *                     ignored.
 *
 * A null argument, an unknown form or flag bit, a misaligned device address, a key of another size, a call out of order (a
 * phase after the last, finish before it, anything but destroy after finish has returned 1 or 0): SNARKV_HOST_ERR_ARG, and
 * the session is as it was.  A failure past the argument checks (a device error: SNARKV_HOST_ERR_DEVICE; a point at infinity
 * that would have to be written: SNARKV_HOST_ERR_TRANSCRIPT) ends the session: only destroy is accepted.  One session is
 * used by one thread at a time. */
#ifndef SNARKV_HOST_PALLAS_PLONK_PROVE_H
#define SNARKV_HOST_PALLAS_PLONK_PROVE_H
#include "snarkv_host_pallas.h"
#include "snarkv_pallas.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SNARKV_HOST_PALLAS_PLONK_COEFFS 0          /* a phase's polynomials come as coefficients       */
#define SNARKV_HOST_PALLAS_PLONK_VALUES 1          /* ... as values over the domain, row i at index i  */
#define SNARKV_HOST_PALLAS_PLONK_QUOTIENT_COSETS 1u /* = SNARKV_HOST_PLONK_QUOTIENT_COSETS              */

typedef struct snarkv_host_pallas_plonk_prover snarkv_host_pallas_plonk_prover;

const char* snarkv_host_pallas_plonk_prover_last_error(void);
int snarkv_host_pallas_plonk_prover_plan(const snarkv_host_pallas_protocol* protocol, uint32_t flags, uint32_t* e, size_t* n_cols,
                                         size_t* n_instr, size_t* n_consts, size_t* bytes);
int snarkv_host_pallas_plonk_prover_begin(const snarkv_host_pallas_protocol* protocol, uint32_t flags, snarkv_ctx* ctx,
                                          const snarkv_ipa_dk* dk, const uint8_t h64[64], const uint8_t s64[64],
                                          const void* d_preprocessed32, const uint8_t* pre_blinds32, const uint8_t* instances,
                                          size_t instances_len, snarkv_host_pallas_plonk_prover** out);
int snarkv_host_pallas_plonk_prover_phase(snarkv_host_pallas_plonk_prover* p, const void* d_witness32, int form,
                                          const uint8_t* blinds32, uint8_t* challenges_out32, size_t cap, size_t* n_challenges);
int snarkv_host_pallas_plonk_prover_finish(snarkv_host_pallas_plonk_prover* p, const uint8_t* chunk_blinds32,
                                           const uint8_t f_blind32[32], const void* d_pbar32, const uint8_t omega_bar32[32],
                                           uint8_t* proof_out, size_t proof_cap, size_t* proof_len, uint8_t* acc_out);
void snarkv_host_pallas_plonk_prover_destroy(snarkv_host_pallas_plonk_prover* p);

#ifdef __cplusplus
}
#endif
#endif /* SNARKV_HOST_PALLAS_PLONK_PROVE_H */
