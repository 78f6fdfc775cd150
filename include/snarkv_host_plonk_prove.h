/* snarkv_host_plonk_prove.h -- a PLONK prover for the callers of snarkv_host.h (libsnarkv_host.so): a protocol and the
 * witness polynomials in device memory in, proof bytes out.  `PlonkProver` of the host mirror (host/plonk_prover.hpp): the
 * mirror image of `PlonkVerifier` (reference verifier/plonk.rs:94-147, verifier/plonk/proof.rs:52-168), driven by the
 * `PlonkProtocol` alone.  It knows no circuit: the protocol fixes the commitments and challenges of every phase, the quotient's
 * numerator, the evaluations and the queries; the caller makes the witness polynomials of each phase from the challenges the
 * earlier phases returned, with the resident-column calls (snarkv_ntt.h, snarkv_poly_prod.h, snarkv_lookup.h).
 *
 * BN254 / KZG.  mos = SNARKV_HOST_MOS_GWC19 or _BDFG21; transcript = SNARKV_HOST_TRANSCRIPT_EVM or _POSEIDON (the host's).
 * Byte layouts and the negative SNARKV_HOST_ERR_* codes are those of snarkv_host.h; snarkv_host_last_error() has the message.
 * The prover draws no randomness: blinding rows and the random polynomial are the caller's columns, and a proof is a function
 * of the arguments.
 *
 * What a protocol must be: no linearization, no instance_committing_key, chunk_degree = 1, no query or evaluation of an
 * instance polynomial, no polynomial index past the quotient's (n_pre + n_inst + n_wit; the quotient itself may be queried at
 * rotation 0, not listed among the evaluations), Lagrange indices within -511 .. 512 and rotations of the numerator within
 * -512 .. 511, a numerator that compiles to the gate program of snarkv_quotient.h (16 registers, 4096 instructions, 1024
 * constants) with an extension e <= 8 (2^e >= its degree) and k + e within the transform's range, num_chunk * 2^k <= 2^(k+e),
 * k >= 1.  Anything else is SNARKV_HOST_ERR_INVALID_PROTOCOL, and the message names the cause.
 *
 * snarkv_host_plonk_prover_plan    needs no device: the numbers of the compiled plan -- the extension e, the columns of the
 *                                  quotient's program (the protocol's polynomials below the quotient, and one each for l_0 and
 *                                  X where the numerator uses them), its instructions and constants -- and the bytes of device
 *                                  memory a session holds (the columns, h, and the work buffer of n_cols * 2^(k+e) elements).
 *                                  Outputs may be null.  Returns 1, or the refusal.
 * snarkv_host_plonk_prover_begin   ctx: a context of libsnarkv_amd.so in the wire form (no SNARKV_FLAG_MONTGOMERY default), on
 *                                  whose stream the inputs are ready.  d_srs64: the n = 2^k points [s^i] G.  d_preprocessed32:
 *                                  the protocol's preprocessed polynomials as coefficients, n each, in its order (null when
 *                                  there are none).  instances: one packed block (`u32 columns, per column u32 m, m x Fr`).
 *                                  Both device inputs are 16-byte aligned; the SRS is read until the session ends, the
 *                                  preprocessed polynomials are copied.  The session allocates its memory, builds the instance
 *                                  polynomials and absorbs the initial state and the instances.  No synchronisation.
 * snarkv_host_plonk_prover_phase   once per phase, in order.  d_witness32: the phase's num_witness polynomials, n elements each,
 *                                  as coefficients (form 0) or as values over the domain (form 1); copied, never written; null
 *                                  for a phase without witnesses.  They are committed in one batch over the SRS and the points
 *                                  written; the phase's challenges are squeezed and returned (32 bytes each) for the caller to
 *                                  build the next phase.  *n_challenges is always set; a `cap` below it is
 *                                  SNARKV_HOST_ERR_CAPACITY before any work.  One synchronisation.  A witness polynomial that is
 *                                  zero commits to the identity, which the transcript refuses as the reference's does:
 *                                  SNARKV_HOST_ERR_TRANSCRIPT, no challenge is written and the session has ended.
 * snarkv_host_plonk_prover_finish  after the last phase: quotient, chunk commitments, z, evaluations, the opening.  Returns 1
 *                                  with the proof (what `PlonkProof::read` reads) in proof_out.  *proof_len is always set; a
 *                                  proof_cap below the proof's length is SNARKV_HOST_ERR_CAPACITY with the needed length in
 *                                  *proof_len, before any work.  A witness that does not satisfy the constraints -- the
 *                                  quotient has coefficients from num_chunk * n on, or numerator(z) != Q(z) (z^n - 1) with the
 *                                  verifier's own evaluation -- returns 0 with "the witness does not satisfy the protocol's
 *                                  constraints" and *proof_len = 0; no proof byte is written.  Three synchronisations with
 *                                  Gwc19, four with Bdfg21.  The verdict on the tail comes before the chunks are written.
 *                                  Without a tail, a chunk of h that is zero commits to the identity:
 *                                  SNARKV_HOST_ERR_TRANSCRIPT.  That is every good witness of a protocol with
 *                                  num_chunk * 2^k = 2^(k+e): h has fewer coefficients than that, so the top chunk is zero and
 *                                  such a protocol never yields a proof; a bad witness of it has no tail to show and is
 *                                  refused by the identity at z alone.  A numerator that names a (polynomial, rotation)
 *                                  which is neither an instance polynomial nor among the protocol's evaluations is found
 *                                  where the verifier finds it, in the identity at z after all the device work:
 *                                  SNARKV_HOST_ERR_INVALID_PROTOCOL, "Missing query".  *proof_len = 0 and no proof byte is
 *                                  written in all of these, and the session has ended.
 * snarkv_host_plonk_prover_destroy frees the session and its device memory (waits for the context's stream); null is ignored.
 *
 * A null argument, an unknown mos / transcript / form, a call out of order (a phase after the last, finish before it, anything
 * but destroy after finish has returned 1 or 0): SNARKV_HOST_ERR_ARG, and the session is as it was.  A failure past the
 * argument checks (a device error, a point at infinity that would have to be written: SNARKV_HOST_ERR_TRANSCRIPT) ends the
 * session: only destroy is accepted.  One session is used by one thread at a time. */
#ifndef SNARKV_HOST_PLONK_PROVE_H
#define SNARKV_HOST_PLONK_PROVE_H
#include "snarkv_host.h"
#include "snarkv_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SNARKV_HOST_PLONK_COEFFS 0 /* a phase's polynomials come as coefficients       */
#define SNARKV_HOST_PLONK_VALUES 1 /* ... as values over the domain, row i at index i  */

typedef struct snarkv_host_plonk_prover snarkv_host_plonk_prover;

int snarkv_host_plonk_prover_plan(const snarkv_host_protocol* protocol, uint32_t* e, size_t* n_cols, size_t* n_instr,
                                  size_t* n_consts, size_t* bytes);
int snarkv_host_plonk_prover_begin(const snarkv_host_protocol* protocol, int mos, int transcript, snarkv_ctx* ctx,
                                   const void* d_srs64, const void* d_preprocessed32, const uint8_t* instances,
                                   size_t instances_len, snarkv_host_plonk_prover** out);
int snarkv_host_plonk_prover_phase(snarkv_host_plonk_prover* p, const void* d_witness32, int form, uint8_t* challenges_out32,
                                   size_t cap, size_t* n_challenges);
int snarkv_host_plonk_prover_finish(snarkv_host_plonk_prover* p, uint8_t* proof_out, size_t proof_cap, size_t* proof_len);
void snarkv_host_plonk_prover_destroy(snarkv_host_plonk_prover* p);

#ifdef __cplusplus
}
#endif
#endif /* SNARKV_HOST_PLONK_PROVE_H */
