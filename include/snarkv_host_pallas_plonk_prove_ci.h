/* snarkv_host_pallas_plonk_prove_ci.h -- the PLONK prover session of snarkv_host_pallas_plonk_prove.h for protocols with
 * COMMITTED INSTANCES, the shape of every halo2 proof over IPA (Config::ipa(): query_instance = true): the instance columns
 * are committed, hashed into the transcript as points, and their polynomials are queried at z like any witness polynomial.
 * libsnarkv_host_pallas_plonk_prove_ci.so, next to libsnarkv_host_pallas_plonk_prove.so.
 *
 * The six calls have the signatures, the conventions, the flags, the forms and the return codes of that header's; read it for
 * them.  What differs, when the protocol carries an instance_committing_key {bases, constant}:
 *   plan / begin   accept the key, and accept queries and evaluations of instance polynomials (without a key both stay
 *                  refused: the verifier computes those values itself).  Refused as SNARKV_HOST_ERR_INVALID_PROTOCOL, by name:
 *                  a `constant` that is not the key's s (begin), and a num_instance entry above the number of bases (plan and
 *                  begin: the verifier would silently truncate that column).
 *   begin          builds the instance polynomials as before, then commits the n_inst of them with ONE
 *                  snarkv_pallas_ipa_commit_blinded_batch_dev -- blind 1 when `constant` is present, 0 when it is absent --
 *                  downloads the points (one synchronisation; begin has none otherwise) and absorbs them with
 *                  common_ec_point where it otherwise absorbs the instance scalars.  The points are not proof bytes.  An
 *                  identity among them (no constant and an all-zero column) is SNARKV_HOST_ERR_TRANSCRIPT.
 *   finish         the instance polynomials go through the one batched evaluation and the opening with their blinds.
 * The verifier recomputes every instance commitment as sum_i instance[i] * bases[i] + constant.  That equals the session's
 * <coefficients, g> + s exactly when bases are the first points of the key's LAGRANGE basis (snarkv_pallas_ipa_dk_lagrange_dev,
 * snarkv_g1_ntt.h).  The bases are NOT checked: over other bases the session writes a proof that the verifier rejects.
 *
 * A protocol without an instance_committing_key behaves, byte for byte, as under snarkv_host_pallas_plonk_prover_*.  The
 * handles of the two libraries are different types and are not interchangeable. */
#ifndef SNARKV_HOST_PALLAS_PLONK_PROVE_CI_H
#define SNARKV_HOST_PALLAS_PLONK_PROVE_CI_H
#include "snarkv_host_pallas_plonk_prove.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct snarkv_host_pallas_plonk_ci_prover snarkv_host_pallas_plonk_ci_prover;

const char* snarkv_host_pallas_plonk_ci_prover_last_error(void);
int snarkv_host_pallas_plonk_ci_prover_plan(const snarkv_host_pallas_protocol* protocol, uint32_t flags, uint32_t* e, size_t* n_cols,
                                            size_t* n_instr, size_t* n_consts, size_t* bytes);
int snarkv_host_pallas_plonk_ci_prover_begin(const snarkv_host_pallas_protocol* protocol, uint32_t flags, snarkv_ctx* ctx,
                                             const snarkv_ipa_dk* dk, const uint8_t h64[64], const uint8_t s64[64],
                                             const void* d_preprocessed32, const uint8_t* pre_blinds32, const uint8_t* instances,
                                             size_t instances_len, snarkv_host_pallas_plonk_ci_prover** out);
int snarkv_host_pallas_plonk_ci_prover_phase(snarkv_host_pallas_plonk_ci_prover* p, const void* d_witness32, int form,
                                             const uint8_t* blinds32, uint8_t* challenges_out32, size_t cap, size_t* n_challenges);
int snarkv_host_pallas_plonk_ci_prover_finish(snarkv_host_pallas_plonk_ci_prover* p, const uint8_t* chunk_blinds32,
                                              const uint8_t f_blind32[32], const void* d_pbar32, const uint8_t omega_bar32[32],
                                              uint8_t* proof_out, size_t proof_cap, size_t* proof_len, uint8_t* acc_out);
void snarkv_host_pallas_plonk_ci_prover_destroy(snarkv_host_pallas_plonk_ci_prover* p);

#ifdef __cplusplus
}
#endif
#endif /* SNARKV_HOST_PALLAS_PLONK_PROVE_CI_H */
