/* snarkv_host_plonk_prove_opts.h -- the PLONK prover session of snarkv_host_plonk_prove.h with options: `plan` and `begin` with
 * a word of flags in front of what they take.  With flags = 0 both are snarkv_host_plonk_prover_plan and _begin, which call
 * them with 0.  The entries are declared here and not in snarkv_host_plonk_prove.h, whose list of names is pinned; the
 * session they return is that header's, for its phase, finish and destroy.
 *
 * SNARKV_HOST_PLONK_QUOTIENT_COSETS   the session takes the quotient one coset of the domain at a time
 *                                     (snarkv_quotient_cosets.h): its work region is n_cols * 2^k elements where the default
 *                                     session's is n_cols * 2^(k+e), and `bytes` of plan_opts is smaller by exactly
 *                                     32 * n_cols * (2^(k+e) - 2^k).  Everything else is the session as it is: the layout in
 *                                     front of the work region, the tail check, the identity at z, the synchronisation
 *                                     counts.  The proof is, byte for byte, the proof of a session without the flag, and
 *                                     every refusal and every 0 verdict comes with the same code and message.  The cost is
 *                                     time: 2^e transforms and program launches of size 2^k where the default makes one of
 *                                     size 2^(k+e) (DESIGN.md 3o has the measurements).
 *
 * A flag bit that is not defined here: SNARKV_HOST_ERR_ARG, "unknown flag bit", after the checks of the arguments that the
 * plain entries make before they look at the protocol or the context. */
#ifndef SNARKV_HOST_PLONK_PROVE_OPTS_H
#define SNARKV_HOST_PLONK_PROVE_OPTS_H
#include "snarkv_host_plonk_prove.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SNARKV_HOST_PLONK_QUOTIENT_COSETS 1u

int snarkv_host_plonk_prover_plan_opts(const snarkv_host_protocol* protocol, uint32_t flags, uint32_t* e, size_t* n_cols,
                                       size_t* n_instr, size_t* n_consts, size_t* bytes);
int snarkv_host_plonk_prover_begin_opts(const snarkv_host_protocol* protocol, int mos, int transcript, uint32_t flags,
                                        snarkv_ctx* ctx, const void* d_srs64, const void* d_preprocessed32,
                                        const uint8_t* instances, size_t instances_len, snarkv_host_plonk_prover** out);

#ifdef __cplusplus
}
#endif
#endif /* SNARKV_HOST_PLONK_PROVE_OPTS_H */
