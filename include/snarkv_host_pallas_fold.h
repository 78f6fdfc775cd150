/* snarkv_host_pallas_fold.h -- `decide_all` as ONE folded check for the callers of snarkv_host_pallas.h
 * (libsnarkv_host_pallas_fold.so, on top of libsnarkv_host_pallas.so and libsnarkv_pallas.so):
 *     sum_i rho^i U_i  ==  < sum_i rho^i h_coeffs(xi_i) , G >          (include/snarkv_ipa_fold.h)
 * one MSM of 2^k terms and one of m terms whatever m, where snarkv_host_pallas_ipa_decide_all pays m MSMs.
 *
 * The device layer takes rho from its caller, who owns its soundness; these calls ARE that caller: they derive rho from
 * the accumulators, so whoever chose the accumulators could not choose them for a known rho.  A false accept has
 * probability below m / r.
 *
 * Handles, byte layouts (an accumulator = k x xi, 32 B each | u, 64 B), return codes (1 accept / done, 0 reject,
 * SNARKV_HOST_ERR_* otherwise) and ownership are those of snarkv_host_pallas.h.  The existing calls of that header keep
 * their route.  The folded check is one call on the process-global context of libsnarkv_pallas.so, which serialises its
 * calls itself; the succinct half and the per-accumulator fallback are the calls of libsnarkv_host_pallas.so. */
#ifndef SNARKV_HOST_PALLAS_FOLD_H
#define SNARKV_HOST_PALLAS_FOLD_H
#include "snarkv_host_pallas.h"

#ifdef __cplusplus
extern "C" {
#endif

/* thread-local message of the last failing call of this header on this thread */
const char* snarkv_host_pallas_fold_last_error(void);

/* rho = BLAKE2b-512, personalisation "snarkv_ipa_fold1", over  u32le k | u32le m | the m accumulators as the API lays
 * them out (k x xi | u each) | the 32 seed bytes if given; the digest read little-endian and reduced mod r, exactly as
 * the Blake2b transcript squeezes.  seed32_or_null: the verifier's own randomness (optional; it may be public once the
 * accumulators are fixed).  No device work.  Returns 1. */
int snarkv_host_pallas_ipa_fold_challenge(const snarkv_host_pallas_ipa_dk* dk, const uint8_t* accs, uint32_t m,
                                          const uint8_t* seed32_or_null, uint8_t rho_out[32]);
/* derives rho and runs the folded decide: 1 if the batch passes (ok_out, optional: all ones), 0 if not.  On a reject
 * with ok_out given, snarkv_host_pallas_ipa_decide_all runs to fill in the verdict of each accumulator, so naming the
 * culprit costs only on the reject path.  m = 0 accepts.  A non-canonical challenge in an accumulator is
 * SNARKV_HOST_ERR_PANIC, as there. */
int snarkv_host_pallas_ipa_decide_all_folded(const snarkv_host_pallas_ipa_dk* dk, const uint8_t* accs, uint32_t m,
                                             const uint8_t* seed32_or_null, uint8_t* ok_out);
/* snarkv_host_pallas_plonk_verify with the folded decide as its second half: the same arguments plus the seed */
int snarkv_host_pallas_plonk_verify_folded(const snarkv_host_pallas_protocol* protocol, const snarkv_host_pallas_ipa_dk* dk,
                                           const uint8_t* instances, size_t instances_len, const uint8_t* proofs,
                                           size_t proofs_len, uint32_t n, unsigned host_threads, int decompress,
                                           const uint8_t* seed32_or_null);

#ifdef __cplusplus
}
#endif
#endif
