/* snarkv_host_pallas_prove.h -- `Ipa::create_proof` (reference snark-verifier/src/pcs/ipa.rs:39-124) in one call for the
 * callers of snarkv_host_pallas.h (libsnarkv_host_pallas_prove.so, on top of libsnarkv_host_pallas.so and
 * libsnarkv_pallas.so): halo2's Blake2b transcript stays on the device between the rounds (include/snarkv_ipa_create.h),
 * so a proof is one enqueue and one synchronisation.
 *
 * Handles, byte layouts (an accumulator = k x xi, 32 B each | u, 64 B), ownership and the negative SNARKV_HOST_ERR_*
 * codes are those of snarkv_host_pallas.h; a call of this header returns 1 when the proof is written.  The existing calls
 * of that header keep their route.  The proof is one call on the process-global context of libsnarkv_pallas.so, which
 * serialises its calls itself. */
#ifndef SNARKV_HOST_PALLAS_PROVE_H
#define SNARKV_HOST_PALLAS_PROVE_H
#include "snarkv_host_pallas.h"

#ifdef __cplusplus
extern "C" {
#endif

/* thread-local message of the last failing call of this header on this thread */
const char* snarkv_host_pallas_prove_last_error(void);

/* Opens poly (n = 2^k canonical scalars, 32 B each) at z32 with the key's g, h (and s: a zero-knowledge key).
 *   zk inputs   a zero-knowledge key takes omega32, pbar32 (n scalars) and omega_bar32 -- what the reference draws from its
 *               rng is the caller's to draw; a key without s takes none of them.  Anything else is SNARKV_HOST_ERR_ARG.
 *   absorbed    the raw bytes the transcript's hasher has taken so far, absorbed_len of them (null when 0)
 *   proof_out   64 k + 64 bytes, + 64 for a zero-knowledge key; proof_cap too small is SNARKV_HOST_ERR_CAPACITY with the
 *               needed length in *proof_len
 *   acc_out     32 k + 64 bytes: the accumulator, as snarkv_host_pallas_ipa_decide_all takes it
 * A point at infinity that would have to be written (the zero polynomial) is SNARKV_HOST_ERR_TRANSCRIPT, as the
 * reference's `write_ec_point` fails; a non-canonical scalar is SNARKV_HOST_ERR_PANIC. */
int snarkv_host_pallas_ipa_create_proof(const snarkv_host_pallas_ipa_dk* dk, const uint8_t* poly32, size_t n,
                                        const uint8_t z32[32], const uint8_t* omega32_or_null,
                                        const uint8_t* pbar32_or_null, const uint8_t* omega_bar32_or_null,
                                        const uint8_t* absorbed, size_t absorbed_len, uint8_t* proof_out, size_t proof_cap,
                                        size_t* proof_len, uint8_t* acc_out);

#ifdef __cplusplus
}
#endif
#endif
