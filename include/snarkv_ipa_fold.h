/* snarkv_ipa_fold.h -- `IpaAs::decide_all` (reference snark-verifier/src/pcs/ipa/decider.rs:57-66) as ONE
 * folded check over a random linear combination: for a challenge rho,
 *     sum_{i<m} rho^i U_i  ==  < sum_{i<m} rho^i h_coeffs(xi_i) , G >
 * is one MSM of 2^k terms and one of m terms whatever m.  If any U_i is wrong the difference of the two
 * sides is a non-zero polynomial in rho of degree < m over a group of prime order r, so a bad batch is
 * accepted for at most m - 1 of the r values of rho: probability (m - 1) / r < 2^-230 for a rho the prover
 * could not predict (both curves have cofactor 1; every U_i is checked to be a point of the curve).
 *
 * THE CALLER OWNS rho.  These calls take it as an argument and say nothing about where it came from: a
 * constant, or a value fixed before the accumulators were, makes the check worthless.  Derive it from the
 * accumulators themselves (a hash of k, m, every xi and every U, and a seed of the verifier's if it has one)
 * or draw it from a CSPRNG after they are fixed.
 *
 * Two families with the same shapes, as in snarkv_ipa_batch.h: snarkv_ipa_* (libsnarkv_amd.so, BN254) and
 * snarkv_pallas_ipa_* (libsnarkv_pallas.so).  Scalars 32-byte little-endian canonical, points x || y
 * 64 bytes little-endian canonical, identity = 64 zero bytes, return 0 or a negative SNARKV_ERR_*.  The
 * calls speak the wire form whatever the context's default flags say.                                 */
#ifndef SNARKV_IPA_FOLD_H
#define SNARKV_IPA_FOLD_H
#include "snarkv_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

/* h = sum_{i<m} rho^i h_coeffs(xi_i): xi32 = m x k scalars (host), d_h32 = 2^k scalars (device, 16-byte
 * aligned).  slices: accumulator slices per coefficient block, 0 = chosen so that the launch fills the
 * device; at most min(m, 32 768), and fewer when their partial vectors would exceed 256 MiB.  1 <= k <= 28,
 * m <= 2^20 (SNARKV_ERR_LENGTH), m == 0 SNARKV_ERR_EMPTY; under SNARKV_FLAG_VALIDATE a non-canonical
 * xi or rho is SNARKV_ERR_ENCODING.  The host arguments are consumed before the call returns; the
 * kernels are enqueued on the context's stream. */
int snarkv_ipa_fold_coeffs_dev(snarkv_ctx* ctx, uint32_t k, const uint8_t* xi32, size_t m, const uint8_t rho32[32],
                               uint32_t slices, void* d_h32);
/* *all_ok = 1 iff sum rho^i U_i == <sum rho^i h_coeffs(xi_i), G>: xi32 = m x k scalars, u64 = m points.
 * An off-curve or non-canonical U_i is a reject (*all_ok = 0), not an error code; an all-zero U_i is the
 * identity.  m == 0 SNARKV_ERR_EMPTY, a shard key SNARKV_ERR_LENGTH, key of another device
 * SNARKV_ERR_ARG; under SNARKV_FLAG_VALIDATE a non-canonical xi or rho is SNARKV_ERR_ENCODING.  Uses the
 * key's window table (snarkv_ipa_batch.h) when it is already built and never builds it.  Synchronous. */
int snarkv_ipa_decide_folded(snarkv_ctx* ctx, const snarkv_ipa_dk* dk, const uint8_t* xi32, const uint8_t* u64,
                             size_t m, const uint8_t rho32[32], int* all_ok);
/* on the library's default context */
int bn254_ipa_decide_folded(const snarkv_ipa_dk* dk, const uint8_t* xi32, const uint8_t* u64, size_t m,
                            const uint8_t rho32[32], int* all_ok);

/* the same on pallas (libsnarkv_pallas.so, include/snarkv_pallas.h's context and key) */
int snarkv_pallas_ipa_fold_coeffs_dev(snarkv_ctx* ctx, uint32_t k, const uint8_t* xi32, size_t m,
                                      const uint8_t rho32[32], uint32_t slices, void* d_h32);
int snarkv_pallas_ipa_decide_folded(snarkv_ctx* ctx, const snarkv_ipa_dk* dk, const uint8_t* xi32, const uint8_t* u64,
                                    size_t m, const uint8_t rho32[32], int* all_ok);
int pallas_ipa_decide_folded(const snarkv_ipa_dk* dk, const uint8_t* xi32, const uint8_t* u64, size_t m,
                             const uint8_t rho32[32], int* all_ok);

#ifdef __cplusplus
}
#endif
#endif /* SNARKV_IPA_FOLD_H */
