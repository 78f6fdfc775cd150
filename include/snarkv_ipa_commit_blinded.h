/* snarkv_ipa_commit_blinded.h -- many BLINDED commitments against one resident IPA key per call: halo2's
 * `commit(poly, Blind)`, the reference's `IpaProvingKey::commit` with `omega`
 * (snark-verifier/src/pcs/ipa.rs:221-229), for a whole batch:
 *
 *     out[a] = sum_{j<n} polys[a][j] G[j] + blinds[a] * S,   a < m.
 *
 * Two families with the same shape, as in snarkv_ipa_batch.h: snarkv_ipa_* (libsnarkv_amd.so, BN254) and
 * snarkv_pallas_ipa_* (libsnarkv_pallas.so).  Encodings, argument rules and codes are those of
 * snarkv_ipa_commit_batch_dev: d_polys32 = m x n canonical scalars in device memory, vector after vector,
 * d_out64s = m points in device memory (both 16-byte aligned), 1 <= n <= 2^k (the first n bases); m == 0 or
 * n == 0 is SNARKV_ERR_EMPTY, n > 2^k or a shard SNARKV_ERR_LENGTH, a null argument SNARKV_ERR_ARG.  Besides:
 *
 *   s64       the point S (the key's `s`), 64 bytes on the host.  Null: SNARKV_ERR_ARG.  The point at infinity
 *             (64 zero bytes) is SNARKV_ERR_ENCODING; under SNARKV_FLAG_VALIDATE so is an S with a
 *             non-canonical coordinate or off the curve.  Without the flag S is taken as the key's points
 *             are: as given.
 *   blinds32  m scalars on the host, one per vector.  Null: SNARKV_ERR_ARG.  Under SNARKV_FLAG_VALIDATE a
 *             non-canonical blind is SNARKV_ERR_ENCODING; without the flag it counts mod r.
 *
 * s64 and blinds32 are read before the call returns.  A refused call has written nothing to d_out64s.
 * A zero blind gives the bytes of snarkv_ipa_commit_batch_dev.
 *
 * The call is enqueued on the context's stream and does not wait for it.  (SNARKV_FLAG_VALIDATE does, as in
 * every call; so does the first batched call on a key, which builds its window table; so does the route of
 * one MSM per vector that a key without a table takes -- snarkv_ipa_batch.h says which keys -- to stage its
 * offsets, as snarkv_ipa_commit_batch_dev does there.)
 *
 * On the table route the blind term costs no launch per vector and nothing after the MSM: the 32 points
 * 2^(8 w) S are kept with the context and rebuilt only when S changes; one more kernel, one wavefront per
 * vector, forms blind * S from them as one more partial of the vector's fold, and runs beside the MSM's
 * kernel on a stream of the context's own.  On the other route one segmented launch adds all m blind terms
 * after the per-vector MSMs.                                                                        */
#ifndef SNARKV_IPA_COMMIT_BLINDED_H
#define SNARKV_IPA_COMMIT_BLINDED_H
#include "snarkv_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

int snarkv_ipa_commit_blinded_batch_dev(snarkv_ctx* ctx, const snarkv_ipa_dk* dk, const uint8_t s64[64],
                                        const void* d_polys32, size_t n, size_t m, const uint8_t* blinds32,
                                        uint32_t slices, void* d_out64s);
/* the same on pallas (libsnarkv_pallas.so, include/snarkv_pallas.h's context and key) */
int snarkv_pallas_ipa_commit_blinded_batch_dev(snarkv_ctx* ctx, const snarkv_ipa_dk* dk, const uint8_t s64[64],
                                               const void* d_polys32, size_t n, size_t m, const uint8_t* blinds32,
                                               uint32_t slices, void* d_out64s);

#ifdef __cplusplus
}
#endif
#endif /* SNARKV_IPA_COMMIT_BLINDED_H */
