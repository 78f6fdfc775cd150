/* snarkv_ipa_batch.h -- many scalar vectors against one resident IPA key per launch: batched
 * `IpaProvingKey::commit` (reference snark-verifier/src/pcs/ipa.rs:221-229), and the window table
 * of a key that it and `snarkv_ipa_decide_batch` share.
 *
 * Two families with the same shapes, as in snarkv_ipa_prover.h: snarkv_ipa_* (libsnarkv_amd.so,
 * BN254, on the snarkv_amd.h context and deciding key) and snarkv_pallas_ipa_* (libsnarkv_pallas.so,
 * on the snarkv_pallas.h context and key).  Scalars 32-byte little-endian canonical, points x || y
 * 64 bytes little-endian canonical, identity = 64 zero bytes, return 0 or a negative SNARKV_ERR_*.
 * The calls speak the wire form whatever the context's default flags say; SNARKV_FLAG_VALIDATE among
 * them makes a non-canonical scalar SNARKV_ERR_ENCODING.
 *
 * The window table of a key is T[w][j] = 2^(8 w) G[j], w < 32: 2 KiB per base, built on the device
 * at most once per key -- by the first batched call that wants it or by snarkv_ipa_dk_prepare -- and
 * freed with the key.  A shard, and a key whose table would exceed 256 MiB (more than 2^17 points),
 * has none: the calls below then run one MSM per vector.  Key handles may be shared between host
 * threads.  The environment variable SNARKV_IPA_SHARED, read once, overrides the routing: 0 = never
 * the table, 1 = whenever it fits.                                                              */
#ifndef SNARKV_IPA_BATCH_H
#define SNARKV_IPA_BATCH_H
#include "snarkv_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Build the window table now.  OK and a no-op if it is built, or if the key has none (see above). */
int snarkv_ipa_dk_prepare(snarkv_ctx* ctx, snarkv_ipa_dk* dk);
/* 0 until the table is built, then 32 * 2^k * 64. */
size_t snarkv_ipa_dk_table_bytes(const snarkv_ipa_dk* dk);
/* out[a] = sum_{j<n} polys[a][j] G[j] for a < m: polys32 = m x n scalars, vector after vector,
 * out64s = m points.  1 <= n <= 2^k (the first n bases); m == 0 or n == 0 is SNARKV_ERR_EMPTY,
 * n > 2^k or a shard SNARKV_ERR_LENGTH.  Synchronous. */
int snarkv_ipa_commit_batch(snarkv_ctx* ctx, const snarkv_ipa_dk* dk, const uint8_t* polys32, size_t n, size_t m,
                            uint8_t* out64s);
/* The same from and to device memory (16-byte aligned), enqueued on the context's stream.  `slices`:
 * how many workgroups share a vector, 0 = chosen so that the launch fills the device. */
int snarkv_ipa_commit_batch_dev(snarkv_ctx* ctx, const snarkv_ipa_dk* dk, const void* d_polys32, size_t n, size_t m,
                                uint32_t slices, void* d_out64s);
/* on the library's default context */
int bn254_ipa_commit_batch(const snarkv_ipa_dk* dk, const uint8_t* polys32, size_t n, size_t m, uint8_t* out64s);

/* the same on pallas (libsnarkv_pallas.so, include/snarkv_pallas.h's context and key) */
int snarkv_pallas_ipa_dk_prepare(snarkv_ctx* ctx, snarkv_ipa_dk* dk);
size_t snarkv_pallas_ipa_dk_table_bytes(const snarkv_ipa_dk* dk);
int snarkv_pallas_ipa_commit_batch(snarkv_ctx* ctx, const snarkv_ipa_dk* dk, const uint8_t* polys32, size_t n, size_t m,
                                   uint8_t* out64s);
int snarkv_pallas_ipa_commit_batch_dev(snarkv_ctx* ctx, const snarkv_ipa_dk* dk, const void* d_polys32, size_t n,
                                       size_t m, uint32_t slices, void* d_out64s);
int pallas_ipa_commit_batch(const snarkv_ipa_dk* dk, const uint8_t* polys32, size_t n, size_t m, uint8_t* out64s);

#ifdef __cplusplus
}
#endif
#endif /* SNARKV_IPA_BATCH_H */
