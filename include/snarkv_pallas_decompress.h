/* snarkv_pallas_decompress.h -- batched point decompression on pallas (libsnarkv_pallas.so), next to
 * snarkv_pallas.h and with its conventions.
 *
 * `C::from_bytes` for C = pallas::Affine as the Blake2b transcript of a halo2 IPA proof calls it once
 * per commitment (`Blake2bRead::read_point`): n compressed points in, one kernel launch, one lane per
 * point, a fixed-trip-count square root in Fp (p - 1 = 2^32 t) per lane.
 *
 *   in32   n x 32 bytes: x little-endian canonical (x < p), bit 255 = parity of y
 *   out64  n x 64 bytes: x || y canonical; the context's SNARKV_FLAG_MONTGOMERY, where set, selects
 *          halo2curves' in-memory form as it does for snarkv_g1_decompress
 *   ok     n bytes: 0 for x >= p or x^3 + 5 not a square (out64 is 64 zero bytes then), 1 otherwise
 *
 * The all-zero encoding is the identity: 64 zero bytes, ok = 1 (a transcript refuses it afterwards).
 * n = 0 -> SNARKV_OK and nothing is touched; a NULL context, or a NULL buffer with n > 0 ->
 * SNARKV_ERR_ARG; n >= 2^32 -> SNARKV_ERR_LENGTH.  Synchronous: the results are in place on return. */
#ifndef SNARKV_PALLAS_DECOMPRESS_H
#define SNARKV_PALLAS_DECOMPRESS_H
#include "snarkv_pallas.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Default flags of a pasta context, as snarkv_ctx_set_flags sets them for a BN254 one (SNARKV_FLAG_VALIDATE,
 * SNARKV_FLAG_MONTGOMERY of snarkv_amd.h; any other bit -> SNARKV_ERR_ARG): OR-ed into every later call on the
 * context.  A new context has none. */
int snarkv_pallas_ctx_set_flags(snarkv_ctx* ctx, uint32_t flags);

int snarkv_pallas_g1_decompress(snarkv_ctx* ctx, const uint8_t* in32, size_t n, uint8_t* out64, uint8_t* ok);
/* over the process-global context of the pallas_* entry points (device 0) */
int pallas_g1_decompress(const uint8_t* in32, size_t n, uint8_t* out64, uint8_t* ok);

#ifdef __cplusplus
}
#endif
#endif
