/* snarkv_pallas_session.h -- what a prover session of the host mirror on pallas (include/snarkv_host_pallas_plonk_prove.h,
 * host/plonk_prover.hpp) needs of libsnarkv_pallas.so besides the stages that exist (snarkv_ntt.h, snarkv_quotient.h,
 * snarkv_quotient_cosets.h, snarkv_poly_batch.h, snarkv_poly.h, snarkv_ipa_commit_blinded.h, snarkv_ipa_multiopen.h): the
 * session's resident memory, copies ordered on the context's stream, and the check that the top of the quotient is zero.
 * The contracts are those of snarkv_plonk_prove.h (libsnarkv_amd.so), call for call; the code behind both is one.
 *
 * libsnarkv_pallas.so only.  Conventions of snarkv_amd.h: return 0 or a negative SNARKV_ERR_*; the context is one of
 * snarkv_pallas_ctx_create (snarkv_pallas.h).
 *
 * pallas_session_alloc       `bytes` of device memory on the context's device, 256-byte aligned, set to zero on the context's
 *                            stream.  SNARKV_ERR_EMPTY for bytes = 0, SNARKV_ERR_DEVICE when the device has no room.
 * pallas_session_free        gives it back; waits for the work that may still use it.  A null address is ignored.
 * pallas_session_upload      host -> device, ordered on the stream; the source is consumed before the call returns
 * pallas_session_copy        device -> device, ordered on the stream; the ranges do not overlap
 * pallas_session_download    device -> host, then waits for the stream: the one call here that synchronises
 * pallas_poly_tail_check_dev *status |= 1 when any of the `count` elements (32 bytes each, 16-byte aligned) at d_tail32 is
 *                            not zero as bytes: the quotient's coefficients from num_chunk * n on, canonical as the inverse
 *                            transform leaves them.  Enqueued on the stream; the word (4 bytes of device memory, 4-byte
 *                            aligned, set by the caller beforehand) is read at the caller's next synchronisation.  Nothing of
 *                            the tail comes to the host.  count = 0 enqueues nothing.  count > 2^36 is SNARKV_ERR_LENGTH.
 *
 * A null context or address, a misaligned address or overlapping ranges of a copy: SNARKV_ERR_ARG, before any device work. */
#ifndef SNARKV_PALLAS_SESSION_H
#define SNARKV_PALLAS_SESSION_H
#include "snarkv_pallas.h"

#ifdef __cplusplus
extern "C" {
#endif

int snarkv_pallas_session_alloc(snarkv_ctx* ctx, size_t bytes, void** d_out);
void snarkv_pallas_session_free(snarkv_ctx* ctx, void* d_mem);
int snarkv_pallas_session_upload(snarkv_ctx* ctx, void* d_dst, const void* src, size_t bytes);
int snarkv_pallas_session_copy(snarkv_ctx* ctx, void* d_dst, const void* d_src, size_t bytes);
int snarkv_pallas_session_download(snarkv_ctx* ctx, void* dst, const void* d_src, size_t bytes);
int snarkv_pallas_poly_tail_check_dev(snarkv_ctx* ctx, const void* d_tail32, size_t count, void* d_status);

#ifdef __cplusplus
}
#endif
#endif /* SNARKV_PALLAS_SESSION_H */
