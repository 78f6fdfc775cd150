/* snarkv_host_kzg_open.h -- the prover's half of the two KZG multi-open schemes in one call for the callers of
 * snarkv_host.h (libsnarkv_host.so): `Gwc19::create_proof` / `Bdfg21::create_proof` of the host mirror (host/pcs.hpp) over a
 * transcript of the caller's kind, on top of the device provers of snarkv_kzg_multiopen.h.  The polynomials and the SRS are
 * resident on the device; the transcript is the host's.
 *
 * Byte layouts and the negative SNARKV_HOST_ERR_* codes are those of snarkv_host.h; the call returns 1 when the opening is
 * written, and snarkv_host_last_error() has the message of a failure.
 *
 *   mos          SNARKV_HOST_MOS_GWC19 or SNARKV_HOST_MOS_BDFG21
 *   transcript   SNARKV_HOST_TRANSCRIPT_EVM or SNARKV_HOST_TRANSCRIPT_POSEIDON: a fresh transcript of that kind, to which
 *                the prefix is replayed first
 *   prefix       a list of tagged items, prefix_len bytes in all: 0 | scalar (32 bytes, written), 1 | point (64 bytes,
 *                written), 2 (squeeze a challenge and discard it).  Enough to reproduce any transcript state.  Null when
 *                prefix_len = 0.
 *   ctx, d_srs64, d_polys32, n, n_polys, z32, q_poly, q_shift32, q_eval32, n_queries
 *                as snarkv_kzg_gwc19_create_proof_dev / snarkv_kzg_bdfg21_create_proof_dev take them; `ctx` is a context of
 *                libsnarkv_amd.so on whose stream the polynomials are ready
 *   proof_out    the bytes the opening wrote to the transcript, after the prefix's: Gwc19 W_1..W_S, Bdfg21 W | W', in the
 *                transcript's encoding (EVM: 64 bytes a point, Poseidon: 32).  *proof_len is always set;
 *                SNARKV_HOST_ERR_CAPACITY when proof_cap is too small.
 *   challenges_out32   Gwc19: v (32 bytes); Bdfg21: mu | gamma | z' (96 bytes)
 *
 * An evaluation that does not match its polynomial, or points of a set that coincide, return 0 (the assertion failure of the
 * mirror) with the device's message; a point at infinity that would have to be written is SNARKV_HOST_ERR_TRANSCRIPT, a
 * non-canonical scalar among the arguments SNARKV_HOST_ERR_ARG. */
#ifndef SNARKV_HOST_KZG_OPEN_H
#define SNARKV_HOST_KZG_OPEN_H
#include "snarkv_host.h"
#include "snarkv_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

int snarkv_host_kzg_open(int mos, int transcript, snarkv_ctx* ctx, const void* d_srs64, const void* d_polys32, size_t n,
                         size_t n_polys, const uint8_t z32[32], const uint32_t* q_poly, const uint8_t* q_shift32,
                         const uint8_t* q_eval32, size_t n_queries, const uint8_t* prefix, size_t prefix_len,
                         uint8_t* proof_out, size_t proof_cap, size_t* proof_len, uint8_t* challenges_out32);

#ifdef __cplusplus
}
#endif
#endif /* SNARKV_HOST_KZG_OPEN_H */
