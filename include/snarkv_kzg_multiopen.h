/* snarkv_kzg_multiopen.h -- the provers of the two KZG multi-open schemes on BN254 (halo2's `ProverGWC` and
 * `ProverSHPLONK`): committed polynomials and a list of (polynomial, rotation, evaluation) queries in, the opening points
 * that `Gwc19Proof::read` / `Bdfg21Proof::read` (reference snark-verifier/src/pcs/kzg/multiopen/gwc19.rs:84-110,
 * bdfg21.rs:85-120) consume out.  The verifier is the definition: the outputs are the ws / (w, w_prime) for which
 * gwc19::msms / bdfg21::msms (host/pcs.hpp, oracle/kzg.py) give lhs = [s] rhs.
 *
 * libsnarkv_amd.so only: KZG is BN254's.  Conventions of snarkv_amd.h: scalars 32-byte little-endian canonical, points
 * x || y 64 bytes with the identity as 64 zero bytes, return 0 or a negative SNARKV_ERR_*.  The calls speak the wire form
 * whatever the context's default flags say: SNARKV_FLAG_MONTGOMERY as a default neither applies to them nor is changed by
 * them; SNARKV_FLAG_VALIDATE as a default applies (below).
 *
 * Arguments
 *   srs64         the n points [s^i] G, i < n (host memory; device memory, 16-byte aligned, for _dev)
 *   polys32       n_polys x n coefficients, poly-major, any 1 <= n <= 2^30 (host memory; device memory, 16-byte aligned, for
 *                 _dev).  Blinding lives in the polynomials: neither scheme draws randomness, the outputs are a function of
 *                 the inputs.
 *   z32           the evaluation challenge
 *   q_poly, q_shift32, q_eval32    the n_queries queries as the three parallel arrays of snarkv_ipa_multiopen.h: the point of
 *                 query i is z * q_shift[i], and q_eval[i] must be polys[q_poly[i]] at that point
 *   v32 / mu32, gamma32    the challenges, which the caller owns: the call knows no transcript
 *   draw_z_prime  Bdfg21: called once on the calling thread, between the two synchronisations, with the 64 bytes of W; writes
 *                 z'.  (A transcript writes W there and squeezes.)  It must not enter the same context.  A non-zero return
 *                 ends the call with SNARKV_ERR_ARG; the context stays usable.
 *
 * snarkv_kzg_multiopen_sets   *n_sets = the number of query sets of a query list.  mos: 0 = Gwc19, 1 = Bdfg21 (the values
 *                 of SNARKV_HOST_MOS_* in snarkv_host.h).  Gwc19 groups the queries by shift, first seen
 *                 (gwc19.rs:142-160); Bdfg21 by polynomial, then polynomials with equal shift sets share a set
 *                 (bdfg21.rs:121-171; a repeated (polynomial, shift) keeps its first evaluation).
 *
 * snarkv_kzg_gwc19_create_proof[_dev]    ws_out64 = W_1..W_S, *n_sets_out = S.  For set k with polynomials p_i and
 *                 evaluations e_i in set order:  W_k = commit((sum_i v^i p_i - sum_i v^i e_i) / (X - z shift_k)).
 *                 ws_cap is in points; too small is SNARKV_ERR_LENGTH with S in *n_sets_out, before any device work.
 *                 All S commitments are one batch of MSMs over the one base; one synchronisation, at the end.
 * snarkv_kzg_bdfg21_create_proof[_dev]   for set i with points z shift_t:  q_i = sum_j mu^j p_j,  r_i the interpolation of
 *                 the mu-combined evaluations,  Z_i = prod_t (X - z shift_t);
 *                   h = sum_i gamma^i (q_i - r_i) / Z_i,                                    w_out64 = commit(h)
 *                   L = sum_i gamma^i (Z_1(z') / Z_i(z')) (q_i - r_i(z')) - Z_1(z') h,      w_prime_out64 = commit(L / (X - z'))
 *                 and z_prime_out32 = z'.  Two synchronisations: after W, and at the end.
 *
 * A commitment of the zero polynomial is the identity: a set with exactly n points is legal and has the zero quotient.
 *
 * Refusals; the outputs are written on success only:
 *   SNARKV_ERR_ARG       a null argument (`user` may be null); a misaligned device address; q_poly[i] >= n_polys; two
 *                        points of a set coinciding (z = 0); a set with more points than n; z' equal to a point of a set;
 *                        draw_z_prime returning non-zero; and an evaluation that does not match its polynomial: a division
 *                        leaves a remainder, which the call notices at its next synchronisation.  snarkv_last_error() then
 *                        names the first offending set ("evaluation does not match the polynomial (query set i)").  The
 *                        context stays usable.
 *   SNARKV_ERR_EMPTY     n = 0, n_polys = 0 or n_queries = 0
 *   SNARKV_ERR_LENGTH    n > 2^30; ws_cap too small
 *   SNARKV_ERR_ENCODING  under SNARKV_FLAG_VALIDATE (a default flag of the context) a non-canonical scalar among z, the
 *                        shifts, the evaluations and the challenges, z' included (checked on the host) or the coefficients
 *                        (on the device, which synchronises once more)
 *   SNARKV_ERR_DEVICE    a HIP error; or, as an internal error with its own message, a remainder of L / (X - z')        */
#ifndef SNARKV_KZG_MULTIOPEN_H
#define SNARKV_KZG_MULTIOPEN_H
#include "snarkv_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SNARKV_KZG_MOS_GWC19 0
#define SNARKV_KZG_MOS_BDFG21 1

typedef int (*snarkv_kzg_challenge_fn)(void* user, const uint8_t w64[64], uint8_t z_prime32[32]);

int snarkv_kzg_multiopen_sets(int mos, const uint32_t* q_poly, const uint8_t* q_shift32, size_t n_queries, size_t* n_sets);

int snarkv_kzg_gwc19_create_proof(snarkv_ctx* ctx, const uint8_t* srs64, const uint8_t* polys32, size_t n, size_t n_polys,
                                  const uint8_t z32[32], const uint32_t* q_poly, const uint8_t* q_shift32,
                                  const uint8_t* q_eval32, size_t n_queries, const uint8_t v32[32], uint8_t* ws_out64,
                                  size_t ws_cap, size_t* n_sets_out);
int snarkv_kzg_gwc19_create_proof_dev(snarkv_ctx* ctx, const void* d_srs64, const void* d_polys32, size_t n, size_t n_polys,
                                      const uint8_t z32[32], const uint32_t* q_poly, const uint8_t* q_shift32,
                                      const uint8_t* q_eval32, size_t n_queries, const uint8_t v32[32], uint8_t* ws_out64,
                                      size_t ws_cap, size_t* n_sets_out);

int snarkv_kzg_bdfg21_create_proof(snarkv_ctx* ctx, const uint8_t* srs64, const uint8_t* polys32, size_t n, size_t n_polys,
                                   const uint8_t z32[32], const uint32_t* q_poly, const uint8_t* q_shift32,
                                   const uint8_t* q_eval32, size_t n_queries, const uint8_t mu32[32],
                                   const uint8_t gamma32[32], snarkv_kzg_challenge_fn draw_z_prime, void* user,
                                   uint8_t w_out64[64], uint8_t z_prime_out32[32], uint8_t w_prime_out64[64]);
int snarkv_kzg_bdfg21_create_proof_dev(snarkv_ctx* ctx, const void* d_srs64, const void* d_polys32, size_t n, size_t n_polys,
                                       const uint8_t z32[32], const uint32_t* q_poly, const uint8_t* q_shift32,
                                       const uint8_t* q_eval32, size_t n_queries, const uint8_t mu32[32],
                                       const uint8_t gamma32[32], snarkv_kzg_challenge_fn draw_z_prime, void* user,
                                       uint8_t w_out64[64], uint8_t z_prime_out32[32], uint8_t w_prime_out64[64]);

#ifdef __cplusplus
}
#endif
#endif /* SNARKV_KZG_MULTIOPEN_H */
