/* snarkv_host_pallas.h -- C ABI of the pasta flavour of the host mirror (libsnarkv_host_pallas.so): verify and
 * aggregate halo2 IPA proofs on pallas -- `PlonkVerifier<IpaAs<pallas::Affine, Bgh19>>` with halo2's Blake2b
 * transcript, the setting of the reference's system/halo2/test/ipa/native.rs -- for callers that hand over BYTES,
 * with every EC operation on the MI355X (through libsnarkv_pallas.so, include/snarkv_pallas.h).
 *
 * What each entry point stands for in the reference (snark-verifier/src/...):
 *   snarkv_host_pallas_protocol_parse     a `PlonkProtocol` value (verifier/plonk/protocol.rs:19-71), packed form
 *   snarkv_host_pallas_ipa_dk_create      `IpaDecidingKey` (pcs/ipa/decider.rs:3-22): svk = (k, g[0], h, s), g = the
 *                                         2^k committing-key points, uploaded to the device once per handle
 *   snarkv_host_pallas_plonk_succinct_verify_batch
 *                                         N x `PlonkSuccinctVerifier::{read_proof, verify}` (verifier/plonk.rs:58-92)
 *                                         with the 2N MSMs of the succinct checks in ONE segmented device launch
 *   snarkv_host_pallas_ipa_decide_all     `AccumulationDecider::decide_all` (pcs/ipa/decider.rs:47-66)
 *   snarkv_host_pallas_plonk_verify       `PlonkVerifier::verify` (verifier/plonk.rs:133): succinct verify + decide_all
 *   snarkv_host_pallas_ipa_as_create_proof  `IpaAs::create_proof` (pcs/ipa/accumulation.rs:148-226), device prover
 *   snarkv_host_pallas_ipa_as_verify      `IpaAs::{read_proof, verify}` (pcs/ipa/accumulation.rs:21-146)
 *   snarkv_host_pallas_aggregate          the whole job: succinct-verify N proofs -> `IpaAs::create_proof` -> decide
 *
 * Byte layouts: Fr (pallas::Scalar) / Fp 32 B little-endian canonical; a point 64 B x|y (identity = zeros);
 * an accumulator = k x xi (32 B each) | u (64 B), k the key's; the protocol in the packed form of
 * snark-verifier_amd/host/wire.hpp; instances per proof `u32 columns, per column u32 m, m x Fr`; proofs per proof
 * `u32 len, bytes` -- as in snarkv_host.h.  A proof's commitments are compressed pallas points (32 B: x, bit 255 =
 * parity of y).
 * Return codes: 1 accept / done, 0 reject (`Error::AssertionFailure`), SNARKV_HOST_ERR_* of snarkv_host.h otherwise.
 * Ownership: the caller owns every buffer; handles are freed with the matching *_free, are immutable after creation
 * and may be shared between threads.  snarkv_host_pallas_last_error is thread-local.  Device work is serialised on the
 * process-global context of libsnarkv_pallas.so.  There is NO CPU fallback.
 */
#ifndef SNARKV_HOST_PALLAS_H
#define SNARKV_HOST_PALLAS_H
#include "snarkv_host.h" /* the SNARKV_HOST_ERR_* codes */

#ifdef __cplusplus
extern "C" {
#endif

/* Who takes the square roots of a batch's compressed points (12 + 2k per StandardPlonk proof; p - 1 = 2^32 t makes
 * each a Tonelli-Shanks on the host):
 *   HOST    the transcripts, on the host pool
 *   DEVICE  one launch of snarkv_pallas_g1_decompress over the points of all N proofs, then the transcripts read
 *           with the answers as hints; whatever the device refuses goes through the host path, so verdicts and
 *           error codes are the same as under HOST
 *   AUTO    DEVICE from SNARKV_HOST_PALLAS_DEVICE_MIN proofs on, HOST below */
#define SNARKV_HOST_PALLAS_DECOMPRESS_HOST 0
#define SNARKV_HOST_PALLAS_DECOMPRESS_DEVICE 1
#define SNARKV_HOST_PALLAS_DECOMPRESS_AUTO 2
/* The smallest measured batch at which DEVICE beat HOST: every one, down to a single proof (k = 8, 16 host threads,
 * ms per call, median [min .. max]: N = 1: 0.80 [0.76 .. 0.85] against 1.31 [1.28 .. 1.32], N = 64: 2.65 against 6.92,
 * N = 1 024: 11.35 against 68.33; the launch itself lasts 0.20 - 0.22 ms whatever the batch;
 * tools/bench_pallas_verify.py, profiles/pallas_verify_bench.txt).  So AUTO is DEVICE for any
 * batch; HOST stays an explicit route. */
#define SNARKV_HOST_PALLAS_DEVICE_MIN 1

typedef struct snarkv_host_pallas_protocol snarkv_host_pallas_protocol;
typedef struct snarkv_host_pallas_ipa_dk snarkv_host_pallas_ipa_dk;

/* thread-local message of the last failing call on this thread */
const char* snarkv_host_pallas_last_error(void);

int snarkv_host_pallas_protocol_parse(const uint8_t* bytes, size_t len, snarkv_host_pallas_protocol** out);
void snarkv_host_pallas_protocol_free(snarkv_host_pallas_protocol* p);

/* g: 2^k points; s_or_null: the blinding base S of a zero-knowledge key (what halo2 proofs need), or NULL */
int snarkv_host_pallas_ipa_dk_create(uint32_t k, const uint8_t* g_points64, const uint8_t h[64], const uint8_t* s_or_null,
                                     snarkv_host_pallas_ipa_dk** out);
void snarkv_host_pallas_ipa_dk_free(snarkv_host_pallas_ipa_dk* dk);

/* N proofs of one protocol -> one accumulator each, in proof order (accs_cap in bytes; N x (32 k + 64) needed).
 * host_threads: threads of the host half (0 = all of the pool); decompress: SNARKV_HOST_PALLAS_DECOMPRESS_*. */
int snarkv_host_pallas_plonk_succinct_verify_batch(const snarkv_host_pallas_protocol* protocol,
                                                   const snarkv_host_pallas_ipa_dk* dk, const uint8_t* instances,
                                                   size_t instances_len, const uint8_t* proofs, size_t proofs_len,
                                                   uint32_t n, unsigned host_threads, int decompress, uint8_t* accs_out,
                                                   size_t accs_cap);

/* 1 if every accumulator passes U == <h_coeffs(xi), G>; ok_out (optional): the verdict of each */
int snarkv_host_pallas_ipa_decide_all(const snarkv_host_pallas_ipa_dk* dk, const uint8_t* accs, uint32_t m, uint8_t* ok_out);

int snarkv_host_pallas_plonk_verify(const snarkv_host_pallas_protocol* protocol, const snarkv_host_pallas_ipa_dk* dk,
                                    const uint8_t* instances, size_t instances_len, const uint8_t* proofs,
                                    size_t proofs_len, uint32_t n, unsigned host_threads, int decompress);

/* m >= 2 accumulators -> one, over a fresh Blake2b transcript.  rand32: the n_rand scalars the reference would draw
 * from its rng, in its order (a zero-knowledge key draws a, b, omega, then 2^k + 1 for the opening; a key without S
 * none); running out is SNARKV_HOST_ERR_PANIC.  proof_out receives the accumulation proof (*proof_len is always set;
 * SNARKV_HOST_ERR_CAPACITY when proof_cap is too small), acc_out the new accumulator. */
int snarkv_host_pallas_ipa_as_create_proof(const snarkv_host_pallas_ipa_dk* dk, const uint8_t* accs, uint32_t m,
                                           const uint8_t* rand32, size_t n_rand, uint8_t* proof_out, size_t proof_cap,
                                           size_t* proof_len, uint8_t* acc_out);
/* the verifier's side: bytes left over after the proof -> SNARKV_HOST_ERR_TRAILING */
int snarkv_host_pallas_ipa_as_verify(const snarkv_host_pallas_ipa_dk* dk, const uint8_t* accs, uint32_t m,
                                     const uint8_t* proof, size_t proof_len, uint8_t* acc_out);

/* succinct-verify N proofs, accumulate (`IpaAs::create_proof` with rand32 as above), decide the result.  With n = 1
 * there is nothing to accumulate: the single accumulator is decided, *as_proof_len = 0 (the SDK's `aggregate`).
 * timings_ms (optional, 5 doubles): read_proofs, succinct_verify, accumulate, decide, total -- written on every return
 * past the argument checks, whatever the code: a stage that was not reached (or that a device error cut short) is 0,
 * total is the time until the return.
 * as_proof_out / acc_out (optional): the accumulation proof and the final accumulator (also written on reject). */
int snarkv_host_pallas_aggregate(const snarkv_host_pallas_protocol* protocol, const snarkv_host_pallas_ipa_dk* dk,
                                 const uint8_t* instances, size_t instances_len, const uint8_t* proofs, size_t proofs_len,
                                 uint32_t n, unsigned host_threads, int decompress, const uint8_t* rand32, size_t n_rand,
                                 double* timings_ms, uint8_t* as_proof_out, size_t as_proof_cap, size_t* as_proof_len,
                                 uint8_t* acc_out);

#ifdef __cplusplus
}
#endif
#endif
