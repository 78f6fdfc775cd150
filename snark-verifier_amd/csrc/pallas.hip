// The pasta build of the curve-generic part of the library -> libsnarkv_pallas.so
// (include/snarkv_pallas.h).  The reference's IPA layer is generic over `C: CurveAffine`
// and its own tests run it on pallas (snark-verifier/src/pcs/ipa.rs:434-466,
// pcs/ipa/accumulation.rs:240-290), whose only device-worthy work is
// `util::msm::multi_scalar_multiplication` (msm.rs:308-343: `IpaProvingKey::commit`,
// pcs/ipa.rs:220-229, and `IpaAs::decide`, pcs/ipa/decider.rs:47-55).
//
// Same sources as the BN254 library -- ctx.hip / msm_api.hip / fq29.h / fr29.h / g1_29.h / glv.h /
// msm_pippenger.hip / msm_naive.hip / ipa.hip / ipa_prover.hip -- compiled with
//   -DSNARKV_CURVE_PALLAS   pallas_consts.h: p, r, b = 5 (curve_consts.h); the pasta policy of the MSM
//                           entry layer (SNARKV_CHUNK_PIPELINE, SNARKV_API_FLAGS: ctx.hpp)
//   -Dsnarkv=snarkv_pallas  the C++ namespace, so both libraries can live in one process
// msm_naive.hip (the segmented small-MSM kernels behind `NativeLoader::multi_scalar_multiplication`,
// loader/native.rs:61-71) comes along; pallas has the same kind of endomorphism as BN254 (j = 0), so
// the GLV split stays on, with pallas' lattice.  There is no pairing, no KZG decider and no transcript.
// This unit holds what has no BN254 twin: the exported host-staged Pippenger (no `flags` argument), the
// entry point of the batched point decompression (decompress_pallas.hip) and the context-free pallas_* forms.
#include <mutex>
#include "ctx.hpp"
#include "../../include/snarkv_ipa_batch.h"
#include "../../include/snarkv_ipa_fold.h"
#include "../../include/snarkv_ipa_create.h"
#include "../../include/snarkv_ipa_multiopen.h"
#include "../../include/snarkv_pallas.h"
#include "../../include/snarkv_pallas_decompress.h"

using namespace snarkv;

extern "C" {

int snarkv_pallas_g1_msm_pippenger(snarkv_ctx* ctx, const uint8_t* scalars32, const uint8_t* points64, size_t n,
                                   uint8_t out64[64]) {
  return msm_pippenger_staged(ctx, scalars32, points64, n, 0, out64);
}

// `C::from_bytes` for a batch (include/snarkv_pallas_decompress.h; the kernel: decompress_pallas.hip), staged as
// snarkv_g1_decompress stages its own
int snarkv_pallas_g1_decompress(snarkv_ctx* ctx, const uint8_t* in32, size_t n, uint8_t* out64, uint8_t* ok) {
  if (!ctx || (n && (!in32 || !out64 || !ok))) return SNARKV_ERR_ARG;
  if (n == 0) return SNARKV_OK;
  if (n > 0xFFFFFFFFull) return SNARKV_ERR_LENGTH;
  SNARKV_HIP(hipSetDevice(ctx->device));
  void *d_in, *d_out;
  SNARKV_TRY(stage_in(ctx, SLOT_IN_POINTS, in32, n * 32, &d_in));
  SNARKV_TRY(ctx_reserve(ctx, SLOT_OUT, n * 64 + n, &d_out));  // the points, then one validity byte each
  SNARKV_TRY(launch_g1_decompress(ctx, d_in, n, d_out, (uint8_t*)d_out + n * 64));
  SNARKV_HIP(hipMemcpyAsync(ok, (const uint8_t*)d_out + n * 64, n, hipMemcpyDeviceToHost, ctx->stream));
  return fetch_out(ctx, d_out, out64, n * 64);
}

// snarkv_ctx_set_flags for a pasta context: the default flags of every call on it
int snarkv_pallas_ctx_set_flags(snarkv_ctx* ctx, uint32_t flags) {
  if (!ctx || (flags & ~(SNARKV_FLAG_VALIDATE | SNARKV_FLAG_MONTGOMERY))) return SNARKV_ERR_ARG;
  ctx->flags = flags;
  ctx->mont = (flags & SNARKV_FLAG_MONTGOMERY) != 0;
  return SNARKV_OK;
}

// ---- context-free forms (what a `NativeLoader`-style unit struct binds: loader.rs:108 has no &self) ----
static std::mutex g_default_mu;
static snarkv_ctx* g_default_ctx = nullptr;
static std::recursive_mutex g_default_call_mu;  // one shared context: calls from different host threads take turns
static int default_ctx(snarkv_ctx** out) {
  std::lock_guard<std::mutex> lk(g_default_mu);
  if (!g_default_ctx) {
    int rc = snarkv_pallas_ctx_create(0, nullptr, &g_default_ctx);
    if (rc < 0) return rc;
  }
  *out = g_default_ctx;
  return SNARKV_OK;
}
#define PALLAS_DEFAULT_CTX()                                             \
  std::lock_guard<std::recursive_mutex> _call_lock(g_default_call_mu);   \
  snarkv_ctx* c;                                                         \
  SNARKV_TRY(default_ctx(&c))

int pallas_g1_msm_naive(const uint8_t* scalars32, const uint8_t* points64, size_t n, uint8_t out64[64]) {
  PALLAS_DEFAULT_CTX();
  return snarkv_pallas_g1_msm_naive(c, scalars32, points64, n, 0, out64);
}
int pallas_g1_msm_batched(const uint8_t* scalars32, const uint8_t* points64, const uint32_t* offsets, size_t n_msm,
                          uint8_t* out) {
  PALLAS_DEFAULT_CTX();
  return snarkv_pallas_g1_msm_batched(c, scalars32, points64, offsets, n_msm, 0, out);
}
int pallas_host_buffer(int slot, size_t bytes, void** out) {
  PALLAS_DEFAULT_CTX();
  return snarkv_pallas_ctx_host_buffer(c, slot, bytes, out);
}
int pallas_g1_msm_pippenger(const uint8_t* scalars32, const uint8_t* points64, size_t n, uint8_t out64[64]) {
  PALLAS_DEFAULT_CTX();
  return snarkv_pallas_g1_msm_pippenger(c, scalars32, points64, n, out64);
}
int pallas_ipa_dk_create(const uint8_t* g_points64, size_t n, snarkv_ipa_dk** out) {
  PALLAS_DEFAULT_CTX();
  return snarkv_pallas_ipa_dk_create(c, g_points64, n, out);
}
int pallas_ipa_decide_batch(const snarkv_ipa_dk* dk, const uint8_t* xi32, const uint8_t* u64, size_t m, uint8_t* ok) {
  PALLAS_DEFAULT_CTX();
  return snarkv_pallas_ipa_decide_batch(c, dk, xi32, u64, m, ok);
}
int pallas_ipa_commit_batch(const snarkv_ipa_dk* dk, const uint8_t* polys32, size_t n, size_t m, uint8_t* out64s) {
  PALLAS_DEFAULT_CTX();
  return snarkv_pallas_ipa_commit_batch(c, dk, polys32, n, m, out64s);
}
int pallas_ipa_decide_folded(const snarkv_ipa_dk* dk, const uint8_t* xi32, const uint8_t* u64, size_t m,
                             const uint8_t rho32[32], int* all_ok) {
  PALLAS_DEFAULT_CTX();
  return snarkv_pallas_ipa_decide_folded(c, dk, xi32, u64, m, rho32, all_ok);
}
int pallas_ipa_create_proof(const snarkv_ipa_dk* dk, const uint8_t h64[64], const uint8_t* s64, const uint8_t* coeffs32, size_t n,
                           const uint8_t z32[32], const uint8_t* omega32, const uint8_t* pbar32, const uint8_t* omega_bar32,
                           const uint8_t* absorbed, size_t absorbed_len, uint8_t* proof_out, size_t proof_cap,
                           size_t* proof_len, uint8_t* xi_out32, uint8_t u_out64[64]) {
  PALLAS_DEFAULT_CTX();
  return snarkv_pallas_ipa_create_proof(c, dk, h64, s64, coeffs32, n, z32, omega32, pbar32, omega_bar32, absorbed, absorbed_len, proof_out,
                                 proof_cap, proof_len, xi_out32, u_out64);
}
int pallas_ipa_multiopen_create_proof(const snarkv_ipa_dk* dk, const uint8_t h64[64], const uint8_t s64[64], const uint8_t* polys32, size_t n, size_t n_polys,
    const uint8_t* blinds32, const uint8_t x32[32], const uint32_t* q_poly, const uint8_t* q_shift32, const uint8_t* q_eval32,
    size_t n_queries, const uint8_t f_blind32[32], const uint8_t* pbar32, const uint8_t omega_bar32[32], const uint8_t* absorbed,
    size_t absorbed_len, uint8_t* proof_out, size_t proof_cap, size_t* proof_len, uint8_t* xi_out32, uint8_t u_out64[64]) {
  PALLAS_DEFAULT_CTX();
  return snarkv_pallas_ipa_multiopen_create_proof(c, dk, h64, s64, polys32, n, n_polys, blinds32, x32, q_poly, q_shift32, q_eval32, n_queries,
                                           f_blind32, pbar32, omega_bar32, absorbed, absorbed_len, proof_out, proof_cap, proof_len,
                                           xi_out32, u_out64);
}

int pallas_g1_decompress(const uint8_t* in32, size_t n, uint8_t* out64, uint8_t* ok) {
  PALLAS_DEFAULT_CTX();
  return snarkv_pallas_g1_decompress(c, in32, n, out64, ok);
}

}  // extern "C"
