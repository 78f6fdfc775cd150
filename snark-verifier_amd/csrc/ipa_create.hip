// `Ipa::create_proof` in one call (include/snarkv_ipa_create.h): the argument checks, the staging of the call's device block
// and the session; the opening itself -- the blinding, the rounds and halo2's Blake2b transcript on the device, one
// synchronisation -- is ipa_opening.hip's, in `TranscriptOrder::Ipa`.  Same source for both curves.
#include <string.h>
#include <vector>
#include "ipa_opening.hpp"
#include "../../include/snarkv_ipa_create.h"

namespace snarkv {
namespace {

struct CreateArgs {
  const uint8_t *h64, *s64, *z32, *omega32, *omega_bar32, *absorbed;
  const void *coeffs, *pbar;
  bool on_device;
  size_t n, absorbed_len;
};
const char kWho[] = "ipa_create_proof";

int create_proof(snarkv_ctx* ctx, const snarkv_ipa_dk* dk, const CreateArgs& a, uint8_t* proof_out, size_t proof_cap,
                 size_t* proof_len, uint8_t* xi_out32, uint8_t* u_out64) {
  if (!ctx || !dk || !a.h64 || !a.coeffs || !a.z32 || !proof_out || !proof_len || !xi_out32 || !u_out64 ||
      (a.absorbed_len && !a.absorbed))
    return SNARKV_ERR_ARG;
  *proof_len = 0;
  const int given = (a.s64 != nullptr) + (a.omega32 != nullptr) + (a.pbar != nullptr) + (a.omega_bar32 != nullptr);
  if (given != 0 && given != 4) {
    set_last_error("ipa_create_proof: s, omega, p_bar and omega_bar come together (zk) or not at all");
    return SNARKV_ERR_ARG;
  }
  const bool zk = given == 4;
  if (dk->device != ctx->device) return SNARKV_ERR_ARG;
  if (dk->first != 0 || dk->count != ((size_t)1 << dk->k) || dk->k < 1 || dk->k > 30) return SNARKV_ERR_LENGTH;
  if (a.n != dk->count) return SNARKV_ERR_LENGTH;
  const size_t need = 64 * (size_t)dk->k + 64 + (zk ? 64 : 0);
  if (proof_cap < need) {
    *proof_len = need;
    set_last_error("ipa_create_proof: the proof has %zu bytes, proof_cap is %zu", need, proof_cap);
    return SNARKV_ERR_LENGTH;
  }
  const bool validate = (ctx->flags & SNARKV_FLAG_VALIDATE) != 0;
  if (validate && (!host_canonical(a.z32) || (zk && (!host_canonical(a.omega32) || !host_canonical(a.omega_bar32))))) {
    set_last_error("ipa_create_proof: z, omega or omega_bar is not canonical");
    return SNARKV_ERR_ENCODING;
  }
  SNARKV_HIP(hipSetDevice(ctx->device));
  // what the host stages: the transcript after the caller's prefix, and the constants of the zk commitment
  std::vector<uint8_t> st(OP_STAGED, 0);
  {
    Blake2bState hs;
    tr_init(hs);
    b2b_update(hs, a.absorbed, a.absorbed_len);
    memcpy(&st[OP_STATE], &hs, sizeof(hs));
  }
  if (zk) {
    memcpy(&st[OP_OMEGA], a.omega32, 32);
    memcpy(&st[OP_OMEGA + 32], a.omega_bar32, 32);
    opening_stage_blinding(st.data(), a.omega_bar32, a.s64);
  }
  snarkv_ipa_prover* p = nullptr;
  SNARKV_TRY(session_open(ctx, dk, a.coeffs, a.on_device, a.n, a.z32, a.h64, nullptr, kWho, &p));
  Buffers bufs(ctx->stream);
  void *d_blk = nullptr, *d_pbar = nullptr;
  int rc = bufs.get(&d_blk, OP_BYTES);
  if (rc == SNARKV_OK && zk) rc = bufs.get(&d_pbar, a.n * 32);
  if (rc == SNARKV_OK && hipMemcpyAsync(d_blk, st.data(), st.size(), hipMemcpyHostToDevice, ctx->stream) != hipSuccess) {
    set_last_error("ipa_create_proof: upload failed");
    rc = SNARKV_ERR_DEVICE;
  }
  if (rc == SNARKV_OK && zk) rc = opening_upload_pbar(ctx, kWho, d_pbar, a.pbar, a.on_device, a.n, (int*)(p->d_small + SM_BAD));
  if (rc != SNARKV_OK) {
    session_close(p);  // a failure may have left work in flight
    return rc;
  }
  SNARKV_TRY(opening_prove(p, (uint8_t*)d_blk, d_pbar, TranscriptOrder::Ipa, kWho, "c_bar", proof_out, xi_out32, u_out64));
  bufs.drained = true;
  *proof_len = need;
  return SNARKV_OK;
}

}  // namespace
}  // namespace snarkv

using namespace snarkv;

extern "C" {

int SNARKV_API(ipa_create_proof)(snarkv_ctx* ctx, const snarkv_ipa_dk* dk, const uint8_t h64[64], const uint8_t* s64,
                                 const uint8_t* coeffs32, size_t n, const uint8_t z32[32], const uint8_t* omega32,
                                 const uint8_t* pbar32, const uint8_t* omega_bar32, const uint8_t* absorbed,
                                 size_t absorbed_len, uint8_t* proof_out, size_t proof_cap, size_t* proof_len,
                                 uint8_t* xi_out32, uint8_t u_out64[64]) {
  const CreateArgs a = {h64, s64, z32, omega32, omega_bar32, absorbed, coeffs32, pbar32, false, n, absorbed_len};
  return create_proof(ctx, dk, a, proof_out, proof_cap, proof_len, xi_out32, u_out64);
}

int SNARKV_API(ipa_create_proof_dev)(snarkv_ctx* ctx, const snarkv_ipa_dk* dk, const uint8_t h64[64], const uint8_t* s64,
                                     const void* d_coeffs32, size_t n, const uint8_t z32[32], const uint8_t* omega32,
                                     const void* d_pbar32, const uint8_t* omega_bar32, const uint8_t* absorbed,
                                     size_t absorbed_len, uint8_t* proof_out, size_t proof_cap, size_t* proof_len,
                                     uint8_t* xi_out32, uint8_t u_out64[64]) {
  const CreateArgs a = {h64, s64, z32, omega32, omega_bar32, absorbed, d_coeffs32, d_pbar32, true, n, absorbed_len};
  return create_proof(ctx, dk, a, proof_out, proof_cap, proof_len, xi_out32, u_out64);
}

}  // extern "C"
