// `decide_all` as one folded check for the pallas product API -> libsnarkv_host_pallas_fold.so
// (include/snarkv_host_pallas_fold.h), compiled with -DSNARKV_HOST_PALLAS like capi_pallas.cpp and linked against
// libsnarkv_host_pallas.so and libsnarkv_pallas.so.  Thin: the challenge is hashed here, the folded check is one call of
// the device library (pallas_ipa_decide_folded, include/snarkv_ipa_fold.h) on the key's resident handle, and everything
// else -- the succinct half of a verify, the per-accumulator verdicts of a rejected batch -- is the C API of
// libsnarkv_host_pallas.so, called as any other client calls it.
#ifndef SNARKV_HOST_PALLAS
#error "compile with -DSNARKV_HOST_PALLAS"
#endif
#include "../../include/snarkv_host_pallas_fold.h"
#include "../../include/snarkv_ipa_fold.h"

#include <cstring>
#include <string>
#include <vector>

#include "blake2b_transcript.hpp"
#include "capi_pallas_handles.hpp"

using namespace snarkv_host;

namespace {
thread_local std::string g_fold_error;

int fail(int code, const std::string& what) {
  g_fold_error = what;
  return code;
}

size_t acc_stride(const snarkv_host_pallas_ipa_dk* dk) { return 32 * dk->dk.svk.k + 64; }

void fold_challenge(uint32_t k, const uint8_t* accs, uint32_t m, size_t stride, const uint8_t* seed32, uint8_t rho_out[32]) {
  Blake2b h(64, "snarkv_ipa_fold1");
  uint8_t head[8];
  for (int i = 0; i < 4; ++i) head[i] = (uint8_t)(k >> (8 * i)), head[4 + i] = (uint8_t)(m >> (8 * i));
  h.update(head, sizeof head);
  h.update(accs, (size_t)m * stride);
  if (seed32) h.update(seed32, 32);
  uint8_t digest[64];
  h.digest(digest);
  Blake2bTranscript::from_uniform_bytes(digest).to_bytes(rho_out);
}

// 1 / 0 / code.  The accumulators' challenges must be canonical (as snarkv_host_pallas_ipa_decide_all demands).
int decide_all_folded(const snarkv_host_pallas_ipa_dk* dk, const uint8_t* accs, uint32_t m, const uint8_t* seed32,
                      uint8_t* ok_out) {
  if (m == 0) return 1;  // decide_all of nothing is Ok(()) (decider.rs:57-66)
  const size_t k = dk->dk.svk.k, stride = acc_stride(dk);
  std::vector<uint8_t> xi((size_t)m * k * 32), u((size_t)m * 64);
  for (uint32_t a = 0; a < m; ++a) {
    for (size_t j = 0; j < k; ++j) {
      Fr x;
      if (!Fr::from_bytes(accs + a * stride + 32 * j, &x))
        return fail(SNARKV_HOST_ERR_PANIC, "panic: non-canonical challenge in an accumulator");
    }
    memcpy(&xi[(size_t)a * k * 32], accs + a * stride, k * 32);
    memcpy(&u[(size_t)a * 64], accs + a * stride + 32 * k, 64);
  }
  uint8_t rho[32];
  fold_challenge((uint32_t)k, accs, m, stride, seed32, rho);
  int all_ok = 0;
  try {
    if (pallas_ipa_decide_folded(dk->dk.handle(), xi.data(), u.data(), m, rho, &all_ok) != SNARKV_OK)
      return fail(SNARKV_HOST_ERR_DEVICE, std::string("pallas_ipa_decide_folded: ") + snarkv_pallas_last_error());
  } catch (const std::exception& e) {
    return fail(SNARKV_HOST_ERR_DEVICE, e.what());
  }
  if (all_ok) {
    if (ok_out) memset(ok_out, 1, m);
    return 1;
  }
  if (!ok_out) return fail(0, "sum rho^i U_i == commit(G, sum rho^i h_i)");
  const int rc = snarkv_host_pallas_ipa_decide_all(dk, accs, m, ok_out);  // who it was
  if (rc < 0) return fail(rc, snarkv_host_pallas_last_error());
  if (rc == 0) return fail(0, snarkv_host_pallas_last_error());
  return rc;
}
}  // namespace

extern "C" {

const char* snarkv_host_pallas_fold_last_error(void) { return g_fold_error.c_str(); }

int snarkv_host_pallas_ipa_fold_challenge(const snarkv_host_pallas_ipa_dk* dk, const uint8_t* accs, uint32_t m,
                                          const uint8_t* seed32_or_null, uint8_t rho_out[32]) {
  if (!dk || !rho_out || (m && !accs)) return fail(SNARKV_HOST_ERR_ARG, "null argument");
  fold_challenge((uint32_t)dk->dk.svk.k, accs, m, acc_stride(dk), seed32_or_null, rho_out);
  return 1;
}

int snarkv_host_pallas_ipa_decide_all_folded(const snarkv_host_pallas_ipa_dk* dk, const uint8_t* accs, uint32_t m,
                                             const uint8_t* seed32_or_null, uint8_t* ok_out) {
  if (!dk || (m && !accs)) return fail(SNARKV_HOST_ERR_ARG, "null argument");
  return decide_all_folded(dk, accs, m, seed32_or_null, ok_out);
}

int snarkv_host_pallas_plonk_verify_folded(const snarkv_host_pallas_protocol* protocol, const snarkv_host_pallas_ipa_dk* dk,
                                           const uint8_t* instances, size_t instances_len, const uint8_t* proofs,
                                           size_t proofs_len, uint32_t n, unsigned host_threads, int decompress,
                                           const uint8_t* seed32_or_null) {
  if (decompress < SNARKV_HOST_PALLAS_DECOMPRESS_HOST || decompress > SNARKV_HOST_PALLAS_DECOMPRESS_AUTO)
    return fail(SNARKV_HOST_ERR_ARG, "unknown decompress route");
  if (!protocol || !dk || (n && (!instances || !proofs))) return fail(SNARKV_HOST_ERR_ARG, "null argument");
  std::vector<uint8_t> accs((size_t)n * acc_stride(dk) + 1);
  const int rc = snarkv_host_pallas_plonk_succinct_verify_batch(protocol, dk, instances, instances_len, proofs, proofs_len, n,
                                                                host_threads, decompress, accs.data(), accs.size());
  if (rc != 1) return fail(rc, snarkv_host_pallas_last_error());
  return decide_all_folded(dk, accs.data(), n, seed32_or_null, nullptr);
}

}  // extern "C"
