// `Ipa::create_proof` in one call for the pallas product API -> libsnarkv_host_pallas_prove.so
// (include/snarkv_host_pallas_prove.h), compiled with -DSNARKV_HOST_PALLAS like capi_pallas.cpp and linked against
// libsnarkv_host_pallas.so and libsnarkv_pallas.so.  Thin: the key handle's resident device key and its h / s go to one call
// of the device library (pallas_ipa_create_proof, include/snarkv_ipa_create.h), whose transcript lives on the device.
#ifndef SNARKV_HOST_PALLAS
#error "compile with -DSNARKV_HOST_PALLAS"
#endif
#include "../../include/snarkv_host_pallas_prove.h"
#include "../../include/snarkv_ipa_create.h"

#include <cstring>
#include <string>
#include <vector>

#include "capi_pallas_handles.hpp"

using namespace snarkv_host;

namespace {
thread_local std::string g_prove_error;

int fail(int code, const std::string& what) {
  g_prove_error = what;
  return code;
}
}  // namespace

extern "C" {

const char* snarkv_host_pallas_prove_last_error(void) { return g_prove_error.c_str(); }

int snarkv_host_pallas_ipa_create_proof(const snarkv_host_pallas_ipa_dk* dk, const uint8_t* poly32, size_t n,
                                        const uint8_t z32[32], const uint8_t* omega32, const uint8_t* pbar32,
                                        const uint8_t* omega_bar32, const uint8_t* absorbed, size_t absorbed_len,
                                        uint8_t* proof_out, size_t proof_cap, size_t* proof_len, uint8_t* acc_out) {
  if (!dk || !poly32 || !z32 || !proof_out || !proof_len || !acc_out || (absorbed_len && !absorbed))
    return fail(SNARKV_HOST_ERR_ARG, "null argument");
  *proof_len = 0;
  const IpaSuccinctVerifyingKey& svk = dk->dk.svk;
  const bool zk = svk.zk();
  if (zk ? (!omega32 || !pbar32 || !omega_bar32) : (omega32 || pbar32 || omega_bar32))
    return fail(SNARKV_HOST_ERR_ARG, "omega, p_bar and omega_bar go with a zero-knowledge key, and only with one");
  const size_t k = svk.k;
  if (n != ((size_t)1 << k)) return fail(SNARKV_HOST_ERR_ARG, "poly has 2^k coefficients");
  const size_t need = 64 * k + 64 + (zk ? 64 : 0);
  if (proof_cap < need) {
    *proof_len = need;
    return fail(SNARKV_HOST_ERR_CAPACITY, "proof_cap is below the length of the proof");
  }
  Fr x;
  bool canon = Fr::from_bytes(z32, &x) && (!zk || (Fr::from_bytes(omega32, &x) && Fr::from_bytes(omega_bar32, &x)));
  for (size_t j = 0; canon && j < n; ++j) canon = Fr::from_bytes(poly32 + 32 * j, &x) && (!zk || Fr::from_bytes(pbar32 + 32 * j, &x));
  if (!canon) return fail(SNARKV_HOST_ERR_PANIC, "panic: non-canonical scalar");
  std::vector<uint8_t> xi(32 * k);
  uint8_t u[64];
  int rc;
  try {
    rc = pallas_ipa_create_proof(dk->dk.handle(), svk.h.b, zk ? svk.s->b : nullptr, poly32, n, z32, omega32, pbar32,
                                 omega_bar32, absorbed, absorbed_len, proof_out, proof_cap, proof_len, xi.data(), u);
  } catch (const std::exception& e) {
    return fail(SNARKV_HOST_ERR_DEVICE, e.what());
  }
  if (rc != SNARKV_OK) {
    const std::string what = std::string("pallas_ipa_create_proof: ") + snarkv_pallas_last_error();
    return fail(rc == SNARKV_ERR_ENCODING ? SNARKV_HOST_ERR_TRANSCRIPT : SNARKV_HOST_ERR_DEVICE, what);
  }
  memcpy(acc_out, xi.data(), xi.size());
  memcpy(acc_out + xi.size(), u, 64);
  return 1;
}

}  // extern "C"
