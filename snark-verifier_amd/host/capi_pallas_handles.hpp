// The handles behind include/snarkv_host_pallas.h, shared by the units that implement its C ABI (capi_pallas.cpp) and the
// folded decide on top of it (capi_pallas_fold.cpp -> libsnarkv_host_pallas_fold.so): both see one definition.
#pragma once
#ifndef SNARKV_HOST_PALLAS
#error "compile with -DSNARKV_HOST_PALLAS"
#endif
#include "ipa.hpp"
#include "plonk.hpp"

struct snarkv_host_pallas_protocol {
  snarkv_host::PlonkProtocol pr;
};
struct snarkv_host_pallas_ipa_dk {
  snarkv_host::IpaDecidingKey dk;
};
