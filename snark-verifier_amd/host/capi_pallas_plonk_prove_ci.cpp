// The PLONK prover session on pallas with committed instances -> libsnarkv_host_pallas_plonk_prove_ci.so
// (include/snarkv_host_pallas_plonk_prove_ci.h): capi_pallas_plonk_prove.cpp's text under the _ci_ names, with plan_prover's
// committed-instances option on.  The old entries keep their refusals; a protocol without an instance_committing_key behaves
// here, byte for byte, as under them.
#include "../../include/snarkv_host_pallas_plonk_prove_ci.h"
#define PROVER_T snarkv_host_pallas_plonk_ci_prover
#define PROVER_FN(name) snarkv_host_pallas_plonk_ci_prover_##name
#define PROVER_CI true
#include "capi_pallas_plonk_prove.cpp"
