// Host build of the recoder of the shared-key MSM (snark-verifier_amd/csrc/msm_shared.h, the SNARKV_HD source the device
// compiles) as a raw-record function in the style of curve_ops.h: n records of 8 words in, 33 words out (the 32 signed
// 8-bit digits of the value's residue below r, low to high, then the carry out of the top window).  One library per curve
// (-DSNARKV_CURVE_PALLAS), built by tests/test_shared_msm_model.py.  Test infrastructure only.
#include <stdint.h>
#include "../../snark-verifier_amd/csrc/msm_shared.h"

using namespace snarkv;

extern "C" {

const char* hs_curve() {
#if defined(SNARKV_CURVE_PALLAS)
  return "pallas";
#else
  return "bn254";
#endif
}

int hs_shared_recode_raw_io() { return (8 << 16) | (kSharedW + 1); }

void hs_shared_recode_raw(const int32_t* in, int32_t* out, int n) {
  for (int i = 0; i < n; ++i) {
    uint32_t s[8];
    for (int j = 0; j < 8; ++j) s[j] = (uint32_t)in[(long)i * 8 + j];
    shared_reduce_mod_r(s);
    int32_t* o = out + (long)i * (kSharedW + 1);
    o[kSharedW] = (int32_t)shared_recode_each(s, [&](int w, int d) { o[w] = d; });
  }
}

}  // extern "C"
