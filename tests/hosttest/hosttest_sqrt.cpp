// Host build of csrc/fq29_sqrt.h (-DSNARKV_CURVE_PALLAS): the square root in Fp and the per-point body of the
// decompression kernel, byte interfaces.  Compiled by tests/test_pallas_sqrt_host.py.  Test infrastructure only.
#include <string.h>
#include "../../snark-verifier_amd/csrc/fq29_sqrt.h"

using namespace snarkv;

extern "C" {
const char* hs_curve() { return SNARKV_CURVE_NAME; }

// a (32 bytes canonical) -> 1 and a root, or 0 for a non-square
int hs_fq_sqrt(const uint8_t* a32, uint8_t* root32) {
  uint32_t w[8];
  memcpy(w, a32, 32);
  const Fq29Sqrt s = fq29_sqrt(fq29_norm(fq29_from_canonical(w)));
  fq29_to_canonical(s.root, w);
  memcpy(root32, w, 32);
  return (int)s.is_square;
}

void hs_g1_decompress(const uint8_t* in32, size_t n, int mont, uint8_t* out64, uint8_t* ok) {
  for (size_t i = 0; i < n; ++i) {
    uint32_t w[8], o[16];
    memcpy(w, in32 + 32 * i, 32);
    ok[i] = g1_decompress_words(w, mont != 0, o) ? 1 : 0;
    memcpy(out64 + 64 * i, o, 64);
  }
}
}
