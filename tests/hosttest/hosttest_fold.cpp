// Host build of the per-lane body and the partial sum of the folded IPA decide (snark-verifier_amd/csrc/ipa_fold.h, the
// SNARKV_HD source the device compiles), driven the way ipa_fold.hip drives it: the challenges and the powers of rho into
// the Montgomery domain, one call of the lane body per (lane, slice), the slices' partials summed per coefficient -- or,
// with a single slice, the lane's sums taken as they are.  Raw words in and out.  One library per curve
// (-DSNARKV_CURVE_PALLAS), built by tests/test_ipa_fold_model.py.  Test infrastructure only.
#include <stdint.h>
#include <vector>
#include "../../snark-verifier_amd/csrc/ipa_fold.h"

using namespace snarkv;

extern "C" {

const char* hf_curve() {
#if defined(SNARKV_CURVE_PALLAS)
  return "pallas";
#else
  return "bn254";
#endif
}

int hf_fold_block_bits() { return kFoldT; }

// xi: m x k canonical scalars (8 words each), rho: 8 words, h: 2^k x 8 words out.  1 <= slices <= m.
void hf_fold_coeffs(const uint32_t* xi, const uint32_t* rho, int m, int k, int slices, uint32_t* h) {
  const uint32_t n = 1u << k, lanes = n >> kFoldT ? n >> kFoldT : 1u;
  std::vector<Fr29> x29((size_t)m * k), pw(m), parts((size_t)slices * n);
  for (size_t i = 0; i < x29.size(); ++i) x29[i] = fr29_from_canonical(xi + 8 * i);
  Fr29 sq[32];
  sq[0] = fr29_from_canonical(rho);
  for (int b = 1; b < 32; ++b) sq[b] = fr29_mul(sq[b - 1], sq[b - 1]);
  for (int i = 0; i < m; ++i) {
    Fr29 acc = fr29_one();
    for (int b = 0; b < 32; ++b)
      if ((i >> b) & 1) acc = fr29_mul(acc, sq[b]);
    pw[i] = acc;
  }
  for (uint32_t s = 0; s < (uint32_t)slices; ++s)
    for (uint32_t lane = 0; lane < lanes; ++lane) {
      Fr29 sums[1 << kFoldT];
      ipa_fold_lane<kFoldT>(x29.data(), pw.data(), (uint32_t)k, lane, fold_slice_begin(s, slices, m),
                            fold_slice_begin(s + 1, slices, m), sums);
      for (uint32_t q = 0; q < (1u << kFoldT) && q < n; ++q) parts[(size_t)s * n + ((size_t)lane << kFoldT) + q] = sums[q];
    }
  for (uint32_t j = 0; j < n; ++j)
    fr29_to_canonical(slices == 1 ? parts[j] : fold_sum_partials(parts.data() + j, n, (uint32_t)slices), h + 8 * (size_t)j);
}

}  // extern "C"
