// The two rounds of the pairing decider emulated lane by lane on the host: every lane's task by the device functions
// (decide_w.h, pairing_coop29.h), the DPP exchanges (group8_sum, row_ror:8) replaced by explicit sums over the lanes of a
// group.  Shared by the whole-program emulations of hosttest.cpp and by the raw-record rounds of hosttest_curve.cpp, which
// tests/devtest/devtest.hip runs with the real exchanges.  Test infrastructure only.
#pragma once
#include "decide_w.h"

namespace snarkv {

// the limb-wise (wrapping, unsigned) sum group8_sum leaves in every lane of the group
inline void emul_group_add(Fq29& s, const Fq29& v) {
  for (int q = 0; q < 9; ++q) s.v[q] = (int32_t)((uint32_t)s.v[q] + (uint32_t)v.v[q]);
}

// one duo's round of k_decide_w for `op`: both wavefront halves read `lds`, the writer lanes store into `next`
inline void wt_round_emul(const Fq29P* lds, Fq29P* next, const WtOp op) {
  for (int half = 0; half < 2; ++half) {
    Fq29 own[8];
    for (int g = 0; g < 8; ++g) {
      Fq29 s = fq29_zero();
      for (int jj = 0; jj < 8; ++jj) emul_group_add(s, wt_task(lds, op, half, 8 * g + jj));
      own[g] = wt_squeeze(s);
    }
    for (int g = 0; g < 8; ++g) wt_write(next, op, half, 8 * g, own[g], own[g ^ 1]);
  }
}

// the round of k_decide (coop_mul_b): fc = fa * fb, 96 lanes; fb's zero coefficients contribute exact zeros, which is
// what the kernel's sparse-line path leaves out
inline void coop3_round_emul(const Fq29* fa, const Fq29* fb, Fq29* fc) {
  Fq29 prod[96];
  Coop3Lane L[96];
  for (int l = 0; l < 96; ++l) {
    L[l] = coop3_lane(l);
    prod[l] = L[l].active ? coop3_product(L[l].e, fa[2 * L[l].i1], fa[2 * L[l].i1 + 1], fb[2 * L[l].i2 + L[l].e],
                                          fb[2 * L[l].i2 + 1 - L[l].e])
                          : fq29_zero();
  }
  Fq29 lo[12], hi[12];
  for (int g = 0; g < 12; ++g) {
    lo[g] = fq29_zero();
    hi[g] = fq29_zero();
    for (int j = 0; j < 8; ++j) {
      int l = 8 * g + j;  // g = 2k + e
      if (!L[l].active) continue;
      emul_group_add(L[l].high ? hi[g] : lo[g], prod[l]);
    }
  }
  for (int g = 0; g < 12; ++g) fc[g] = coop3_finalize(g & 1, lo[g], hi[g], hi[g ^ 1]);
}

}  // namespace snarkv
