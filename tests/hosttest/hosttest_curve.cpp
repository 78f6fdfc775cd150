// Host build of the CURVE-GENERIC device headers (fq29.h, fr29.h, g1_29.h, glv.h), compiled twice
// by tests/conftest.py: default (BN254) and -DSNARKV_CURVE_PALLAS.  Test infrastructure only.
#include <string.h>
#include "../../snark-verifier_amd/csrc/fr29.h"
#include "../../snark-verifier_amd/csrc/g1_29.h"
#include "../../snark-verifier_amd/csrc/glv.h"
#include "curve_ops.h"
#if !defined(SNARKV_CURVE_PALLAS)
#include <algorithm>
#include <set>
#include <utility>
#include "../../snark-verifier_amd/csrc/decide_sched.hpp"
#include "../../snark-verifier_amd/csrc/round_emul.h"
#endif

using namespace snarkv;

static Fq29 ld(const uint8_t* b) {
  uint32_t w[8];
  memcpy(w, b, 32);
  return fq29_from_canonical(w);
}
static void st(const Fq29& a, uint8_t* b) {
  uint32_t w[8];
  fq29_to_canonical(a, w);
  memcpy(b, w, 32);
}
static G1Affine29 ldp(const uint8_t* b) {
  uint32_t w[16];
  memcpy(w, b, 64);
  return g1a29_from_canonical(w);
}
static void stp(const G1Xyzz29& p, uint8_t* out) {
  uint32_t w[16];
  g1a29_to_canonical(xyzz29_to_affine(p), w);
  memcpy(out, w, 64);
}

extern "C" {
const char* hc_curve() { return SNARKV_CURVE_NAME; }
void hc_fq_mul(const uint8_t* a, const uint8_t* b, uint8_t* o) { st(fq29_mul(ld(a), ld(b)), o); }
void hc_fq_sqr(const uint8_t* a, uint8_t* o) { st(fq29_sqr(ld(a)), o); }
void hc_fq_mul2(const uint8_t* a, const uint8_t* b, const uint8_t* c, const uint8_t* d, uint8_t* o) {
  st(fq29_mul2(ld(a), ld(b), fq29_neg(ld(c)), ld(d)), o);  // a b - c d
}
void hc_fq_inv(const uint8_t* a, uint8_t* o) { st(fq29_inv(ld(a)), o); }
void hc_fr_mul(const uint8_t* a, const uint8_t* b, uint8_t* o) {
  uint32_t x[8], y[8], w[8];
  memcpy(x, a, 32);
  memcpy(y, b, 32);
  fr29_to_canonical(fr29_mul(fr29_from_canonical(x), fr29_from_canonical(y)), w);
  memcpy(o, w, 32);
}
// (P + Q) careful, P + Q fast (distinct, non-special inputs), 2^n P through the Jacobian chain
void hc_g1_add(const uint8_t* p, const uint8_t* q, uint8_t* o) {
  G1Xyzz29 a = xyzz29_from_affine(ldp(p));
  xyzz29_add_careful(a, xyzz29_from_affine(ldp(q)));
  stp(a, o);
}
void hc_g1_madd_chain(const uint8_t* p, const uint8_t* qs, int n, uint8_t* o) {
  G1Xyzz29 a = xyzz29_from_affine(ldp(p));
  for (int i = 0; i < n; ++i) xyzz29_madd_fast(a, ldp(qs + 64 * i));
  stp(a, o);
}
void hc_g1_double_n(const uint8_t* p, int n, uint8_t* o) {
  G1Xyzz29 a = xyzz29_double(xyzz29_from_affine(ldp(p)));  // a non-trivial ZZ to start from
  stp(xyzz29_double_n(a, n), o);
}
void hc_glv_decompose(const uint8_t* k, uint8_t* out32) {
  uint32_t w[8], o[8];
  memcpy(w, k, 32);
  glv_decompose(w, o);
  memcpy(out32, o, 32);
}
void hc_glv_phi(const uint8_t* p, uint8_t* out) {
  G1Affine29 a = ldp(p);
  constexpr int32_t b[9] = SNARKV_GLV_BETA29_LIMBS;
  Fq29 beta;
  for (int i = 0; i < 9; ++i) beta.v[i] = b[i];
  a.x = fq29_mul(a.x, beta);
  stp(xyzz29_from_affine(a), out);
}

// raw-record entry points (curve_ops.h): n records in, n records out, limbs untouched on both sides
#define HC_RAW(name, IN, OUT)                                               \
  void hc_##name##_raw(const int32_t* in, int32_t* out, int n) {            \
    for (int i = 0; i < n; ++i) rawops::op_##name(in + (long)i * IN, out + (long)i * OUT); \
  }                                                                         \
  int hc_##name##_raw_io() { return (IN << 16) | OUT; }
SNARKV_RAW_OPS(HC_RAW)
SNARKV_RAW_DECIDER_OPS(HC_RAW)
#undef HC_RAW
#if !defined(SNARKV_CURVE_PALLAS)
// the level program of k_g2_prepare_w as the kernel reads it: 14 int8-sized fields per task widened to int32
// (dst, out, as[3], ac[3], bs[3], bc[3], conj, used); returns levels * tasks
int hc_g2w_prog(int32_t* out, int cap) {
  int n = 0;
  for (int lv = 0; lv < kG2wLevels; ++lv)
    for (int t = 0; t < kG2wTasks; ++t, ++n) {
      if (n >= cap) continue;
      const G2wTask& k = kG2wProg[lv][t];
      int32_t* o = out + 16 * n;
      o[0] = k.dst, o[1] = k.out;
      for (int j = 0; j < 3; ++j) o[2 + j] = k.as[j], o[5 + j] = k.ac[j], o[8 + j] = k.bs[j], o[11 + j] = k.bc[j];
      o[14] = k.conj, o[15] = k.used;
    }
  return n;
}
// the distinct (kind, flags) of the operations wt_build_program() emits (WT_IDLE left out), sorted; returns their number
int hc_wt_variants(int32_t* out, int cap) {
  static const WtProgram prog = wt_build_program();
  std::set<std::pair<int, int>> seen;
  for (const WtOp& o : prog.ops)
    if (o.kind != WT_IDLE) seen.insert({o.kind, o.flags});
  int n = 0;
  for (const auto& kf : seen) {
    if (n < cap) out[2 * n] = kf.first, out[2 * n + 1] = kf.second;
    ++n;
  }
  return n;
}
// The records of tests/devtest/devtest.hip k_wt_round / k_coop3_round, emulated lane by lane (csrc/round_emul.h).
// wt_round: A (24 values), B (24 values), kind, flags -> dst (24 values)
void hc_wt_round_raw(const int32_t* in, int32_t* out, int n) {
  for (int r = 0; r < n; ++r) {
    const int32_t* rec = in + (long)r * kWtRoundIn;
    Fq29P lds[72];
    memset(lds, 0, sizeof(lds));
    for (int j = 0; j < 48 * 9; ++j) lds[j / 9].v[j % 9] = rec[j];
    WtOp op;
    op.a = 0, op.b = 24, op.dst = 48, op.kind = (uint8_t)rec[432], op.flags = (uint8_t)rec[433];
    wt_round_emul(lds, lds, op);  // dst overlaps neither operand
    for (int j = 0; j < 24 * 9; ++j) out[(long)r * kWtRoundOut + j] = lds[48 + j / 9].v[j % 9];
  }
}
int hc_wt_round_raw_io() { return (kWtRoundIn << 16) | kWtRoundOut; }
// coop3_round: A, B (12 coefficients each), mode (0: B a register, 1: B a sparse line: only w^0, w^1, w^3 are read)
void hc_coop3_round_raw(const int32_t* in, int32_t* out, int n) {
  for (int r = 0; r < n; ++r) {
    const int32_t* rec = in + (long)r * kCoop3RoundIn;
    Fq29 fa[12], fb[12], fc[12];
    for (int c = 0; c < 12; ++c) fa[c] = rawops::ldq(rec + 9 * c), fb[c] = rawops::ldq(rec + 108 + 9 * c);
    if (rec[216])
      for (int c = 0; c < 12; ++c)
        if (!wt_line_has(c >> 1)) fb[c] = fq29_zero();
    coop3_round_emul(fa, fb, fc);
    for (int c = 0; c < 12; ++c) rawops::stq(fc[c], out + (long)r * kCoop3RoundOut + 9 * c);
  }
}
int hc_coop3_round_raw_io() { return (kCoop3RoundIn << 16) | kCoop3RoundOut; }
int hc_g2w_dims(int which) { return which == 0 ? kG2wLevels : which == 1 ? kG2wTasks : kG2wSlots; }
// the slots the program starts from, as g2_prepare_prog.inc names them: the six constants, Q = (QX, QY), then the running
// point T = (TX, TZ, TYA, TYB); -1 past the end
int hc_g2w_slot(int which) {
  const int s[12] = {kG2wSlotONE, kG2wSlotB3, kG2wSlotG12, kG2wSlotG13, kG2wSlotG22, kG2wSlotG23,
                     kG2wSlotQX,  kG2wSlotQY, kG2wSlotTX,  kG2wSlotTZ,  kG2wSlotTYA, kG2wSlotTYB};
  return which >= 0 && which < 12 ? s[which] : -1;
}
#endif
}
