// Host build of the friendly-multiple products of fq29.h and of the fast adders of g1_29.h run on them, raw limb records in
// and out (tests/fq29_fm_model.py has the table).  Compiled per curve like hosttest_curve.cpp.  Test infrastructure only.
#include <stdint.h>
#include "../../snark-verifier_amd/csrc/g1_29.h"

using namespace snarkv;

namespace {
Fq29 ldq(const int32_t* p) {
  Fq29 r;
  for (int i = 0; i < 9; ++i) r.v[i] = p[i];
  return r;
}
void stq(const Fq29& a, int32_t* p) {
  for (int i = 0; i < 9; ++i) p[i] = a.v[i];
}
G1Xyzz29 ldx(const int32_t* p) {
  G1Xyzz29 r;
  r.x = ldq(p), r.y = ldq(p + 9), r.zz = ldq(p + 18), r.zzz = ldq(p + 27);
  return r;
}
void stx(const G1Xyzz29& a, int32_t* p) { stq(a.x, p), stq(a.y, p + 9), stq(a.zz, p + 18), stq(a.zzz, p + 27); }
G1Affine29 lda(const int32_t* p) {
  G1Affine29 r;
  r.x = ldq(p), r.y = ldq(p + 9);
  return r;
}

void op_fq29_mul_fm(const int32_t* in, int32_t* out) { stq(fq29_mul_fm(ldq(in), ldq(in + 9)), out); }
void op_fq29_sqr_fm(const int32_t* in, int32_t* out) { stq(fq29_sqr_fm(ldq(in)), out); }
void op_fq29_mul2_fm(const int32_t* in, int32_t* out) {
  stq(fq29_mul2_fm(ldq(in), ldq(in + 9), ldq(in + 18), ldq(in + 27)), out);
}
void op_xyzz29_madd_fast_fm(const int32_t* in, int32_t* out) {
  G1Xyzz29 acc = ldx(in);
  xyzz29_madd_fast_fm(acc, lda(in + 36));
  stx(acc, out);
}
void op_xyzz29_add_fast_fm(const int32_t* in, int32_t* out) {
  G1Xyzz29 acc = ldx(in);
  xyzz29_add_fast_fm(acc, ldx(in + 36));
  stx(acc, out);
}
void op_xyzz29_add_skipid_fast_fm(const int32_t* in, int32_t* out) {
  G1Xyzz29 acc = ldx(in);
  bool bad = in[72] != 0;
  xyzz29_add_skipid_fast_fm(acc, ldx(in + 36), bad);
  stx(acc, out);
  out[36] = bad ? 1 : 0;
}
// the pinned adders on the same records, for the comparison as points
void op_xyzz29_madd_fast(const int32_t* in, int32_t* out) {
  G1Xyzz29 acc = ldx(in);
  xyzz29_madd_fast(acc, lda(in + 36));
  stx(acc, out);
}
void op_xyzz29_add_fast(const int32_t* in, int32_t* out) {
  G1Xyzz29 acc = ldx(in);
  xyzz29_add_fast(acc, ldx(in + 36));
  stx(acc, out);
}
}  // namespace

extern "C" {
const char* hf_curve() { return SNARKV_CURVE_NAME; }
#define HF_RAW(name, IN, OUT)                                                                      \
  void hf_##name(const int32_t* in, int32_t* out, int n) {                                         \
    for (int i = 0; i < n; ++i) op_##name(in + (long)i * IN, out + (long)i * OUT);                 \
  }                                                                                                \
  int hf_##name##_io() { return (IN << 16) | OUT; }
HF_RAW(fq29_mul_fm, 18, 9)
HF_RAW(fq29_sqr_fm, 9, 9)
HF_RAW(fq29_mul2_fm, 36, 9)
HF_RAW(xyzz29_madd_fast_fm, 54, 36)
HF_RAW(xyzz29_add_fast_fm, 72, 36)
HF_RAW(xyzz29_add_skipid_fast_fm, 73, 37)
HF_RAW(xyzz29_madd_fast, 54, 36)
HF_RAW(xyzz29_add_fast, 72, 36)
#undef HF_RAW
// record i: an accumulator and an affine point; the point is added n times IN A ROW onto the accumulator of record 0 -- a
// chain: out[i] is the accumulator after records 0 .. i
void hf_madd_chain_fm(const int32_t* in, int32_t* out, int n) {
  G1Xyzz29 acc = ldx(in);
  for (int i = 0; i < n; ++i) {
    xyzz29_madd_fast_fm(acc, lda(in + (long)i * 54 + 36));
    stx(acc, out + (long)i * 36);
  }
}
int hf_madd_chain_fm_io() { return (54 << 16) | 36; }
}
