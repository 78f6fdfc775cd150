// Host build of the Blake2b transcript the device compiles (snark-verifier_amd/csrc/blake2b_dev.h): the hash, the reduction of
// a digest mod r, point compression and the transcript operations, raw bytes in and out.  One library per curve
// (-DSNARKV_CURVE_PALLAS), built by tests/test_blake2b_model.py.  With -DHB_MAIN the file is a stand-alone program that runs
// the same hooks over block boundaries against the RFC 7693 test vector (for a sanitizer build).  Test infrastructure only.
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include "../../snark-verifier_amd/csrc/blake2b_dev.h"

using namespace snarkv;

extern "C" {

const char* hb_curve() {
#if defined(SNARKV_CURVE_PALLAS)
  return "pallas";
#else
  return "bn254";
#endif
}

int hb_state_bytes() { return (int)sizeof(Blake2bState); }

// BLAKE2b-512 with the transcript's personalisation over msg[0..cut) then msg[cut..len): two updates, one digest
void hb_digest_split(const uint8_t* msg, size_t len, size_t cut, uint8_t out[64]) {
  Blake2bState s;
  tr_init(s);
  b2b_update(s, msg, cut);
  b2b_update(s, msg + cut, len - cut);
  uint64_t d[8];
  b2b_digest(s, d);
  memcpy(out, d, 64);
}

// the same hash with a personalisation of the caller's (16 bytes)
void hb_digest_person(const uint8_t person[16], const uint8_t* msg, size_t len, uint8_t out[64]) {
  Blake2bState s;
  b2b_init(s, person);
  b2b_update(s, msg, len);
  uint64_t d[8];
  b2b_digest(s, d);
  memcpy(out, d, 64);
}

// from_uniform_bytes: a 64-byte digest -> the canonical scalar
void hb_reduce(const uint8_t digest[64], uint8_t out[32]) {
  uint64_t d[8];
  memcpy(d, digest, 64);
  uint32_t w[8];
  fr29_to_canonical(fr_from_uniform(d), w);
  memcpy(out, w, 32);
}

void hb_compress_point(const uint8_t x[32], const uint8_t y[32], uint8_t out[32]) { tr_compress_point(x, y, out); }

// a transcript in caller-owned memory of hb_state_bytes() bytes
void hb_tr_init(void* st) { tr_init(*(Blake2bState*)st); }
void hb_tr_update(void* st, const uint8_t* in, size_t len) { b2b_update(*(Blake2bState*)st, in, len); }
int hb_tr_common_point(void* st, const uint8_t x[32], const uint8_t y[32]) {
  return tr_common_point(*(Blake2bState*)st, x, y) ? 1 : 0;
}
void hb_tr_common_scalar(void* st, const uint8_t s32[32]) { tr_common_scalar(*(Blake2bState*)st, s32); }
void hb_tr_squeeze(void* st, uint8_t out[32]) {
  uint32_t w[8];
  (void)tr_squeeze(*(Blake2bState*)st, w);
  memcpy(out, w, 32);
}
// what k_ipa_transcript_round does with L | R: one message of two points and the challenge's prefix, one update, the challenge
int hb_tr_round(void* st, const uint8_t lr[128], uint8_t proof64[64], uint8_t xi[32]) {
  uint8_t msg[2 * kTrPointBytes + kTrSqueezeBytes];
  bool ok = tr_put_point(msg, lr, lr + 32);
  ok = tr_put_point(msg + kTrPointBytes, lr + 64, lr + 96) && ok;
  tr_put_squeeze(msg + 2 * kTrPointBytes);
  tr_compress_point(lr, lr + 32, proof64);
  tr_compress_point(lr + 64, lr + 96, proof64 + 32);
  b2b_update(*(Blake2bState*)st, msg, sizeof(msg));
  uint32_t w[8];
  (void)tr_challenge(*(Blake2bState*)st, w);
  memcpy(xi, w, 32);
  return ok ? 1 : 0;
}

}  // extern "C"

#if defined(HB_MAIN)
int main() {
  // RFC 7693 appendix A: BLAKE2b-512("abc"), no personalisation
  static const uint8_t want[64] = {
      0xba, 0x80, 0xa5, 0x3f, 0x98, 0x1c, 0x4d, 0x0d, 0x6a, 0x27, 0x97, 0xb6, 0x9f, 0x12, 0xf6, 0xe9, 0x4c, 0x21, 0x2f, 0x14, 0x68, 0x5a,
      0xc4, 0xb7, 0x4b, 0x12, 0xbb, 0x6f, 0xdb, 0xff, 0xa2, 0xd1, 0x7d, 0x87, 0xc5, 0x39, 0x2a, 0xab, 0x79, 0x2d, 0xc2, 0x52, 0xd5, 0xde,
      0x45, 0x33, 0xcc, 0x95, 0x18, 0xd3, 0x8a, 0xa8, 0xdb, 0xf1, 0x92, 0x5a, 0xb9, 0x23, 0x86, 0xed, 0xd4, 0x00, 0x99, 0x23};
  const uint8_t zero16[16] = {0};
  uint8_t out[64];
  hb_digest_person(zero16, (const uint8_t*)"abc", 3, out);
  if (memcmp(out, want, 64) != 0) {
    printf("RFC 7693 vector: mismatch\n");
    return 1;
  }
  // every length and every split across three blocks: one-shot and split digests agree
  uint8_t msg[300];
  for (int i = 0; i < 300; ++i) msg[i] = (uint8_t)(i * 131 + 7);
  for (size_t len = 0; len <= 300; ++len) {
    uint8_t a[64], b[64];
    hb_digest_split(msg, len, 0, a);
    for (size_t cut = 0; cut <= len; ++cut) {
      hb_digest_split(msg, len, cut, b);
      if (memcmp(a, b, 64) != 0) {
        printf("split %zu of %zu: mismatch\n", cut, len);
        return 1;
      }
    }
  }
  // the transcript operations at every offset of a block
  for (size_t pre = 0; pre <= 130; ++pre) {
    Blake2bState s;
    hb_tr_init(&s);
    hb_tr_update(&s, msg, pre);
    uint8_t xi[32], proof[64], dig[64], sq[32];
    if (!hb_tr_round(&s, msg + 1, proof, xi)) return 1;
    hb_tr_common_scalar(&s, xi);
    hb_tr_squeeze(&s, sq);
    memset(dig, 0xff, 64);
    hb_reduce(dig, xi);
  }
  uint8_t z64[64] = {0};
  Blake2bState s;
  hb_tr_init(&s);
  if (hb_tr_common_point(&s, z64, z64 + 32)) {
    printf("the identity was absorbed\n");
    return 1;
  }
  printf("blake2b host checks ok (%s)\n", hb_curve());
  return 0;
}
#endif
