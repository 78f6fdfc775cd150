// Host build of the argument checks that the entry points of the resident-polynomial units share
// (snark-verifier_amd/csrc/poly_args.hpp), one call per check, addresses as integers: nothing is ever followed.  One library
// per curve (-DSNARKV_CURVE_PALLAS, for below_r), built by snark-verifier_amd/build.py; tests/test_poly_args_model.py compares
// it with Python integers.  har_selftest runs the edge cases of that test on constants, so that the same source is a
// stand-alone program for the host sanitizers:
//   g++ -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=all -DHOSTTEST_ARGS_MAIN hosttest_args.cpp && ./a.out
// Test infrastructure only.
#include <stdarg.h>
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include "../../snark-verifier_amd/csrc/poly_args.hpp"

namespace snarkv {

static char g_error[256];

void set_last_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_error, sizeof g_error, fmt, ap);
  va_end(ap);
}

}  // namespace snarkv

using namespace snarkv;

static const void* at(uint64_t a) { return (const void*)(uintptr_t)a; }

extern "C" {

const char* har_curve() {
#if defined(SNARKV_CURVE_PALLAS)
  return "pallas";
#else
  return "bn254";
#endif
}

const char* har_last_error() { return g_error; }
void har_clear_error() { g_error[0] = 0; }

int har_overlap(uint64_t a, uint64_t an, uint64_t b, uint64_t bn) { return overlap(at(a), an, at(b), bn); }
int har_partial_overlap(uint64_t a, uint64_t b, uint64_t bytes) { return partial_overlap(at(a), at(b), bytes); }
int har_aligned16(uint64_t a) { return aligned16(at(a)); }
uint64_t har_bytes_of(uint64_t n) { return bytes_of(n); }
int har_check_len(uint64_t n, uint64_t max_len) { return check_len(n, max_len); }
int har_below_r(const uint8_t* s32) { return below_r(s32); }
int har_all_below_r(const uint8_t* s32, uint64_t count) { return all_below_r(s32, count); }
int har_is_zero32(const uint8_t* s32) { return is_zero32(s32); }
int har_refuse_overlap(const char* call, const char* what) { return refuse_overlap(call, what); }

// idx: n_idx arrays of `count` indices, one after the other; none_ok: one byte per array; outs, out_bytes: n_outs each
int har_check_columns(uint64_t polys, uint64_t n, uint64_t n_polys, const uint32_t* idx, uint64_t n_idx, const uint8_t* none_ok,
                      uint64_t count, const uint64_t* outs, const uint64_t* out_bytes, uint64_t n_outs) {
  enum { kMax = 8 };
  if (n_idx > kMax || n_outs > kMax) return 1;  // no code of the header
  const uint32_t* arrays[kMax];
  bool ok[kMax];
  const void* o[kMax];
  size_t ob[kMax];
  for (size_t a = 0; a < n_idx; ++a) arrays[a] = idx + a * count, ok[a] = none_ok[a] != 0;
  for (size_t i = 0; i < n_outs; ++i) o[i] = at(outs[i]), ob[i] = out_bytes[i];
  return check_columns("hosttest", at(polys), n, n_polys, arrays, n_idx, ok, count, o, ob, n_outs);
}

// the edge cases of tests/test_poly_args_model.py on constants: 0, or the line of the first one that fails
int har_selftest() {
#define EXPECT(cond) \
  if (!(cond)) return __LINE__
  const uint64_t top = ~(uint64_t)0;  // 2^64 - 1
  // overlap: empty ranges, adjacent, nested, identical
  EXPECT(!har_overlap(0x1000, 0, 0x1000, 32) && !har_overlap(0x1000, 32, 0x1000, 0) && !har_overlap(0x1000, 0, 0x1000, 0));
  EXPECT(har_overlap(0x1000, 1, 0x1000, 1) && !har_overlap(0x1000, 1, 0x1001, 1) && !har_overlap(0x1001, 1, 0x1000, 1));
  EXPECT(!har_overlap(0x1000, 32, 0x1020, 32) && har_overlap(0x1000, 33, 0x1020, 32) && !har_overlap(0x1020, 32, 0x1000, 32));
  EXPECT(har_overlap(0x1000, 64, 0x1010, 16) && har_overlap(0x1010, 16, 0x1000, 64) && har_overlap(0x1000, 64, 0x1000, 64));
  // ... and next to 2^64, where a sum of address and length wraps: [2^64 - 32, 2^64) against ranges far below
  EXPECT(!har_overlap(top - 31, 32, 0x1000, 32) && !har_overlap(0x1000, 32, top - 31, 32));
  EXPECT(!har_overlap(top - 63, 32, top - 31, 32) && har_overlap(top - 63, 33, top - 31, 32) && har_overlap(top - 31, 32, top - 15, 16));
  EXPECT(!har_overlap(top, 1, 0, 1) && !har_overlap(0, 1, top, 1) && har_overlap(top, 1, top, 1));
  EXPECT(!har_partial_overlap(0x1000, 0x1000, 64) && har_partial_overlap(0x1000, 0x1020, 64) && !har_partial_overlap(0x1000, 0x1040, 64));
  EXPECT(!har_aligned16(0) && har_aligned16(0x1000) && !har_aligned16(0x1008) && har_aligned16(top - 15));
  // bytes_of saturates above 2^40 elements
  EXPECT(har_bytes_of(0) == 0 && har_bytes_of(1) == 32 && har_bytes_of((uint64_t)1 << 40) == (uint64_t)1 << 45);
  EXPECT(har_bytes_of(((uint64_t)1 << 40) + 1) == (uint64_t)1 << 45 && har_bytes_of((uint64_t)1 << 63) == (uint64_t)1 << 45);
  EXPECT(har_check_len(0, 8) == SNARKV_ERR_EMPTY && har_check_len(8, 8) == SNARKV_OK && har_check_len(9, 8) == SNARKV_ERR_LENGTH);
  // below_r at 0, r - 1, r, r + 1, 2^256 - 1
  constexpr uint32_t rw[8] = SNARKV_FR_R_LIMBS;
  uint8_t s[5][32];
  memset(s[0], 0, 32);
  memcpy(s[2], rw, 32);
  memcpy(s[1], rw, 32), s[1][0] -= 1;  // r is odd: no borrow
  memcpy(s[3], rw, 32), s[3][0] += 1;  // ... and r + 1 has no carry
  memset(s[4], 0xFF, 32);
  EXPECT((rw[0] & 1u) && (rw[0] & 0xFFu) != 0xFFu);
  EXPECT(har_below_r(s[0]) && har_below_r(s[1]) && !har_below_r(s[2]) && !har_below_r(s[3]) && !har_below_r(s[4]));
  EXPECT(har_all_below_r(s[0], 2) && !har_all_below_r(s[0], 3) && har_all_below_r(s[2], 0));
  EXPECT(har_is_zero32(s[0]) && !har_is_zero32(s[1]) && !har_is_zero32(s[4]));
  EXPECT(har_refuse_overlap("call", "what") == SNARKV_ERR_ARG && !strcmp(har_last_error(), "call: overlap: what"));
  // check_columns: three columns of n = 4 at 0x10000, one output of a column's size
  const uint64_t polys = 0x10000, n = 4, col = 32 * n, far = 0x80000;
  const uint8_t strict[2] = {0, 0}, lax[2] = {0, 1};
  const uint32_t ok_idx[4] = {0, 1, 2, 0}, past[4] = {0, 1, 3, 0}, none[4] = {0, 1, 0, SNARKV_POLY_NONE}, two[4] = {0, 1, 0, 1};
  uint64_t out[1] = {far}, bytes[1] = {col};
  EXPECT(har_check_columns(polys, n, 3, ok_idx, 2, strict, 2, out, bytes, 1) == SNARKV_OK);
  har_clear_error();
  EXPECT(har_check_columns(polys, n, 3, past, 2, strict, 2, out, bytes, 1) == SNARKV_ERR_ARG && strstr(har_last_error(), "index 3"));
  EXPECT(har_check_columns(polys, n, 3, none, 2, lax, 2, out, bytes, 1) == SNARKV_OK);
  EXPECT(har_check_columns(polys, n, 3, none, 2, strict, 2, out, bytes, 1) == SNARKV_ERR_ARG && strstr(har_last_error(), "index"));
  EXPECT(har_check_columns(polys, n, 0, past, 2, strict, 2, out, bytes, 1) == SNARKV_OK);  // no columns: nothing to index
  // an output that touches only the last 32 bytes of column 1: refused when the column is named, not otherwise
  out[0] = polys + 2 * col - 32, bytes[0] = 32;
  har_clear_error();
  EXPECT(har_check_columns(polys, n, 3, two, 2, strict, 2, out, bytes, 1) == SNARKV_ERR_ARG && strstr(har_last_error(), "overlap"));
  const uint32_t others[4] = {0, 2, 2, 0};
  EXPECT(har_check_columns(polys, n, 3, others, 2, strict, 2, out, bytes, 1) == SNARKV_OK);
  out[0] = polys + 2 * col;  // the first byte after it
  EXPECT(har_check_columns(polys, n, 3, two, 2, strict, 2, out, bytes, 1) == SNARKV_OK);
  return 0;
#undef EXPECT
}

}  // extern "C"

#if defined(HOSTTEST_ARGS_MAIN)
int main() {
  const int line = har_selftest();
  if (line) printf("hosttest_args (%s): the check at line %d fails\n", har_curve(), line);
  else printf("hosttest_args (%s): ok\n", har_curve());
  return line ? 1 : 0;
}
#endif
