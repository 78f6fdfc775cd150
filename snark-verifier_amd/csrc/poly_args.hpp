// Internal: the host-side argument checks that the entry points of the resident-polynomial units share (poly.hip, ntt.hip,
// poly_prod.hip, quotient.hip, lookup.hip).  What to check and in which order is each entry point's own; what a check means
// is here.  Host only and free of HIP types, so that the host compiles it alone (tests/hosttest/hosttest_args.cpp).
// `static`: none of it is a symbol of either library.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>
#include "../../include/snarkv_poly_prod.h"
#include "curve_consts.h"

namespace snarkv {

void set_last_error(const char* fmt, ...);

// do [a, a + an) and [b, b + bn) share a byte?  Written on the distance of the two addresses: no sum that could wrap
static inline bool overlap(const void* a, size_t an, const void* b, size_t bn) {
  const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
  return an && bn && (x < y ? y - x < an : x - y < bn);
}
// ... other than being the same buffer
static inline bool partial_overlap(const void* a, const void* b, size_t bytes) { return a != b && overlap(a, bytes, b, bytes); }
static inline bool aligned16(const void* p) { return p && (uintptr_t)p % 16 == 0; }
// the bytes of n elements for the overlap checks that come before the length's: no wrap for an absurd n
static inline size_t bytes_of(size_t n) { return n > ((size_t)1 << 40) ? (size_t)1 << 45 : 32 * n; }
static inline int check_len(size_t n, size_t max_len) {
  return n == 0 ? SNARKV_ERR_EMPTY : (n > max_len ? SNARKV_ERR_LENGTH : SNARKV_OK);
}

// 32 bytes little-endian of host memory: canonical?
static inline bool below_r(const uint8_t* s32) {
  constexpr uint32_t rw[8] = SNARKV_FR_R_LIMBS;
  uint32_t w[8];
  memcpy(w, s32, 32);
  for (int i = 7; i >= 0; --i)
    if (w[i] != rw[i]) return w[i] < rw[i];
  return false;
}
static inline bool all_below_r(const uint8_t* s32, size_t count) {
  for (size_t j = 0; j < count; ++j)
    if (!below_r(s32 + 32 * j)) return false;
  return true;
}
static inline bool is_zero32(const uint8_t* s32) {
  for (int i = 0; i < 32; ++i)
    if (s32[i]) return false;
  return true;
}

static inline int refuse_overlap(const char* call, const char* what) {
  set_last_error("%s: overlap: %s", call, what);
  return SNARKV_ERR_ARG;
}

// the index and overlap checks of a call that reads the columns idx[0][j], idx[1][j], ... (SNARKV_POLY_NONE allowed where
// `none_ok`) and writes `n_outs` buffers.  Without columns (n_polys = 0) there is nothing to index: the call is empty.
static inline int check_columns(const char* call, const void* d_polys, size_t n, size_t n_polys, const uint32_t* const* idx,
                                size_t n_idx, const bool* none_ok, size_t count, const void* const* outs,
                                const size_t* out_bytes, size_t n_outs) {
  if (n_polys == 0) return SNARKV_OK;
  const size_t col = bytes_of(n);
  for (size_t a = 0; a < n_idx; ++a)
    for (size_t j = 0; j < count; ++j) {
      const uint32_t i = idx[a][j];
      if (i == SNARKV_POLY_NONE && none_ok[a]) continue;
      if (i >= n_polys) {
        set_last_error("%s: index %u at %zu, there are %zu columns", call, i, j, n_polys);
        return SNARKV_ERR_ARG;
      }
      for (size_t o = 0; o < n_outs; ++o)
        if (overlap(outs[o], out_bytes[o], (const void*)((uintptr_t)d_polys + col * i), col)) {
          set_last_error("%s: overlap: a buffer the call writes and column %u", call, i);
          return SNARKV_ERR_ARG;
        }
    }
  return SNARKV_OK;
}

}  // namespace snarkv
