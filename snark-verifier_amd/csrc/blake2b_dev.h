// halo2's Blake2b transcript (`Blake2bWrite` with `Challenge255`) for the device and the host, from RFC 7693 and the
// transcript definition at the top of host/blake2b_transcript.hpp:
//   state    BLAKE2b-512, unkeyed, personalisation "Halo2-Transcript"
//   prefix   0x00 before a challenge, 0x01 before a point (x | y, 32 bytes little-endian each), 0x02 before a scalar
//   squeeze  digest of a COPY of the state, read as a 512-bit little-endian integer, reduced mod r (`from_uniform_bytes`)
//   points   travel compressed: x with the parity of y in bit 255; the identity is never written
// Same source for the kernels of ipa_opening.hip and for the host (tests/hosttest/hosttest_blake2b.cpp, and the host side of
// snarkv_ipa_create_proof, which hashes the caller's prefix with it), as ipa_fold.h.
//
// The state is meant to live in memory (device global memory between launches): `buf` is written byte by byte at the
// run-time index `fill`, which a register array could not take without going to scratch.  What must stay in registers is the
// compression's m[16] and v[16]: both loops of b2b_compress are fully unrolled and the sigma table is constexpr, so every
// index is a constant when the code is generated.  Each inlined b2b_update / b2b_digest carries one copy of the compression
// (about 2 700 instructions): a kernel collects what it absorbs in one message (tr_put_*) and calls b2b_update once.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include "fr29.h"

namespace snarkv {

struct Blake2bState {
  uint64_t h[8];
  uint64_t t;        // bytes compressed so far, the buffered ones not counted (64 bits: v[13] stays IV[5])
  uint64_t buf[16];  // one block, little-endian words; bytes [0, fill) are pending
  uint32_t fill;
  uint32_t pad_;
};

SNARKV_HD uint64_t b2b_iv(int i) {
  constexpr uint64_t iv[8] = {0x6a09e667f3bcc908ull, 0xbb67ae8584caa73bull, 0x3c6ef372fe94f82bull, 0xa54ff53a5f1d36f1ull,
                              0x510e527fade682d1ull, 0x9b05688c2b3e6c1full, 0x1f83d9abfb41bd6bull, 0x5be0cd19137e2179ull};
  return iv[i];
}
// by 32 a register swap; by 24, 16, 63 two v_alignbit_b32 on the vector unit, or s_lshr_b64 | s_lshl_b64 where the work is
// uniform (the transcript kernels: one lane, addresses from kernel arguments -- the compiler keeps the whole hash in SGPRs)
SNARKV_HD uint64_t b2b_rotr(uint64_t x, int n) { return (x >> n) | (x << (64 - n)); }

// h <- F(h, m, t, last), RFC 7693 section 3.2
SNARKV_HD void b2b_compress(uint64_t (&h)[8], const uint64_t (&m)[16], uint64_t t, bool last) {
  constexpr uint8_t sigma[12][16] = {
      {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15}, {14, 10, 4, 8, 9, 15, 13, 6, 1, 12, 0, 2, 11, 7, 5, 3},
      {11, 8, 12, 0, 5, 2, 15, 13, 10, 14, 3, 6, 7, 1, 9, 4}, {7, 9, 3, 1, 13, 12, 11, 14, 2, 6, 5, 10, 4, 0, 15, 8},
      {9, 0, 5, 7, 2, 4, 10, 15, 14, 1, 11, 12, 6, 8, 3, 13}, {2, 12, 6, 10, 0, 11, 8, 3, 4, 13, 7, 5, 15, 14, 1, 9},
      {12, 5, 1, 15, 14, 13, 4, 10, 0, 7, 6, 3, 9, 2, 8, 11}, {13, 11, 7, 14, 12, 1, 3, 9, 5, 0, 15, 4, 8, 6, 2, 10},
      {6, 15, 14, 9, 11, 3, 0, 8, 12, 2, 13, 7, 1, 4, 10, 5}, {10, 2, 8, 4, 7, 6, 1, 5, 15, 11, 9, 14, 3, 12, 13, 0},
      {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15}, {14, 10, 4, 8, 9, 15, 13, 6, 1, 12, 0, 2, 11, 7, 5, 3}};
  constexpr uint8_t mix[8][4] = {{0, 4, 8, 12}, {1, 5, 9, 13}, {2, 6, 10, 14}, {3, 7, 11, 15},
                                 {0, 5, 10, 15}, {1, 6, 11, 12}, {2, 7, 8, 13}, {3, 4, 9, 14}};
  uint64_t v[16];
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    v[i] = h[i];
    v[8 + i] = b2b_iv(i);
  }
  v[12] ^= t;
  if (last) v[14] = ~v[14];
#pragma unroll
  for (int r = 0; r < 12; ++r) {
#pragma unroll
    for (int g = 0; g < 8; ++g) {
      uint64_t a = v[mix[g][0]], b = v[mix[g][1]], c = v[mix[g][2]], d = v[mix[g][3]];
      a = a + b + m[sigma[r][2 * g]];
      d = b2b_rotr(d ^ a, 32);
      c = c + d;
      b = b2b_rotr(b ^ c, 24);
      a = a + b + m[sigma[r][2 * g + 1]];
      d = b2b_rotr(d ^ a, 16);
      c = c + d;
      b = b2b_rotr(b ^ c, 63);
      v[mix[g][0]] = a;
      v[mix[g][1]] = b;
      v[mix[g][2]] = c;
      v[mix[g][3]] = d;
    }
  }
#pragma unroll
  for (int i = 0; i < 8; ++i) h[i] ^= v[i] ^ v[8 + i];
}

// BLAKE2b-512, no key, personalisation = 16 bytes (parameter block bytes 48..63)
SNARKV_HD void b2b_init(Blake2bState& s, const uint8_t person16[16]) {
  uint64_t p[2] = {0, 0};
  for (int i = 0; i < 16; ++i) p[i >> 3] |= (uint64_t)person16[i] << (8 * (i & 7));
  for (int i = 0; i < 8; ++i) s.h[i] = b2b_iv(i);
  s.h[0] ^= 0x01010000ull ^ 64ull;  // digest length 64, key length 0, fanout 1, depth 1
  s.h[6] ^= p[0];
  s.h[7] ^= p[1];
  s.t = 0;
  s.fill = 0;
  s.pad_ = 0;
  for (int i = 0; i < 16; ++i) s.buf[i] = 0;
}
SNARKV_HD void tr_init(Blake2bState& s) {
  const uint8_t person[16] = {'H', 'a', 'l', 'o', '2', '-', 'T', 'r', 'a', 'n', 's', 'c', 'r', 'i', 'p', 't'};
  b2b_init(s, person);
}

// A buffer that is exactly full is compressed only when more input arrives: the last block is special.
SNARKV_HD void b2b_update(Blake2bState& s, const uint8_t* in, size_t len) {
  uint8_t* bytes = reinterpret_cast<uint8_t*>(s.buf);
  uint32_t fill = s.fill;
#pragma unroll 1
  for (size_t i = 0; i < len; ++i) {
    if (fill == 128) {
      uint64_t h[8], m[16];
#pragma unroll
      for (int j = 0; j < 8; ++j) h[j] = s.h[j];
#pragma unroll
      for (int j = 0; j < 16; ++j) m[j] = s.buf[j];
      s.t += 128;
      b2b_compress(h, m, s.t, false);
#pragma unroll
      for (int j = 0; j < 8; ++j) s.h[j] = h[j];
      fill = 0;
    }
    bytes[fill++] = in[i];
  }
  s.fill = fill;
}

// digest of everything absorbed so far, of a copy: the state keeps absorbing.  out = 8 little-endian words.
SNARKV_HD void b2b_digest(const Blake2bState& s, uint64_t (&out)[8]) {
  uint64_t m[16];
  const int fill = (int)s.fill;
#pragma unroll
  for (int j = 0; j < 16; ++j) {  // the pending bytes, zero-padded (what lies beyond `fill` is stale)
    const int nb = fill - 8 * j;
    const uint64_t w = s.buf[j];
    m[j] = nb >= 8 ? w : (nb <= 0 ? 0ull : (w & ((1ull << (8 * (nb & 7))) - 1ull)));
  }
#pragma unroll
  for (int j = 0; j < 8; ++j) out[j] = s.h[j];
  b2b_compress(out, m, s.t + (uint64_t)fill, true);
}

// ---- the transcript's messages: what an operation absorbs, written to `msg` (the caller absorbs it with b2b_update) -----
constexpr size_t kTrPointBytes = 65, kTrScalarBytes = 33, kTrSqueezeBytes = 1;

// 0x01 | x | y.  The identity (64 zero bytes) is refused: false, and `msg` holds what a caller that goes on regardless absorbs.
SNARKV_HD bool tr_put_point(uint8_t* msg, const uint8_t* x32, const uint8_t* y32) {
  uint8_t any = 0;
  msg[0] = 0x01;
  for (int i = 0; i < 32; ++i) {
    msg[1 + i] = x32[i];
    msg[33 + i] = y32[i];
    any |= x32[i] | y32[i];
  }
  return any != 0;
}
SNARKV_HD void tr_put_scalar(uint8_t* msg, const uint8_t* s32) {
  msg[0] = 0x02;
  for (int i = 0; i < 32; ++i) msg[1 + i] = s32[i];
}
SNARKV_HD void tr_put_squeeze(uint8_t* msg) { msg[0] = 0x00; }

// x with the parity of y in bit 255
SNARKV_HD void tr_compress_point(const uint8_t* x32, const uint8_t* y32, uint8_t* out32) {
  for (int i = 0; i < 32; ++i) out32[i] = x32[i];
  out32[31] = (uint8_t)(out32[31] | ((y32[0] & 1u) << 7));
}

// ---- from_uniform_bytes: the 512-bit digest reduced mod r, exactly, as lo + hi 2^256 ---------------------------------------
// A 256-bit half reaches 2^256 > 5 r on BN254 (4 r on pallas), outside fr29_from_canonical's contract (< r): it is first
// brought below r by trial subtraction, 2^256 / r < 6 times at most.
SNARKV_HD void fr_reduce256(uint32_t (&w)[8]) {
  constexpr uint32_t r[8] = SNARKV_FR_R_LIMBS;
#pragma unroll 1
  for (int it = 0; it < 6; ++it) {
    uint32_t d[8];
    uint32_t borrow = 0;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const uint64_t t = (uint64_t)w[i] - r[i] - borrow;
      d[i] = (uint32_t)t;
      borrow = (uint32_t)(t >> 63);
    }
    const uint32_t keep = 0u - borrow;  // all ones: w < r
#pragma unroll
    for (int i = 0; i < 8; ++i) w[i] = (w[i] & keep) | (d[i] & ~keep);
  }
}

// digest (8 little-endian u64) -> lo + hi 2^256 mod r in the Montgomery domain.  Both terms are products, each in
// (-r/2, 3r/2) by fr29_mul's bound, so their sum is within (-r, 3r): inside the |a| < 8 r that fr29_mul and
// fr29_to_canonical take.  2^256 mod r is formed as (2^128)^2, 2^128 being canonical in both fields.
SNARKV_HD Fr29 fr_from_uniform(const uint64_t (&dig)[8]) {
  uint32_t lo[8], hi[8];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    lo[2 * i] = (uint32_t)dig[i];
    lo[2 * i + 1] = (uint32_t)(dig[i] >> 32);
    hi[2 * i] = (uint32_t)dig[4 + i];
    hi[2 * i + 1] = (uint32_t)(dig[4 + i] >> 32);
  }
  fr_reduce256(lo);
  fr_reduce256(hi);
  const uint32_t w128[8] = {0, 0, 0, 0, 1, 0, 0, 0};
  const Fr29 t128 = fr29_from_canonical(w128);
  const Fr29 t256 = fr29_mul(t128, t128);  // 2^256 mod r
  return fr29_add(fr29_from_canonical(lo), fr29_mul(fr29_from_canonical(hi), t256));
}

// the challenge of the state as it stands AFTER its 0x00 prefix was absorbed: Montgomery form, and canonical words
SNARKV_HD Fr29 tr_challenge(const Blake2bState& s, uint32_t (&canon)[8]) {
  uint64_t dig[8];
  b2b_digest(s, dig);
  const Fr29 c = fr_from_uniform(dig);
  fr29_to_canonical(c, canon);
  return c;
}

// ---- the operations one at a time (host callers; a kernel batches its messages instead) ------------------------------------
SNARKV_HD bool tr_common_point(Blake2bState& s, const uint8_t* x32, const uint8_t* y32) {
  uint8_t msg[kTrPointBytes];
  if (!tr_put_point(msg, x32, y32)) return false;  // nothing is absorbed
  b2b_update(s, msg, kTrPointBytes);
  return true;
}
SNARKV_HD void tr_common_scalar(Blake2bState& s, const uint8_t* s32) {
  uint8_t msg[kTrScalarBytes];
  tr_put_scalar(msg, s32);
  b2b_update(s, msg, kTrScalarBytes);
}
SNARKV_HD Fr29 tr_squeeze(Blake2bState& s, uint32_t (&canon)[8]) {
  uint8_t msg[kTrSqueezeBytes];
  tr_put_squeeze(msg);
  b2b_update(s, msg, kTrSqueezeBytes);
  return tr_challenge(s, canon);
}

}  // namespace snarkv
