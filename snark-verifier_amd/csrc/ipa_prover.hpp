// Internal: the prover session of ipa_prover.hip as the units built on it see it -- the session object, the layout of its
// small device buffer, the enqueue steps both the session calls (include/snarkv_ipa_prover.h) and the blinded opening
// (ipa_opening.hpp) are made of, and the few device helpers their kernels share.  None of the enqueue steps synchronises
// unless its comment says so.
#pragma once
#include "ctx.hpp"
#include "fr29.h"

namespace snarkv {

#if defined(__HIPCC__)
__device__ __forceinline__ Fr29 ld_fr(const uint32_t* __restrict__ p) {
  const uint4* s = reinterpret_cast<const uint4*>(p);
  uint4 a = s[0], b = s[1];
  uint32_t w[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
  return fr29_from_canonical(w);
}
__device__ __forceinline__ void st_fr(uint32_t* __restrict__ p, const Fr29& v) {
  uint32_t w[8];
  fr29_to_canonical(v, w);
  uint4* o = reinterpret_cast<uint4*>(p);
  o[0] = make_uint4(w[0], w[1], w[2], w[3]);
  o[1] = make_uint4(w[4], w[5], w[6], w[7]);
}
// a + b brought back to (-r/8, 9r/8) (one Montgomery product by 1), so sums of any length stay in fr29_mul's range
__device__ __forceinline__ Fr29 fr_add_red(const Fr29& a, const Fr29& b) { return fr29_mul(fr29_add(a, b), fr29_one()); }
// ---- fr29_mul and fr29_to_canonical with their loops spelled out, for the one-lane inversion k_ipa_xi_inv alone.  That
// kernel is wave-uniform, a serial chain of 380 products on the scalar unit, once per round of the prover.  Through
// mont29_product and the shared tail its loop body compiled 3 % longer on pallas (1 143 -> 1 177 instructions per exponent
// bit; the two together, either one alone changes nothing), and the prover's fold phase at k = 16 measured 14.49 -> 14.76 ms,
// slower in every round with disjoint ranges (profiles/r09_field_layer_refactor.txt).  With these two bodies the loop is
// instruction for instruction what it was.  Same column schedule, same limbs as fr29_mul; same words as fr29_to_canonical.
__device__ __forceinline__ Fr29 fr_inv_mul(const Fr29& a, const Fr29& b) {
  int32_t m[9];
  Fr29 r;
  int64_t acc = 0;
#pragma unroll
  for (int k = 0; k < 9; ++k) {
#pragma unroll
    for (int i = 0; i <= k; ++i) acc += (int64_t)a.v[i] * b.v[k - i];
#pragma unroll
    for (int i = 0; i < k; ++i) acc += (int64_t)m[i] * fr29_r(k - i);
    m[k] = (int32_t)(((uint32_t)acc * (uint32_t)SNARKV_FR29_NINV) & (uint32_t)kMask29);
    acc += (int64_t)m[k] * fr29_r(0);
    acc >>= 29;
  }
#pragma unroll
  for (int k = 9; k < 17; ++k) {
#pragma unroll
    for (int i = k - 8; i < 9; ++i) acc += (int64_t)a.v[i] * b.v[k - i];
#pragma unroll
    for (int i = k - 8; i < 9; ++i) acc += (int64_t)m[i] * fr29_r(k - i);
    r.v[k - 9] = (int32_t)acc & kMask29;
    acc >>= 29;
  }
  r.v[8] = (int32_t)acc;
  return r;
}
__device__ __forceinline__ void fr_inv_store(uint32_t* __restrict__ p, const Fr29& a) {
  Fr29 one_raw = fr29_zero();
  one_raw.v[0] = 1;
  Fr29 y = fr_inv_mul(fr29_norm(a), one_raw);  // a * R^-1
  Fr29 t;
  int32_t neg = y.v[8] >> 31;
#pragma unroll
  for (int i = 0; i < 9; ++i) t.v[i] = y.v[i] + (fr29_r(i) & neg);
  t = fr29_norm(t);
  Fr29 d;
  int32_t c = 0;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    int32_t s = t.v[i] - fr29_r(i) + c;
    d.v[i] = s & kMask29;
    c = s >> 29;
  }
  d.v[8] = t.v[8] - fr29_r(8) + c;
  int32_t keep = d.v[8] >> 31;
#pragma unroll
  for (int i = 0; i < 9; ++i) t.v[i] = (t.v[i] & keep) | (d.v[i] & ~keep);
  uint32_t w[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) w[j] = 0;
#pragma unroll
  for (int i = 0; i < 9; ++i) {
    int bit = 29 * i;
    int word = bit >> 5, sh = bit & 31;
    uint64_t v = (uint64_t)(uint32_t)t.v[i] << sh;
    w[word] |= (uint32_t)v;
    if (word + 1 < 8) w[word + 1] |= (uint32_t)(v >> 32);
  }
  uint4* o = reinterpret_cast<uint4*>(p);
  o[0] = make_uint4(w[0], w[1], w[2], w[3]);
  o[1] = make_uint4(w[4], w[5], w[6], w[7]);
}
// x^(r-2): 254 squarings on the calling lane; 0 -> 0
__device__ __forceinline__ Fr29 fr_inv(const Fr29& x) {
  constexpr uint32_t rw[8] = SNARKV_FR_R_LIMBS;
  uint32_t e[8];
  uint32_t borrow = 2;
  for (int i = 0; i < 8; ++i) {
    uint32_t v = rw[i];
    e[i] = v - borrow;
    borrow = v < borrow ? 1u : 0u;
  }
  Fr29 acc = fr29_one();
#pragma unroll 1
  for (int b = 255; b >= 0; --b) {
    acc = fr_inv_mul(acc, acc);
    if ((e[b >> 5] >> (b & 31)) & 1u) acc = fr_inv_mul(acc, x);
  }
  return acc;
}
#endif

// the inner-product kernels: threads per workgroup, and the cap on workgroups (= partials kept per sum)
constexpr uint32_t kIpThreads = 256;
constexpr uint32_t kIpMaxBlocks = 512;

// layout of a session's small device buffer
enum : size_t {
  SM_COMB_S = 0,      // [1, ip_L, 1, ip_R]         4 x 32
  SM_COMB_P = 128,    // [MSM_L, h', MSM_R, h']     4 x 64
  SM_COMB_OFF = 384,  // {0, 2, 4}
  SM_LR = 400,        // L | R out                  128
  SM_XI = 528,        // xi | xi^-1                 64 (+ 32 spare)
  SM_Z = 624,         // z                          32
  SM_OFF1 = 656,      // {0, 1}
  SM_OFFN = 672,      // {0, 2^b} for b < 32        256
  SM_BAD = 928,       // SNARKV_FLAG_VALIDATE count
  SM_PARTIALS = 1024, // kIpMaxBlocks x 2 Fr29
  SM_BYTES = SM_PARTIALS + kIpMaxBlocks * 2 * sizeof(Fr29),
};

}  // namespace snarkv

struct snarkv_ipa_prover {
  enum State { WANT_ROUND, WANT_FOLD, DONE, FAILED };
  snarkv_ctx* ctx;
  uint32_t k;
  uint32_t rounds;  // rounds completed (folds done)
  State state;
  const void* d_key;  // the deciding key's points: read until the first fold
  void* d_coeffs;     // n x 32
  void* d_zs;         // n x 32
  void* d_bases;      // n/2 x 64
  void* d_ts;         // n/2 x 2 x 32: the base fold's scalars
  void* d_tp;         // n/2 x 2 x 64: its points
  void* d_foff;       // n/2 + 1 offsets {0, 2, 4, ...}
  uint8_t* d_small;
  uint8_t xi_host[32];
};

namespace snarkv {

bool host_canonical(const uint8_t* s32);  // s < r
int device_malloc(void** out, size_t bytes);
// SNARKV_FLAG_VALIDATE: *bad = how many of the n device scalars are >= r.  Synchronises.
int count_bad(snarkv_ctx* ctx, const void* d_s, size_t n, int* d_bad, int* bad);
// one MSM of n terms: the naive segmented kernels up to SNARKV_IPA_NAIVE_MAX terms, the Pippenger beyond
// (`d_off01n` = the offsets {0, n} in device memory)
int ipa_msm(snarkv_ctx* ctx, const void* d_s, const void* d_p, size_t n, const void* d_off01n, void* d_out);
// `IpaProvingKey::commit` on device-resident scalars: out = <s, points> (+ sc2[1] pts2[1] when `blind`).  pts2 = 2 points
// ([0] is written here, [1] = the key's s), sc2 = the scalars [1, omega], off02 = {0, 2}, off0n = {0, n}.
int ipa_enqueue_commit(snarkv_ctx* ctx, const void* d_points, const void* d_s, size_t n, const void* d_off0n, void* d_pts2,
                       const void* d_sc2, const void* d_off02, void* d_out, bool blind);

// A session with its buffers allocated and its inputs staged: coefficients, z, h (in the h' slot) and, when given, xi_0 (in
// the slot of ip_L, where session_enqueue_hprime reads it).  `who` names the entry point in error texts.  Checks the
// coefficients under SNARKV_FLAG_VALIDATE (which synchronises); on any failure nothing is left allocated.
int session_open(snarkv_ctx* ctx, const snarkv_ipa_dk* dk, const void* coeffs, bool on_device, size_t n, const uint8_t* z32,
                 const uint8_t* h64, const uint8_t* xi0_32_or_null, const char* who, snarkv_ipa_prover** out);
// frees the buffers and the object; session_close waits for the stream first
void session_free(snarkv_ipa_prover* p);
void session_close(snarkv_ipa_prover* p);
int session_enqueue_powers(snarkv_ipa_prover* p);   // zs[i] = z^i
int session_enqueue_hprime(snarkv_ipa_prover* p);   // h' = xi_0 h into both h' slots of the L / R combination
int session_enqueue_round(snarkv_ipa_prover* p);    // L | R of round p->rounds at SM_LR, canonical affine
int session_fold_staging(snarkv_ipa_prover* p);     // the base fold's staging, allocated on first use (hipMalloc only)
int session_enqueue_fold(snarkv_ipa_prover* p);     // the fold of round p->rounds by xi | xi^-1 at SM_XI

}  // namespace snarkv
