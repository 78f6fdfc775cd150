// `IpaAs::decide_all` (reference snark-verifier/src/pcs/ipa/decider.rs:57-66) as one folded check
// (include/snarkv_ipa_fold.h): for a challenge rho from the caller
//     sum_i rho^i U_i  ==  < sum_i rho^i h_coeffs(xi_i) , G >
// -- one MSM of 2^k terms and one of m terms whatever m.  Same source for both curves, as ipa.hip.
//   k_ipa_fold_prep     the m x k challenges into the Montgomery domain once
//   k_ipa_fold_powers   rho^i, i < m: Montgomery for the fold, canonical for the MSM over the U_i
//   k_ipa_fold_coeffs   grid (blocks of coefficients, slices of the accumulator range): a lane owns 2^kFoldT consecutive
//                       coefficients and shares the products of their high bits (ipa_fold.h); each slice leaves a partial
//                       vector, a single slice writes h itself
//   k_ipa_fold_sum      h[j] = the sum of the slices' partials: one lane per coefficient, no atomics
// then the two MSMs by the chooser of ipa_prover.hip (the naive segmented kernels up to SNARKV_IPA_NAIVE_MAX terms, the
// Pippenger above; the key's window table for the 2^k-term one when a batched call or prepare() already built it).
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include "ctx.hpp"
#include "ipa_fold.h"
#include "../../include/snarkv_ipa_fold.h"

namespace snarkv {

constexpr uint32_t kFoldLanes = 64;                  // one wavefront: 64 x 2^kFoldT = 512 coefficients per workgroup
constexpr uint32_t kFoldFillWorkgroups = 2048;       // slices = 0: as launch_msm_shared fills the device
constexpr uint32_t kFoldMinPerSlice = 4;             // ... without a slice of fewer accumulators than this
constexpr size_t kFoldPartialsCap = (size_t)256 << 20;
constexpr size_t kFoldMaxSlices = 32768;             // gridDim.y
constexpr uint32_t kFoldMaxM = 1u << 20;

__device__ __forceinline__ Fr29 fold_ld(const uint32_t* __restrict__ p) {
  const uint4* s = reinterpret_cast<const uint4*>(p);
  const uint4 a = s[0], b = s[1];
  const uint32_t w[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
  return fr29_from_canonical(w);
}
__device__ __forceinline__ void fold_st(uint32_t* __restrict__ p, const Fr29& v) {
  uint32_t w[8];
  fr29_to_canonical(v, w);
  uint4* o = reinterpret_cast<uint4*>(p);
  o[0] = make_uint4(w[0], w[1], w[2], w[3]);
  o[1] = make_uint4(w[4], w[5], w[6], w[7]);
}

__global__ void __launch_bounds__(256) k_ipa_fold_prep(const uint32_t* __restrict__ xi_canon, uint32_t count,
                                                       Fr29* __restrict__ out) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i < count) out[i] = fold_ld(xi_canon + 8 * (size_t)i);
}

// pw[i] = rho^i, i < m: rho^(2^b) in LDS, one product per set bit of i (m <= 2^20: 21 squares); canon (optional) = the same
// as canonical scalars
__global__ void __launch_bounds__(256) k_ipa_fold_powers(const uint32_t* __restrict__ rho_canon, uint32_t m,
                                                         Fr29* __restrict__ pw, uint32_t* __restrict__ canon) {
  __shared__ Fr29 sq[21];
  if (threadIdx.x == 0) {
    Fr29 x = fold_ld(rho_canon);
    for (uint32_t b = 0; b < 21; ++b) {
      sq[b] = x;
      x = fr29_mul(x, x);
    }
  }
  __syncthreads();
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= m) return;
  Fr29 acc = fr29_one();
#pragma unroll 1
  for (uint32_t b = 0; b < 21; ++b)
    if ((i >> b) & 1u) acc = fr29_mul(acc, sq[b]);
  pw[i] = acc;
  if (canon) fold_st(canon + 8 * (size_t)i, acc);
}

// blockIdx.y = the slice of the accumulator range.  gridDim.y == 1: canonical coefficients into h; otherwise the slice's
// reduced partial sums into parts[slice][j].
__global__ void __launch_bounds__(kFoldLanes) k_ipa_fold_coeffs(const Fr29* __restrict__ xi, const Fr29* __restrict__ pw,
                                                                uint32_t m, uint32_t k, Fr29* __restrict__ parts,
                                                                uint32_t* __restrict__ h) {
  const uint32_t n = 1u << k;
  const uint32_t lanes = n >> kFoldT ? n >> kFoldT : 1u;
  const uint32_t lane = blockIdx.x * kFoldLanes + threadIdx.x;
  if (lane >= lanes) return;
  const uint32_t i0 = fold_slice_begin(blockIdx.y, gridDim.y, m), i1 = fold_slice_begin(blockIdx.y + 1, gridDim.y, m);
  Fr29 sums[1 << kFoldT];
  ipa_fold_lane<kFoldT>(xi, pw, k, lane, i0, i1, sums);
  const size_t j0 = (size_t)lane << kFoldT;
#pragma unroll
  for (int q = 0; q < (1 << kFoldT); ++q) {
    if ((uint32_t)q < n) {
      if (gridDim.y == 1) fold_st(h + 8 * (j0 + q), sums[q]);
      else parts[(size_t)blockIdx.y * n + j0 + q] = sums[q];
    }
  }
}

__global__ void __launch_bounds__(256) k_ipa_fold_sum(const Fr29* __restrict__ parts, uint32_t n, uint32_t slices,
                                                      uint32_t* __restrict__ h) {
  const uint32_t j = blockIdx.x * 256u + threadIdx.x;
  if (j >= n) return;
  fold_st(h + 8 * (size_t)j, fold_sum_partials(parts + j, n, slices));
}

static bool fold_host_canonical(const uint8_t* s32) {
  constexpr uint32_t rw[8] = SNARKV_FR_R_LIMBS;
  for (int w = 7; w >= 0; --w) {
    uint32_t v;
    memcpy(&v, s32 + 4 * w, 4);
    if (v != rw[w]) return v < rw[w];
  }
  return false;
}

// slices of the accumulator range when `blocks` workgroups cover the coefficients
static uint32_t fold_slices(uint32_t blocks, size_t n, size_t m, uint32_t slices) {
  size_t s = slices ? std::min<size_t>(slices, m) : 1;
  if (!slices)
    while ((size_t)blocks * s < kFoldFillWorkgroups && m / (2 * s) >= kFoldMinPerSlice) s *= 2;
  const size_t cap = std::max<size_t>(1, kFoldPartialsCap / (n * sizeof(Fr29)));  // the partial vectors stay bounded
  return (uint32_t)std::min({s, cap, kFoldMaxSlices});
}

// d_h = sum_i rho^i h_coeffs(xi_i) from d_xi (m x k canonical) and d_rho (canonical); d_pw_canon (optional) receives the
// powers as canonical scalars.  Enqueued.
static int launch_ipa_fold(snarkv_ctx* ctx, const void* d_xi, const void* d_rho, size_t m, uint32_t k, uint32_t slices,
                           void* d_pw_canon, void* d_h) {
  const size_t n = (size_t)1 << k, count = m * k;
  const uint32_t lanes = (uint32_t)std::max<size_t>(1, n >> kFoldT);
  const uint32_t blocks = (lanes + kFoldLanes - 1) / kFoldLanes;
  const uint32_t S = fold_slices(blocks, n, m, slices);
  // scratch: xi (Montgomery) | powers (Montgomery) | S partial vectors
  const size_t o_pw = (count * sizeof(Fr29) + 15) / 16 * 16, o_parts = o_pw + (m * sizeof(Fr29) + 15) / 16 * 16;
  void* d_sc;
  SNARKV_TRY(ctx_reserve(ctx, SLOT_IPA_FOLD, o_parts + (S > 1 ? (size_t)S * n * sizeof(Fr29) : 0), &d_sc));
  Fr29* x29 = (Fr29*)d_sc;
  Fr29* pw = (Fr29*)((uint8_t*)d_sc + o_pw);
  Fr29* parts = (Fr29*)((uint8_t*)d_sc + o_parts);
  hipLaunchKernelGGL(k_ipa_fold_prep, dim3((uint32_t)((count + 255) / 256)), dim3(256), 0, ctx->stream,
                     (const uint32_t*)d_xi, (uint32_t)count, x29);
  hipLaunchKernelGGL(k_ipa_fold_powers, dim3((uint32_t)((m + 255) / 256)), dim3(256), 0, ctx->stream,
                     (const uint32_t*)d_rho, (uint32_t)m, pw, (uint32_t*)d_pw_canon);
  hipLaunchKernelGGL(k_ipa_fold_coeffs, dim3(blocks, S), dim3(kFoldLanes), 0, ctx->stream, (const Fr29*)x29,
                     (const Fr29*)pw, (uint32_t)m, k, parts, (uint32_t*)d_h);
  if (S > 1)
    hipLaunchKernelGGL(k_ipa_fold_sum, dim3((uint32_t)((n + 255) / 256)), dim3(256), 0, ctx->stream, (const Fr29*)parts,
                       (uint32_t)n, S, (uint32_t*)d_h);
  SNARKV_HIP(hipGetLastError());
  return SNARKV_OK;
}

// the argument checks the two entry points share; SNARKV_FLAG_VALIDATE on the host (k m + 1 scalars)
static int fold_check(snarkv_ctx* ctx, uint32_t k, const uint8_t* xi32, size_t m, const uint8_t* rho32) {
  if (k < 1 || k > 28 || m > kFoldMaxM) return SNARKV_ERR_LENGTH;
  if (ctx->flags & SNARKV_FLAG_VALIDATE) {
    bool ok = fold_host_canonical(rho32);
    for (size_t i = 0; ok && i < m * k; ++i) ok = fold_host_canonical(xi32 + 32 * i);
    if (!ok) {
      set_last_error("ipa_fold: a scalar is not canonical");
      return SNARKV_ERR_ENCODING;
    }
  }
  return SNARKV_OK;
}

// one MSM of n terms, as ipa_prover.hip chooses it (`d_off01n` = the offsets {0, n} in device memory)
static int fold_msm(snarkv_ctx* ctx, const void* d_s, const void* d_p, size_t n, const void* d_off01n, void* d_out) {
  static const size_t naive_max = [] {
    const char* e = getenv("SNARKV_IPA_NAIVE_MAX");
    return e ? (size_t)strtoull(e, nullptr, 10) : (size_t)4096;
  }();
  if (n <= naive_max) return launch_msm_batched(ctx, d_s, d_p, d_off01n, 1, n, d_out);
  return launch_msm_pippenger_auto(ctx, d_s, d_p, n, 0, d_out, false);
}

// the table of a key serves a single vector up to this k (ipa.hip's thresholds: it wins at m = 1 up to k = 14 and loses
// at 16); only a table that is already built is used
constexpr uint32_t kFoldTableMaxK = 14;
static bool fold_table_built(const snarkv_ipa_dk* dk) {
  std::lock_guard<std::mutex> lk(dk->table_mu);
  return dk->table_state == 1 && dk->d_table != nullptr;
}

}  // namespace snarkv

using namespace snarkv;

// layout of the small device buffer (SLOT_IPA_OUT)
enum : size_t {
  FS_RHO = 0,     // rho                         32
  FS_OFF_N = 32,  // {0, 2^k}
  FS_OFF_M = 40,  // {0, m}
  FS_OUT = 64,    // <h, G> | sum rho^i U_i      128
  FS_BYTES = 192,
};

extern "C" {

int SNARKV_API(ipa_fold_coeffs_dev)(snarkv_ctx* ctx, uint32_t k, const uint8_t* xi32, size_t m, const uint8_t rho32[32],
                                    uint32_t slices, void* d_h32) {
  if (!ctx || !xi32 || !rho32 || !d_h32) return SNARKV_ERR_ARG;
  if (reinterpret_cast<uintptr_t>(d_h32) % 16) return SNARKV_ERR_ARG;  // 16-byte stores
  if (m == 0) return SNARKV_ERR_EMPTY;
  SNARKV_TRY(fold_check(ctx, k, xi32, m, rho32));
  SNARKV_HIP(hipSetDevice(ctx->device));
  SNARKV_WIRE_FORM(ctx);
  void *d_xi, *d_sm;
  SNARKV_TRY(stage_in(ctx, SLOT_IPA_XI, xi32, m * k * 32, &d_xi));
  SNARKV_TRY(stage_in(ctx, SLOT_IPA_OUT, rho32, 32, &d_sm));
  SNARKV_HIP(hipStreamSynchronize(ctx->stream));  // the host arguments are consumed: the caller may reuse them
  return launch_ipa_fold(ctx, d_xi, d_sm, m, k, slices, nullptr, d_h32);
}

int SNARKV_API(ipa_decide_folded)(snarkv_ctx* ctx, const snarkv_ipa_dk* dk, const uint8_t* xi32, const uint8_t* u64,
                                  size_t m, const uint8_t rho32[32], int* all_ok) {
  if (!ctx || !dk || !xi32 || !u64 || !rho32 || !all_ok) return SNARKV_ERR_ARG;
  *all_ok = 0;
  if (m == 0) return SNARKV_ERR_EMPTY;
  if (dk->device != ctx->device) return SNARKV_ERR_ARG;
  if (dk->first != 0 || dk->count != ((size_t)1 << dk->k)) return SNARKV_ERR_LENGTH;  // a shard cannot decide alone
  const uint32_t k = dk->k;
  SNARKV_TRY(fold_check(ctx, k, xi32, m, rho32));
  SNARKV_HIP(hipSetDevice(ctx->device));
  SNARKV_WIRE_FORM(ctx);
  const size_t n = (size_t)1 << k;
  // 1. stage xi, U and the small buffer
  void *d_xi, *d_u, *d_pw, *d_h, *d_small;
  SNARKV_TRY(stage_in(ctx, SLOT_IPA_XI, xi32, m * k * 32, &d_xi));
  SNARKV_TRY(stage_in(ctx, SLOT_IN_POINTS, u64, m * 64, &d_u));
  SNARKV_TRY(ctx_reserve(ctx, SLOT_IN_SCALARS, m * 32, &d_pw));
  SNARKV_TRY(ctx_reserve(ctx, SLOT_IPA_H, n * 32, &d_h));
  uint8_t st[FS_OUT] = {0};
  memcpy(st + FS_RHO, rho32, 32);
  const uint32_t offs[4] = {0, (uint32_t)n, 0, (uint32_t)m};
  memcpy(st + FS_OFF_N, offs, sizeof(offs));
  SNARKV_TRY(ctx_reserve(ctx, SLOT_IPA_OUT, FS_BYTES, &d_small));
  uint8_t* sm = (uint8_t*)d_small;
  SNARKV_HIP(hipMemcpyAsync(sm, st, sizeof(st), hipMemcpyHostToDevice, ctx->stream));
  SNARKV_HIP(hipStreamSynchronize(ctx->stream));  // `st` lives on this frame
  // 2. every U canonical and on the curve (or the identity): anything else is a reject
  int bad = 0;
  SNARKV_TRY(launch_validate(ctx, nullptr, d_u, m, &bad));
  if (bad) return SNARKV_OK;
  // 3. the power table and the folded coefficients
  SNARKV_TRY(launch_ipa_fold(ctx, d_xi, sm + FS_RHO, m, k, 0, d_pw, d_h));
  // 4. <h, G>: one MSM of n terms
  if (k <= kFoldTableMaxK && fold_table_built(dk)) SNARKV_TRY(launch_msm_shared(ctx, dk, d_h, n, 1, 0, sm + FS_OUT));
  else SNARKV_TRY(fold_msm(ctx, d_h, dk->d_points, n, sm + FS_OFF_N, sm + FS_OUT));
  // 5. sum rho^i U_i: one MSM of m terms
  SNARKV_TRY(fold_msm(ctx, d_pw, d_u, m, sm + FS_OFF_M, sm + FS_OUT + 64));
  // 6. compare
  uint8_t got[128];
  SNARKV_TRY(fetch_out(ctx, sm + FS_OUT, got, sizeof(got)));
  *all_ok = memcmp(got, got + 64, 64) == 0 ? 1 : 0;
  return SNARKV_OK;
}

}  // extern "C"
