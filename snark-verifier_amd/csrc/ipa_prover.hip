// The IPA prover on the device (include/snarkv_ipa_prover.h): the rounds of `Ipa::create_proof`
// (reference snark-verifier/src/pcs/ipa.rs:39-124) and the h-combination of `IpaAs::create_proof`
// (pcs/ipa/accumulation.rs:186-207).  Same source for both curves, as ipa.hip.
//
// A session holds the folded state in buffers of its own: n coefficients, n powers of z, n/2 folded bases and
// the staging of the base fold.  Per round:
//   round  k_ipa_inner2 + k_ipa_inner_final  <coeffs[half..], zs[..half]>, <coeffs[..half], zs[half..]>
//          two MSMs of `half` terms         Pippenger (the naive segmented kernels below SNARKV_IPA_NAIVE_MAX)
//          one segmented launch of 2 x 2    L = MSM_L + ip_L h',  R = MSM_R + ip_R h';  128 B back to the host
//   fold   k_ipa_xi_inv                      xi^-1 = xi^(r-2) on one lane (the host has no Fr arithmetic here)
//          k_ipa_fold_scalars                coeffs[j] += xi^-1 coeffs[half+j],  zs[j] += xi zs[half+j]
//          k_ipa_fold_terms + segmented MSM  G'[j] = 1 G[j] + xi G[half+j]: half MSMs of 2 terms each
// The base fold is the 2-term segmented MSM of msm_naive.hip (k_term_* + k_segment_fold, which handle the identity,
// equal and opposite points).  A dedicated fold kernel (one GLV double-and-add per lane on the same steps, careful
// additions, one inversion per workgroup) was measured against it and lost at every size: profiles/r07_ipa_prover.txt.
#include <stdlib.h>
#include <algorithm>
#include <string.h>
#include <vector>
#include "ipa_prover.hpp"
#include "../../include/snarkv_ipa_prover.h"
#include "../../include/snarkv_ipa_batch.h"
#include "../../include/snarkv_ipa_commit_blinded.h"

namespace snarkv {

// zs[i] = z^i, i < n (the reference's `powers(*z)`): z^(2^b) in LDS, one product per set bit of i
__global__ void __launch_bounds__(256) k_ipa_powers(const uint32_t* __restrict__ z_canon, uint32_t k, uint32_t n,
                                                    uint32_t* __restrict__ zs) {
  __shared__ Fr29 sq[32];
  if (threadIdx.x == 0) {
    Fr29 x = ld_fr(z_canon);
    for (uint32_t b = 0; b < k; ++b) {
      sq[b] = x;
      x = fr29_mul(x, x);
    }
  }
  __syncthreads();
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= n) return;
  Fr29 acc = fr29_one();
#pragma unroll 1
  for (uint32_t b = 0; b < k; ++b)
    if ((i >> b) & 1u) acc = fr29_mul(acc, sq[b]);
  st_fr(zs + 8 * (size_t)i, acc);
}

// xi_pair[8..16) = xi_pair[0..8)^(r-2), on one lane (254 squarings)
__global__ void k_ipa_xi_inv(uint32_t* __restrict__ xi_pair) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  fr_inv_store(xi_pair + 8, fr_inv(ld_fr(xi_pair)));
}

// coeffs[j] += xi^-1 coeffs[half + j],  zs[j] += xi zs[half + j]   (in place: lane j alone reads half+j and writes j)
__global__ void __launch_bounds__(256) k_ipa_fold_scalars(uint32_t* __restrict__ coeffs, uint32_t* __restrict__ zs,
                                                          uint32_t half, const uint32_t* __restrict__ xi_pair) {
  const uint32_t j = blockIdx.x * 256u + threadIdx.x;
  if (j >= half) return;
  const Fr29 xi = ld_fr(xi_pair), xi_inv = ld_fr(xi_pair + 8);
  const size_t lo = 8 * (size_t)j, hi = 8 * ((size_t)half + j);
  st_fr(coeffs + lo, fr29_add(ld_fr(coeffs + lo), fr29_mul(xi_inv, ld_fr(coeffs + hi))));
  st_fr(zs + lo, fr29_add(ld_fr(zs + lo), fr29_mul(xi, ld_fr(zs + hi))));
}

// the terms of the base fold: MSM j = (1, G[j]) + (xi, G[half + j])
__global__ void __launch_bounds__(256) k_ipa_fold_terms(const uint32_t* __restrict__ bases, uint32_t half,
                                                        const uint32_t* __restrict__ xi_pair, uint32_t* __restrict__ ts,
                                                        uint32_t* __restrict__ tp) {
  const uint32_t j = blockIdx.x * 256u + threadIdx.x;
  if (j >= half) return;
  const uint4* x = reinterpret_cast<const uint4*>(xi_pair);
  uint4* s = reinterpret_cast<uint4*>(ts + 16 * (size_t)j);
  s[0] = make_uint4(1u, 0u, 0u, 0u);
  s[1] = make_uint4(0u, 0u, 0u, 0u);
  s[2] = x[0];
  s[3] = x[1];
  const uint4* a = reinterpret_cast<const uint4*>(bases + 16 * (size_t)j);
  const uint4* b = reinterpret_cast<const uint4*>(bases + 16 * ((size_t)half + j));
  uint4* p = reinterpret_cast<uint4*>(tp + 32 * (size_t)j);
#pragma unroll
  for (int q = 0; q < 4; ++q) p[q] = a[q];
#pragma unroll
  for (int q = 0; q < 4; ++q) p[4 + q] = b[q];
}

// the offsets of the base fold's 2-term MSMs: {0, 2, 4, ..., 2 (count - 1)}
__global__ void __launch_bounds__(256) k_ipa_fold_offsets(uint32_t* __restrict__ foff, uint32_t count) {
  const uint32_t j = blockIdx.x * 256u + threadIdx.x;
  if (j < count) foff[j] = 2u * j;
}

// per-workgroup partial sums of <coeffs[half..], zs[..half]> (L) and <coeffs[..half], zs[half..]> (R)
__global__ void __launch_bounds__(kIpThreads) k_ipa_inner2(const uint32_t* __restrict__ coeffs, const uint32_t* __restrict__ zs,
                                                           uint32_t half, Fr29* __restrict__ partials) {
  __shared__ Fr29 sl[kIpThreads], sr[kIpThreads];
  Fr29 al = fr29_zero(), ar = fr29_zero();
  for (uint32_t j = blockIdx.x * kIpThreads + threadIdx.x; j < half; j += gridDim.x * kIpThreads) {
    const size_t lo = 8 * (size_t)j, hi = 8 * ((size_t)half + j);
    al = fr_add_red(al, fr29_mul(ld_fr(coeffs + hi), ld_fr(zs + lo)));
    ar = fr_add_red(ar, fr29_mul(ld_fr(coeffs + lo), ld_fr(zs + hi)));
  }
  sl[threadIdx.x] = al;
  sr[threadIdx.x] = ar;
  __syncthreads();
  for (uint32_t s = kIpThreads / 2; s > 0; s >>= 1) {
    if (threadIdx.x < s) {
      sl[threadIdx.x] = fr_add_red(sl[threadIdx.x], sl[threadIdx.x + s]);
      sr[threadIdx.x] = fr_add_red(sr[threadIdx.x], sr[threadIdx.x + s]);
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    partials[2 * blockIdx.x] = sl[0];
    partials[2 * blockIdx.x + 1] = sr[0];
  }
}

// the final fold of the partials: canonical ip_L -> out_l, ip_R -> out_r (the scalar slots of the L / R combination)
__global__ void __launch_bounds__(kIpThreads) k_ipa_inner_final(const Fr29* __restrict__ partials, uint32_t blocks,
                                                                uint32_t* __restrict__ out_l, uint32_t* __restrict__ out_r) {
  __shared__ Fr29 sl[kIpThreads], sr[kIpThreads];
  Fr29 al = fr29_zero(), ar = fr29_zero();
  for (uint32_t b = threadIdx.x; b < blocks; b += kIpThreads) {
    al = fr_add_red(al, partials[2 * b]);
    ar = fr_add_red(ar, partials[2 * b + 1]);
  }
  sl[threadIdx.x] = al;
  sr[threadIdx.x] = ar;
  __syncthreads();
  for (uint32_t s = kIpThreads / 2; s > 0; s >>= 1) {
    if (threadIdx.x < s) {
      sl[threadIdx.x] = fr_add_red(sl[threadIdx.x], sl[threadIdx.x + s]);
      sr[threadIdx.x] = fr_add_red(sr[threadIdx.x], sr[threadIdx.x + s]);
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    st_fr(out_l, sl[0]);
    st_fr(out_r, sr[0]);
  }
}

// SNARKV_FLAG_VALIDATE: count the scalars >= r
__global__ void __launch_bounds__(256) k_ipa_check_canon(const uint32_t* __restrict__ s, uint32_t n, int* __restrict__ bad) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= n) return;
  constexpr uint32_t rw[8] = SNARKV_FR_R_LIMBS;
  int cmp = 0;  // -1: s < r, 1: s > r, 0: equal so far
#pragma unroll
  for (int w = 7; w >= 0; --w) {
    const uint32_t v = s[8 * (size_t)i + w];
    if (cmp == 0) cmp = v < rw[w] ? -1 : (v > rw[w] ? 1 : 0);
  }
  if (cmp >= 0) atomicAdd(bad, 1);
}

// the m x k challenges into the Montgomery domain once (the combination reads each n times)
__global__ void __launch_bounds__(256) k_ipa_as_prep(const uint32_t* __restrict__ xi_canon, uint32_t count, Fr29* __restrict__ out) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i < count) out[i] = ld_fr(xi_canon + 8 * (size_t)i);
}

// h[j] = sum_{i<m} alpha^i h_coeffs(xi_i)[j] (+ alpha^m (b, a, 0, ...)) by Horner over i, from the zk term down;
// h_coeffs(xi_i)[j] = prod over the set bits b of j of xi_i[k-1-b] (k_h_coeffs of ipa.hip).  `small` = alpha | a | b.
__global__ void __launch_bounds__(256) k_ipa_as_combine(const Fr29* __restrict__ xi, uint32_t m, uint32_t k,
                                                        const uint32_t* __restrict__ small, uint32_t zk,
                                                        uint32_t* __restrict__ h) {
  const uint32_t n = 1u << k;
  const uint32_t j = blockIdx.x * 256u + threadIdx.x;
  if (j >= n) return;
  const Fr29 alpha = ld_fr(small);
  Fr29 acc = fr29_zero();
  if (zk && j < 2) acc = ld_fr(small + (j == 0 ? 16 : 8));  // b at 0, a at 1 (accumulation.rs:188-191)
#pragma unroll 1
  for (int i = (int)m - 1; i >= 0; --i) {
    const Fr29* x = xi + (size_t)i * k;
    Fr29 c = fr29_one();
#pragma unroll 1
    for (uint32_t b = 0; b < k; ++b)
      if ((j >> b) & 1u) c = fr29_mul(c, x[k - 1 - b]);
    acc = fr29_add(fr29_mul(acc, alpha), c);
  }
  st_fr(h + 8 * (size_t)j, acc);
}

bool host_canonical(const uint8_t* s32) {
  constexpr uint32_t rw[8] = SNARKV_FR_R_LIMBS;
  for (int w = 7; w >= 0; --w) {
    uint32_t v;
    memcpy(&v, s32 + 4 * w, 4);
    if (v != rw[w]) return v < rw[w];
  }
  return false;
}

static size_t naive_max() {
  static const size_t v = [] {
    const char* e = getenv("SNARKV_IPA_NAIVE_MAX");
    return e ? (size_t)strtoull(e, nullptr, 10) : (size_t)4096;  // measured crossover: profiles/r07_ipa_prover.txt
  }();
  return v;
}
int ipa_msm(snarkv_ctx* ctx, const void* d_s, const void* d_p, size_t n, const void* d_off01n, void* d_out) {
  if (n <= naive_max()) return launch_msm_batched(ctx, d_s, d_p, d_off01n, 1, n, d_out);
  return launch_msm_pippenger_auto(ctx, d_s, d_p, n, 0, d_out, false);  // the product path of snarkv_g1_msm_pippenger_dev
}

static void prover_free(snarkv_ipa_prover* p) {
  void* bufs[] = {p->d_coeffs, p->d_zs, p->d_bases, p->d_ts, p->d_tp, p->d_foff, p->d_small};
  for (void* b : bufs)
    if (b) (void)hipFree(b);
}

int device_malloc(void** out, size_t bytes) {
  if (hipMalloc(out, bytes) != hipSuccess) {
    *out = nullptr;
    set_last_error("ipa_prover: hipMalloc of %zu bytes failed", bytes);
    return SNARKV_ERR_DEVICE;
  }
  return SNARKV_OK;
}

int count_bad(snarkv_ctx* ctx, const void* d_s, size_t n, int* d_bad, int* bad) {
  SNARKV_HIP(hipMemsetAsync(d_bad, 0, sizeof(int), ctx->stream));
  hipLaunchKernelGGL(k_ipa_check_canon, dim3((uint32_t)((n + 255) / 256)), dim3(256), 0, ctx->stream,
                     (const uint32_t*)d_s, (uint32_t)n, d_bad);
  SNARKV_HIP(hipGetLastError());
  SNARKV_HIP(hipMemcpyAsync(bad, d_bad, sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
  SNARKV_HIP(hipStreamSynchronize(ctx->stream));
  return SNARKV_OK;
}

void session_free(snarkv_ipa_prover* p) {
  prover_free(p);
  delete p;
}

void session_close(snarkv_ipa_prover* p) {
  (void)hipSetDevice(p->ctx->device);
  (void)hipStreamSynchronize(p->ctx->stream);  // enqueued work may still read the buffers
  session_free(p);
}

int session_open(snarkv_ctx* ctx, const snarkv_ipa_dk* dk, const void* coeffs, bool on_device, size_t n, const uint8_t* z32,
                 const uint8_t* h64, const uint8_t* xi0_32, const char* who, snarkv_ipa_prover** out) {
  *out = nullptr;
  if (dk->device != ctx->device) return SNARKV_ERR_ARG;
  if (dk->first != 0 || dk->count != ((size_t)1 << dk->k)) return SNARKV_ERR_LENGTH;  // a shard cannot prove alone
  if (n != dk->count) return SNARKV_ERR_LENGTH;
  const bool validate = (ctx->flags & SNARKV_FLAG_VALIDATE) != 0;
  if (validate && (!host_canonical(z32) || (xi0_32 && !host_canonical(xi0_32)))) {
    set_last_error("%s: z or xi_0 is not canonical", who);
    return SNARKV_ERR_ENCODING;
  }
  SNARKV_HIP(hipSetDevice(ctx->device));
  snarkv_ipa_prover* p = new snarkv_ipa_prover();
  memset(p, 0, sizeof(*p));
  p->ctx = ctx;
  p->k = dk->k;
  p->d_key = dk->d_points;
  const size_t half = n / 2;
  int rc = SNARKV_OK;
  auto fail = [&](int code) {
    session_close(p);
    return code;
  };
  if ((rc = device_malloc(&p->d_coeffs, n * 32)) || (rc = device_malloc(&p->d_zs, n * 32)) ||
      (rc = device_malloc(&p->d_bases, half * 64)) || (rc = device_malloc((void**)&p->d_small, SM_BYTES)))
    return fail(rc);
  // the constant part of the small buffer, staged once
  std::vector<uint8_t> st(SM_BAD, 0);
  st[SM_COMB_S] = 1;
  if (xi0_32) memcpy(&st[SM_COMB_S + 32], xi0_32, 32);  // slot of ip_L: xi_0 until h' is formed
  st[SM_COMB_S + 64] = 1;
  memcpy(&st[SM_COMB_P + 64], h64, 64);
  const uint32_t comb_off[3] = {0, 2, 4};
  memcpy(&st[SM_COMB_OFF], comb_off, sizeof(comb_off));
  memcpy(&st[SM_Z], z32, 32);
  const uint32_t off1[2] = {0, 1};
  memcpy(&st[SM_OFF1], off1, sizeof(off1));
  for (uint32_t b = 0; b < 32; ++b) {
    const uint32_t o[2] = {0, b < 31 ? 1u << b : 0u};
    memcpy(&st[SM_OFFN + 8 * b], o, 8);
  }
  hipStream_t s = ctx->stream;
  // `st` is pageable memory: the copy has left it when hipMemcpyAsync returns
  if (hipMemcpyAsync(p->d_small, st.data(), st.size(), hipMemcpyHostToDevice, s) != hipSuccess ||
      hipMemcpyAsync(p->d_coeffs, coeffs, n * 32, on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, s) !=
          hipSuccess) {
    set_last_error("%s: upload failed", who);
    return fail(SNARKV_ERR_DEVICE);
  }
  if (validate) {
    int bad = 0;
    if ((rc = count_bad(ctx, p->d_coeffs, n, (int*)(p->d_small + SM_BAD), &bad))) return fail(rc);
    if (bad) {
      set_last_error("%s: %d of %zu coefficients are not canonical", who, bad, n);
      return fail(SNARKV_ERR_ENCODING);
    }
  }
  p->state = snarkv_ipa_prover::WANT_ROUND;
  *out = p;
  return SNARKV_OK;
}

int session_enqueue_powers(snarkv_ipa_prover* p) {
  const size_t n = (size_t)1 << p->k;
  hipLaunchKernelGGL(k_ipa_powers, dim3((uint32_t)((n + 255) / 256)), dim3(256), 0, p->ctx->stream,
                     (const uint32_t*)(p->d_small + SM_Z), p->k, (uint32_t)n, (uint32_t*)p->d_zs);
  SNARKV_HIP(hipGetLastError());
  return SNARKV_OK;
}

// h' = xi_0 h (ipa.rs:71), into both h' slots of the L / R combination
int session_enqueue_hprime(snarkv_ipa_prover* p) {
  snarkv_ctx* ctx = p->ctx;
  SNARKV_WIRE_FORM(ctx);
  uint8_t* sm = p->d_small;
  SNARKV_TRY(launch_msm_batched(ctx, sm + SM_COMB_S + 32, sm + SM_COMB_P + 64, sm + SM_OFF1, 1, 1, sm + SM_LR));
  SNARKV_HIP(hipMemcpyAsync(sm + SM_COMB_P + 64, sm + SM_LR, 64, hipMemcpyDeviceToDevice, ctx->stream));
  SNARKV_HIP(hipMemcpyAsync(sm + SM_COMB_P + 192, sm + SM_LR, 64, hipMemcpyDeviceToDevice, ctx->stream));
  return SNARKV_OK;
}

int session_enqueue_round(snarkv_ipa_prover* p) {
  snarkv_ctx* ctx = p->ctx;
  SNARKV_HIP(hipSetDevice(ctx->device));
  SNARKV_WIRE_FORM(ctx);
  const size_t half = (size_t)1 << (p->k - p->rounds - 1);
  const uint8_t* bases = (const uint8_t*)(p->rounds == 0 ? p->d_key : p->d_bases);
  const uint8_t* coeffs = (const uint8_t*)p->d_coeffs;
  uint8_t* sm = p->d_small;
  hipStream_t s = ctx->stream;
  const uint32_t blocks = (uint32_t)std::min<size_t>(kIpMaxBlocks, (half + kIpThreads - 1) / kIpThreads);
  hipLaunchKernelGGL(k_ipa_inner2, dim3(blocks), dim3(kIpThreads), 0, s, (const uint32_t*)coeffs,
                     (const uint32_t*)p->d_zs, (uint32_t)half, (Fr29*)(sm + SM_PARTIALS));
  hipLaunchKernelGGL(k_ipa_inner_final, dim3(1), dim3(kIpThreads), 0, s, (const Fr29*)(sm + SM_PARTIALS), blocks,
                     (uint32_t*)(sm + SM_COMB_S + 32), (uint32_t*)(sm + SM_COMB_S + 96));
  SNARKV_HIP(hipGetLastError());
  const uint8_t* offn = sm + SM_OFFN + 8 * (p->k - p->rounds - 1);
  SNARKV_TRY(ipa_msm(ctx, coeffs + 32 * half, bases, half, offn, sm + SM_COMB_P));       // <coeffs[half..], G[..half]>
  SNARKV_TRY(ipa_msm(ctx, coeffs, bases + 64 * half, half, offn, sm + SM_COMB_P + 128)); // <coeffs[..half], G[half..]>
  return launch_msm_batched(ctx, sm + SM_COMB_S, sm + SM_COMB_P, sm + SM_COMB_OFF, 2, 4, sm + SM_LR);
}

// the staging of the base fold (half 2-term MSMs through the segmented kernels of msm_naive.hip) and its offsets
int session_fold_staging(snarkv_ipa_prover* p) {
  if (p->d_ts) return SNARKV_OK;
  const size_t nh = (size_t)1 << (p->k - 1);
  SNARKV_TRY(device_malloc(&p->d_ts, nh * 64));
  SNARKV_TRY(device_malloc(&p->d_tp, nh * 128));
  SNARKV_TRY(device_malloc(&p->d_foff, (nh + 1) * 4));
  hipLaunchKernelGGL(k_ipa_fold_offsets, dim3((uint32_t)((nh + 1 + 255) / 256)), dim3(256), 0, p->ctx->stream,
                     (uint32_t*)p->d_foff, (uint32_t)(nh + 1));
  SNARKV_HIP(hipGetLastError());
  return SNARKV_OK;
}

int session_enqueue_fold(snarkv_ipa_prover* p) {
  snarkv_ctx* ctx = p->ctx;
  SNARKV_HIP(hipSetDevice(ctx->device));
  SNARKV_WIRE_FORM(ctx);
  const size_t half = (size_t)1 << (p->k - p->rounds - 1);
  const uint8_t* bases = (const uint8_t*)(p->rounds == 0 ? p->d_key : p->d_bases);
  uint8_t* sm = p->d_small;
  hipStream_t s = ctx->stream;
  const uint32_t grid = (uint32_t)((half + 255) / 256);
  hipLaunchKernelGGL(k_ipa_fold_scalars, dim3(grid), dim3(256), 0, s, (uint32_t*)p->d_coeffs, (uint32_t*)p->d_zs,
                     (uint32_t)half, (const uint32_t*)(sm + SM_XI));
  SNARKV_TRY(session_fold_staging(p));
  hipLaunchKernelGGL(k_ipa_fold_terms, dim3(grid), dim3(256), 0, s, (const uint32_t*)bases, (uint32_t)half,
                     (const uint32_t*)(sm + SM_XI), (uint32_t*)p->d_ts, (uint32_t*)p->d_tp);
  SNARKV_HIP(hipGetLastError());
  return launch_msm_batched(ctx, p->d_ts, p->d_tp, p->d_foff, half, 2 * half, p->d_bases);
}

int ipa_enqueue_commit(snarkv_ctx* ctx, const void* d_points, const void* d_s, size_t n, const void* d_off0n, void* d_pts2,
                       const void* d_sc2, const void* d_off02, void* d_out, bool blind) {
  SNARKV_TRY(ipa_msm(ctx, d_s, d_points, n, d_off0n, blind ? d_pts2 : d_out));
  if (blind) SNARKV_TRY(launch_msm_batched(ctx, d_sc2, d_pts2, d_off02, 1, 2, d_out));
  return SNARKV_OK;
}

}  // namespace snarkv

using namespace snarkv;

namespace {

int prover_begin(snarkv_ctx* ctx, const snarkv_ipa_dk* dk, const void* coeffs, bool on_device, size_t n,
                 const uint8_t* z32, const uint8_t* h64, const uint8_t* xi0_32, snarkv_ipa_prover** out) {
  if (!ctx || !dk || !coeffs || !z32 || !h64 || !xi0_32 || !out) return SNARKV_ERR_ARG;
  snarkv_ipa_prover* p = nullptr;
  SNARKV_TRY(session_open(ctx, dk, coeffs, on_device, n, z32, h64, xi0_32, "ipa_prover_begin", &p));
  int rc = SNARKV_OK;
  if ((rc = session_enqueue_powers(p)) || (rc = session_enqueue_hprime(p))) {
    session_close(p);
    return rc;
  }
  if (hipStreamSynchronize(ctx->stream) != hipSuccess) {
    set_last_error("ipa_prover_begin: %s", hipGetErrorString(hipGetLastError()));
    session_close(p);
    return SNARKV_ERR_DEVICE;
  }
  *out = p;
  return SNARKV_OK;
}

int prover_round(snarkv_ipa_prover* p, uint8_t* l64, uint8_t* r64) {
  SNARKV_TRY(session_enqueue_round(p));
  hipStream_t s = p->ctx->stream;
  uint8_t lr[128];
  SNARKV_HIP(hipMemcpyAsync(lr, p->d_small + SM_LR, 128, hipMemcpyDeviceToHost, s));
  SNARKV_HIP(hipStreamSynchronize(s));
  memcpy(l64, lr, 64);
  memcpy(r64, lr + 64, 64);
  return SNARKV_OK;
}

int prover_fold(snarkv_ipa_prover* p) {
  snarkv_ctx* ctx = p->ctx;
  SNARKV_HIP(hipSetDevice(ctx->device));
  uint8_t* sm = p->d_small;
  hipStream_t s = ctx->stream;
  SNARKV_HIP(hipMemcpyAsync(sm + SM_XI, p->xi_host, 32, hipMemcpyHostToDevice, s));
  hipLaunchKernelGGL(k_ipa_xi_inv, dim3(1), dim3(64), 0, s, (uint32_t*)(sm + SM_XI));
  SNARKV_TRY(session_enqueue_fold(p));
  if (p->rounds == 0) {
    SNARKV_HIP(hipStreamSynchronize(s));  // the key is no longer read: the caller may destroy it
    p->d_key = nullptr;
  }
  return SNARKV_OK;
}

// the order checks of a session call: SNARKV_OK when `want` is the state
int session_check(snarkv_ipa_prover* p, snarkv_ipa_prover::State want) {
  if (!p || p->state != want) return SNARKV_ERR_ARG;
  return SNARKV_OK;
}

}  // namespace

extern "C" {

int SNARKV_API(ipa_commit)(snarkv_ctx* ctx, const snarkv_ipa_dk* dk, const uint8_t* poly32, size_t n,
                           const uint8_t* omega32, const uint8_t* s64, uint8_t out64[64]) {
  if (!ctx || !dk || !poly32 || !out64 || (omega32 == nullptr) != (s64 == nullptr)) return SNARKV_ERR_ARG;
  if (dk->device != ctx->device) return SNARKV_ERR_ARG;
  if (n == 0) return SNARKV_ERR_EMPTY;
  if (dk->first != 0 || n > dk->count) return SNARKV_ERR_LENGTH;
  const bool validate = (ctx->flags & SNARKV_FLAG_VALIDATE) != 0;
  if (validate && omega32 && !host_canonical(omega32)) {
    set_last_error("ipa_commit: omega is not canonical");
    return SNARKV_ERR_ENCODING;
  }
  SNARKV_HIP(hipSetDevice(ctx->device));
  SNARKV_WIRE_FORM(ctx);
  void *d_s, *d_sm;
  SNARKV_TRY(ctx_reserve(ctx, SLOT_IN_SCALARS, n * 32, &d_s));
  SNARKV_TRY(ctx_reserve(ctx, SLOT_IPA_OUT, 512, &d_sm));
  // SLOT_IPA_OUT: points [MSM, s] | scalars [1, omega] | {0, 2} | {0, n} | bad | out
  uint8_t st[256] = {0};
  if (s64) memcpy(st + 64, s64, 64);
  st[128] = 1;
  if (omega32) memcpy(st + 160, omega32, 32);
  const uint32_t offs[4] = {0, 2, 0, (uint32_t)n};
  memcpy(st + 192, offs, sizeof(offs));
  uint8_t* sm = (uint8_t*)d_sm;
  SNARKV_HIP(hipMemcpyAsync(sm, st, sizeof(st), hipMemcpyHostToDevice, ctx->stream));
  SNARKV_HIP(hipMemcpyAsync(d_s, poly32, n * 32, hipMemcpyHostToDevice, ctx->stream));
  if (validate) {
    int bad = 0;
    SNARKV_TRY(count_bad(ctx, d_s, n, (int*)(sm + 224), &bad));
    if (bad) {
      set_last_error("ipa_commit: %d of %zu scalars are not canonical", bad, n);
      return SNARKV_ERR_ENCODING;
    }
  }
  SNARKV_TRY(ipa_enqueue_commit(ctx, dk->d_points, d_s, n, sm + 200, sm, sm + 128, sm + 192, sm + 256, omega32 != nullptr));
  SNARKV_HIP(hipMemcpyAsync(out64, sm + 256, 64, hipMemcpyDeviceToHost, ctx->stream));
  SNARKV_HIP(hipStreamSynchronize(ctx->stream));
  return SNARKV_OK;
}

// m commitments against the resident key: the shared-key MSM (msm_shared.hip) when the key can have its window table,
// one MSM per vector otherwise (a key over kSharedTableCap, SNARKV_IPA_SHARED=0).  Device to device, enqueued.
static bool commit_shared_never() {
  static const bool never = [] {
    const char* e = getenv("SNARKV_IPA_SHARED");
    return e && *e && atoi(e) == 0;
  }();
  return never;
}

static int commit_batch_run(snarkv_ctx* ctx, const snarkv_ipa_dk* dk, const void* d_polys, size_t n, size_t m,
                            uint32_t slices, void* d_out, uint8_t* d_small) {
  bool shared = false;
  if (!commit_shared_never()) SNARKV_TRY(ipa_dk_table_prepare(ctx, dk, &shared));
  if (shared) return launch_msm_shared(ctx, dk, d_polys, n, m, slices, d_out);
  const uint32_t off[2] = {0, (uint32_t)n};
  SNARKV_HIP(hipMemcpyAsync(d_small + 8, off, sizeof(off), hipMemcpyHostToDevice, ctx->stream));
  SNARKV_HIP(hipStreamSynchronize(ctx->stream));  // `off` lives on this frame
  for (size_t a = 0; a < m; ++a)
    SNARKV_TRY(ipa_msm(ctx, (const uint8_t*)d_polys + 32 * a * n, dk->d_points, n, d_small + 8, (uint8_t*)d_out + 64 * a));
  return SNARKV_OK;
}

static int commit_batch_check(snarkv_ctx* ctx, const snarkv_ipa_dk* dk, const void* polys, size_t n, size_t m, const void* out) {
  if (!ctx || !dk || !polys || !out) return SNARKV_ERR_ARG;
  if (dk->device != ctx->device) return SNARKV_ERR_ARG;
  if (n == 0 || m == 0) return SNARKV_ERR_EMPTY;
  if (dk->first != 0 || n > dk->count) return SNARKV_ERR_LENGTH;
  return SNARKV_OK;
}

// SNARKV_FLAG_VALIDATE over `total` device scalars
static int commit_batch_validate(snarkv_ctx* ctx, const void* d_s, size_t total, uint8_t* d_small) {
  if (!(ctx->flags & SNARKV_FLAG_VALIDATE)) return SNARKV_OK;
  const size_t step = (size_t)1 << 30;
  for (size_t i = 0; i < total; i += step) {
    int bad = 0;
    SNARKV_TRY(count_bad(ctx, (const uint8_t*)d_s + 32 * i, std::min(step, total - i), (int*)d_small, &bad));
    if (bad) {
      set_last_error("ipa_commit_batch: %d scalars are not canonical", bad);
      return SNARKV_ERR_ENCODING;
    }
  }
  return SNARKV_OK;
}

int SNARKV_API(ipa_commit_batch_dev)(snarkv_ctx* ctx, const snarkv_ipa_dk* dk, const void* d_polys32, size_t n, size_t m,
                                     uint32_t slices, void* d_out64s) {
  SNARKV_TRY(commit_batch_check(ctx, dk, d_polys32, n, m, d_out64s));
  SNARKV_HIP(hipSetDevice(ctx->device));
  SNARKV_WIRE_FORM(ctx);
  void* d_sm;
  SNARKV_TRY(ctx_reserve(ctx, SLOT_IPA_OUT, 64, &d_sm));
  SNARKV_TRY(commit_batch_validate(ctx, d_polys32, m * n, (uint8_t*)d_sm));
  return commit_batch_run(ctx, dk, d_polys32, n, m, slices, d_out64s, (uint8_t*)d_sm);
}

// The per-vector route of the blinded batch: the m MSMs write C_a into the point pairs [C_a, S], then ONE segmented launch
// forms 1 C_a + blind_a S for every a.  Staging (SLOT_IPA_H): pairs | scalars [1, blind_a] | offsets {0, 2, .., 2 m} | {0, n}.
static int commit_blinded_per_vector(snarkv_ctx* ctx, const snarkv_ipa_dk* dk, const uint8_t* s64, const void* d_polys, size_t n,
                                     size_t m, const uint8_t* blinds32, void* d_out) {
  const size_t o_sc = 128 * m, o_off = o_sc + 64 * m, o_0n = o_off + 4 * (m + 1), bytes = o_0n + 8;
  std::vector<uint8_t> st(bytes, 0);
  for (size_t a = 0; a < m; ++a) {
    memcpy(&st[128 * a + 64], s64, 64);
    st[o_sc + 64 * a] = 1;
    memcpy(&st[o_sc + 64 * a + 32], blinds32 + 32 * a, 32);
  }
  for (size_t a = 0; a <= m; ++a) {
    const uint32_t o = (uint32_t)(2 * a);
    memcpy(&st[o_off + 4 * a], &o, 4);
  }
  const uint32_t off0n[2] = {0, (uint32_t)n};
  memcpy(&st[o_0n], off0n, sizeof(off0n));
  void* d;
  SNARKV_TRY(ctx_reserve(ctx, SLOT_IPA_H, bytes, &d));
  uint8_t* d_st = (uint8_t*)d;
  SNARKV_HIP(hipMemcpyAsync(d_st, st.data(), bytes, hipMemcpyHostToDevice, ctx->stream));
  SNARKV_HIP(hipStreamSynchronize(ctx->stream));  // `st` lives on this frame (as commit_batch_run's offsets do)
  for (size_t a = 0; a < m; ++a)
    SNARKV_TRY(ipa_msm(ctx, (const uint8_t*)d_polys + 32 * a * n, dk->d_points, n, d_st + o_0n, d_st + 128 * a));
  return launch_msm_batched(ctx, d_st + o_sc, d_st, d_st + o_off, m, 2 * m, d_out);
}

int SNARKV_API(ipa_commit_blinded_batch_dev)(snarkv_ctx* ctx, const snarkv_ipa_dk* dk, const uint8_t s64[64],
                                             const void* d_polys32, size_t n, size_t m, const uint8_t* blinds32,
                                             uint32_t slices, void* d_out64s) {
  if (!s64 || !blinds32) return SNARKV_ERR_ARG;
  SNARKV_TRY(commit_batch_check(ctx, dk, d_polys32, n, m, d_out64s));
  if (m > ((size_t)1 << 24)) return SNARKV_ERR_LENGTH;  // the staging of the blinds is one buffer
  bool s_zero = true;
  for (int i = 0; i < 64; ++i) s_zero = s_zero && s64[i] == 0;
  if (s_zero) {
    set_last_error("ipa_commit_blinded_batch: S is the point at infinity");
    return SNARKV_ERR_ENCODING;
  }
  const bool validate = (ctx->flags & SNARKV_FLAG_VALIDATE) != 0;
  if (validate)
    for (size_t a = 0; a < m; ++a)
      if (!host_canonical(blinds32 + 32 * a)) {
        set_last_error("ipa_commit_blinded_batch: blind %zu is not canonical", a);
        return SNARKV_ERR_ENCODING;
      }
  SNARKV_HIP(hipSetDevice(ctx->device));
  SNARKV_WIRE_FORM(ctx);
  void* d_sm;
  SNARKV_TRY(ctx_reserve(ctx, SLOT_IPA_OUT, 128, &d_sm));
  if (validate) {  // S as every point under the flag: canonical coordinates, on the curve
    int bad = 0;
    SNARKV_HIP(hipMemcpyAsync((uint8_t*)d_sm + 64, s64, 64, hipMemcpyHostToDevice, ctx->stream));
    SNARKV_TRY(launch_validate(ctx, nullptr, (uint8_t*)d_sm + 64, 1, &bad));
    if (bad) {
      set_last_error("ipa_commit_blinded_batch: S is not a canonical point of the curve");
      return SNARKV_ERR_ENCODING;
    }
  }
  SNARKV_TRY(commit_batch_validate(ctx, d_polys32, m * n, (uint8_t*)d_sm));
  bool shared = false;
  if (!commit_shared_never()) SNARKV_TRY(ipa_dk_table_prepare(ctx, dk, &shared));
  if (!shared) return commit_blinded_per_vector(ctx, dk, s64, d_polys32, n, m, blinds32, d_out64s);
  // the blinds through a buffer of this frame: pageable memory, which the transfer has left when hipMemcpyAsync returns
  // (session_open's `st`), whatever memory the caller's are in
  std::vector<uint8_t> st(blinds32, blinds32 + 32 * m);
  void* d_bl;
  SNARKV_TRY(ctx_reserve(ctx, SLOT_IPA_XI, 32 * m, &d_bl));
  SNARKV_HIP(hipMemcpyAsync(d_bl, st.data(), st.size(), hipMemcpyHostToDevice, ctx->stream));
  return launch_msm_shared_blinded(ctx, dk, d_polys32, n, m, slices, d_bl, s64, d_out64s);
}

int SNARKV_API(ipa_commit_batch)(snarkv_ctx* ctx, const snarkv_ipa_dk* dk, const uint8_t* polys32, size_t n, size_t m,
                                 uint8_t* out64s) {
  SNARKV_TRY(commit_batch_check(ctx, dk, polys32, n, m, out64s));
  SNARKV_HIP(hipSetDevice(ctx->device));
  SNARKV_WIRE_FORM(ctx);
  // vectors are staged in groups of bounded size, so m x n is unbounded
  const size_t cap = (size_t)64 << 20;
  const size_t group = std::min(m, std::max<size_t>(1, cap / (n * 32)));
  void *d_s, *d_o, *d_sm;
  SNARKV_TRY(ctx_reserve(ctx, SLOT_IN_SCALARS, group * n * 32, &d_s));
  SNARKV_TRY(ctx_reserve(ctx, SLOT_OUT, group * 64, &d_o));
  SNARKV_TRY(ctx_reserve(ctx, SLOT_IPA_OUT, 64, &d_sm));
  for (size_t a0 = 0; a0 < m; a0 += group) {
    const size_t g = std::min(group, m - a0);
    SNARKV_HIP(hipMemcpyAsync(d_s, polys32 + 32 * a0 * n, g * n * 32, hipMemcpyHostToDevice, ctx->stream));
    SNARKV_TRY(commit_batch_validate(ctx, d_s, g * n, (uint8_t*)d_sm));
    SNARKV_TRY(commit_batch_run(ctx, dk, d_s, n, g, 0, d_o, (uint8_t*)d_sm));
    SNARKV_HIP(hipMemcpyAsync(out64s + 64 * a0, d_o, g * 64, hipMemcpyDeviceToHost, ctx->stream));
    SNARKV_HIP(hipStreamSynchronize(ctx->stream));
  }
  return SNARKV_OK;
}

int SNARKV_API(ipa_prover_begin)(snarkv_ctx* ctx, const snarkv_ipa_dk* dk, const uint8_t* coeffs32, size_t n,
                                 const uint8_t z32[32], const uint8_t h64[64], const uint8_t xi0_32[32],
                                 snarkv_ipa_prover** out) {
  return prover_begin(ctx, dk, coeffs32, false, n, z32, h64, xi0_32, out);
}

int SNARKV_API(ipa_prover_begin_dev)(snarkv_ctx* ctx, const snarkv_ipa_dk* dk, const void* d_coeffs32, size_t n,
                                     const uint8_t z32[32], const uint8_t h64[64], const uint8_t xi0_32[32],
                                     snarkv_ipa_prover** out) {
  return prover_begin(ctx, dk, d_coeffs32, true, n, z32, h64, xi0_32, out);
}

int SNARKV_API(ipa_prover_round)(snarkv_ipa_prover* p, uint8_t l64[64], uint8_t r64[64]) {
  if (!l64 || !r64) return SNARKV_ERR_ARG;
  SNARKV_TRY(session_check(p, snarkv_ipa_prover::WANT_ROUND));
  const int rc = prover_round(p, l64, r64);
  p->state = rc == SNARKV_OK ? snarkv_ipa_prover::WANT_FOLD : snarkv_ipa_prover::FAILED;
  return rc;
}

int SNARKV_API(ipa_prover_fold)(snarkv_ipa_prover* p, const uint8_t xi32[32]) {
  if (!xi32) return SNARKV_ERR_ARG;
  SNARKV_TRY(session_check(p, snarkv_ipa_prover::WANT_FOLD));
  if ((p->ctx->flags & SNARKV_FLAG_VALIDATE) && !host_canonical(xi32)) {
    set_last_error("ipa_prover_fold: xi is not canonical");
    return SNARKV_ERR_ENCODING;  // nothing was folded: the session still wants this fold
  }
  memcpy(p->xi_host, xi32, 32);
  const int rc = prover_fold(p);
  if (rc != SNARKV_OK) {
    p->state = snarkv_ipa_prover::FAILED;
    return rc;
  }
  p->rounds += 1;
  p->state = p->rounds == p->k ? snarkv_ipa_prover::DONE : snarkv_ipa_prover::WANT_ROUND;
  return SNARKV_OK;
}

int SNARKV_API(ipa_prover_finish)(snarkv_ipa_prover* p, uint8_t u64[64], uint8_t c32[32]) {
  if (!u64 || !c32) return SNARKV_ERR_ARG;
  SNARKV_TRY(session_check(p, snarkv_ipa_prover::DONE));
  snarkv_ctx* ctx = p->ctx;
  int rc = SNARKV_OK;
  if (hipSetDevice(ctx->device) != hipSuccess ||
      hipMemcpyAsync(u64, p->d_bases, 64, hipMemcpyDeviceToHost, ctx->stream) != hipSuccess ||
      hipMemcpyAsync(c32, p->d_coeffs, 32, hipMemcpyDeviceToHost, ctx->stream) != hipSuccess ||
      hipStreamSynchronize(ctx->stream) != hipSuccess) {
    set_last_error("ipa_prover_finish: %s", hipGetErrorString(hipGetLastError()));
    rc = SNARKV_ERR_DEVICE;
    p->state = snarkv_ipa_prover::FAILED;
  }
  return rc;
}

void SNARKV_API(ipa_prover_destroy)(snarkv_ipa_prover* p) {
  if (!p) return;
  session_close(p);  // waits: enqueued folds may still read the buffers
}

int SNARKV_API(ipa_as_combine_dev)(snarkv_ctx* ctx, const uint8_t* xi32, size_t m, uint32_t k, const uint8_t alpha32[32],
                                   const uint8_t* ab64, void* d_h32) {
  if (!ctx || !xi32 || !alpha32 || !d_h32) return SNARKV_ERR_ARG;
  if (reinterpret_cast<uintptr_t>(d_h32) % 16) return SNARKV_ERR_ARG;  // 16-byte stores
  if (m == 0) return SNARKV_ERR_EMPTY;
  if (k < 1 || k > 28 || m > (1u << 20)) return SNARKV_ERR_LENGTH;
  if (ctx->flags & SNARKV_FLAG_VALIDATE) {
    bool ok = host_canonical(alpha32) && (!ab64 || (host_canonical(ab64) && host_canonical(ab64 + 32)));
    for (size_t i = 0; ok && i < m * k; ++i) ok = host_canonical(xi32 + 32 * i);
    if (!ok) {
      set_last_error("ipa_as_combine: a scalar is not canonical");
      return SNARKV_ERR_ENCODING;
    }
  }
  SNARKV_HIP(hipSetDevice(ctx->device));
  SNARKV_WIRE_FORM(ctx);
  const size_t count = m * k;
  void *d_xi, *d_x29, *d_sm;
  SNARKV_TRY(ctx_reserve(ctx, SLOT_IPA_XI, count * 32, &d_xi));
  SNARKV_TRY(ctx_reserve(ctx, SLOT_IPA_H, count * sizeof(Fr29), &d_x29));
  SNARKV_TRY(ctx_reserve(ctx, SLOT_IPA_OUT, 96, &d_sm));
  uint8_t st[96] = {0};
  memcpy(st, alpha32, 32);
  if (ab64) memcpy(st + 32, ab64, 64);
  SNARKV_HIP(hipMemcpyAsync(d_xi, xi32, count * 32, hipMemcpyHostToDevice, ctx->stream));
  SNARKV_HIP(hipMemcpyAsync(d_sm, st, sizeof(st), hipMemcpyHostToDevice, ctx->stream));
  hipLaunchKernelGGL(k_ipa_as_prep, dim3((uint32_t)((count + 255) / 256)), dim3(256), 0, ctx->stream,
                     (const uint32_t*)d_xi, (uint32_t)count, (Fr29*)d_x29);
  const size_t n = (size_t)1 << k;
  hipLaunchKernelGGL(k_ipa_as_combine, dim3((uint32_t)((n + 255) / 256)), dim3(256), 0, ctx->stream,
                     (const Fr29*)d_x29, (uint32_t)m, k, (const uint32_t*)d_sm, ab64 ? 1u : 0u, (uint32_t*)d_h32);
  SNARKV_HIP(hipGetLastError());
  SNARKV_HIP(hipStreamSynchronize(ctx->stream));  // the staged inputs live on this stack frame
  return SNARKV_OK;
}

}  // extern "C"
