// Polynomials over the scalar field in device memory (include/snarkv_poly.h): linear combination, evaluation, division by a
// linear factor.  Same source for both curves, as ipa_create.hip.
//
// Division and evaluation are the blocked scan of poly_scan.h with B = 256, one coefficient per thread:
//   k_poly_scan    phase 1 of one level: the block's suffix sums by 8 steps through LDS (two buffers of 256 Fr29, one
//                  barrier per step), the block's total to the level above, a^256 as that level's root
//   k_poly_apply   phase 3 of one level: c_i = s_i + a^(256 - lane) carry_b for every block but the last
// Phase 2 is the same pair one level up, on the totals in place: 2^30 coefficients take four levels.  Values travel between
// kernels as canonical words, so that a level's totals are a polynomial like any other.  The evaluation runs phase 1 only and
// keeps the totals: p(a) = sum_b T_b (a^256)^b.
#include <string.h>
#include <algorithm>
#include "poly.hpp"
#include "poly_args.hpp"
#include "ipa_prover.hpp"
#include "poly_scan.h"
#include "../../include/snarkv_poly.h"

namespace snarkv {

using Scan = PolyScan<kPolyBlock>;
constexpr uint32_t kPolyLevels = 5;  // 256^4 >= 2^30: levels 0..3 hold more than one coefficient, level 4 would hold one

// layout of the context's SLOT_POLY
enum : size_t {
  PS_ROOTS = 0,       // the root of each level: a, a^256, a^65536, ...     kPolyLevels x 32
  PS_LC_IDX = 256,    // the staged pass of the linear combination: indices  kPolyLincombTerms x 4
  PS_LC_SC = 512,     // ... and scalars                                    kPolyLincombTerms x 32
  PS_LEVELS = 2048,   // the totals of level 1, 2, ...: 32 bytes each
};

// the address of c_i: c_0 has a place of its own (the remainder), c_i the i-1'th place of the sequence
__device__ __forceinline__ uint32_t* scan_slot(uint32_t* out0, uint32_t* out1, uint32_t i) {
  return i == 0 ? out0 : out1 + 8 * (size_t)(i - 1);
}

template <bool STORE>
__global__ void __launch_bounds__(kPolyBlock) k_poly_scan(const uint32_t* in, uint32_t n, const uint32_t* __restrict__ root,
                                                          uint32_t* out0, uint32_t* out1, uint32_t* __restrict__ totals,
                                                          uint32_t* __restrict__ next_root) {  // a level above 0 runs in place
  __shared__ Fr29 sh[2][kPolyBlock];
  const uint32_t lane = threadIdx.x, b = blockIdx.x, i = b * kPolyBlock + lane;
  const uint32_t len = Scan::block_len(b, n);
  Fr29 a_pow = ld_fr(root);
  Fr29 s = lane < len ? ld_fr(in + 8 * (size_t)i) : fr29_zero();
#pragma unroll 1
  for (uint32_t step = 0; step < Scan::steps(); ++step) {
    sh[step & 1u][lane] = s;
    __syncthreads();
    if (Scan::has_partner(lane, step, len)) s = poly_scan_step(s, sh[step & 1u][lane + Scan::distance(step)], a_pow, step);
    a_pow = fr29_mul(a_pow, a_pow);
  }
  if (STORE && lane < len) st_fr(scan_slot(out0, out1, i), s);
  if (lane == 0) {
    if (totals) st_fr(totals + 8 * (size_t)b, s);
    if (b == 0 && next_root) st_fr(next_root, a_pow);  // a^256
  }
}

// launched over the blocks that have a carry: all but the last, every one of them full
__global__ void __launch_bounds__(kPolyBlock) k_poly_apply(uint32_t* out0, uint32_t* out1,
                                                           const uint32_t* __restrict__ root,
                                                           const uint32_t* __restrict__ carries) {
  constexpr uint32_t kBits = 9;  // carry_exp is in [1, 256]
  __shared__ Fr29 sq[kBits];
  const uint32_t lane = threadIdx.x, b = blockIdx.x, i = b * kPolyBlock + lane;
  if (lane == 0) {
    Fr29 x = ld_fr(root);
    for (uint32_t j = 0; j < kBits; ++j) {
      sq[j] = x;
      x = fr29_mul(x, x);
    }
  }
  __syncthreads();
  const Fr29 w = poly_scan_pow(sq, Scan::carry_exp(lane), kBits);
  uint32_t* p = scan_slot(out0, out1, i);
  st_fr(p, poly_scan_apply(ld_fr(p), w, ld_fr(carries + 8 * (size_t)Scan::carry_index(b))));
}

// the 9 x 29-bit limbs of 8 words, as they stand (not yet in the Montgomery domain)
__device__ __forceinline__ Fr29 ld_raw(const uint32_t* __restrict__ p) {
  const uint4* s = reinterpret_cast<const uint4*>(p);
  const uint4 a = s[0], b = s[1];
  const uint32_t w[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
  return fr29_limbs_of_words(w);
}

// out[i] (+)= sum_{j < count} scalars[j] polys[idx[j]][i], count <= kPolyLincombTerms.  The scalars go to LDS as s R^2, so
// that one product with a coefficient's raw limbs (< 2^256 < 8r) is the term in the Montgomery domain.  The sum is lazy: a
// product is within (-r/2, 3r/2), what is accumulated from an earlier pass too; after every fourth term, (-5r/2, 15r/2) at
// most, a product by one brings the sum back to (-r/8, 9r/8), and the up to three terms after the last one leave it below
// the 8r that fr29_to_canonical takes.  The limbs are carry-normalised after every term: five normalised values added limb
// by limb would pass 2^31.
__global__ void __launch_bounds__(256) k_poly_lincomb(const uint32_t* __restrict__ polys, uint32_t n,
                                                      const uint32_t* __restrict__ idx, const uint32_t* __restrict__ scalars,
                                                      uint32_t count, uint32_t accumulate, uint32_t* __restrict__ out) {
  __shared__ Fr29 sc[kPolyLincombTerms];
  __shared__ uint32_t ix[kPolyLincombTerms];
  if (threadIdx.x < count) {
    constexpr int32_t r2[9] = SNARKV_FR29_R2_LIMBS;
    Fr29 m;
#pragma unroll
    for (int i = 0; i < 9; ++i) m.v[i] = r2[i];
    sc[threadIdx.x] = fr29_mul(ld_fr(scalars + 8 * threadIdx.x), m);
    ix[threadIdx.x] = idx[threadIdx.x];
  }
  __syncthreads();
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= n) return;
  Fr29 acc = accumulate ? ld_fr(out + 8 * (size_t)i) : fr29_zero();
#pragma unroll 1
  for (uint32_t j = 0; j < count; ++j) {
    acc = fr29_norm(fr29_add(acc, fr29_mul(ld_raw(polys + 8 * ((size_t)ix[j] * n + i)), sc[j])));
    if ((j & 3u) == 3u) acc = fr29_mul(acc, fr29_one());
  }
  st_fr(out + 8 * (size_t)i, acc);
}

namespace {

struct Levels {
  uint32_t count;               // levels that run (the last one has a single block)
  uint32_t len[kPolyLevels];    // coefficients of each
  size_t off[kPolyLevels + 1];  // where level l >= 1 lies in SLOT_POLY
};

Levels levels_of(size_t n) {
  Levels lv;
  lv.count = 0;
  size_t off = PS_LEVELS, m = n;
  for (;;) {
    lv.len[lv.count] = (uint32_t)m;
    lv.off[lv.count] = off;  // unused for level 0
    lv.count += 1;
    if (Scan::blocks((uint32_t)m) == 1) break;
    m = Scan::blocks((uint32_t)m);
    if (lv.count > 1) off += 32 * (size_t)lv.len[lv.count - 1];
  }
  lv.off[lv.count] = lv.count == 1 ? off : off + 32 * (size_t)lv.len[lv.count - 1];
  return lv;
}

// the scan of every level, bottom up; `store`: the suffix sums are kept (division), or only the totals (evaluation, whose
// result the last level writes to `d_rem`)
int scan_levels(snarkv_ctx* ctx, const void* d_coeffs, size_t n, const void* d_root, void* d_quot, void* d_rem, bool store) {
  const Levels lv = levels_of(n);
  void* d_scr;
  SNARKV_TRY(ctx_reserve(ctx, SLOT_POLY, lv.off[lv.count], &d_scr));
  uint8_t* scr = (uint8_t*)d_scr;
  hipStream_t s = ctx->stream;
  auto root_of = [&](uint32_t l) { return l == 0 ? (const uint32_t*)d_root : (const uint32_t*)(scr + PS_ROOTS + 32 * l); };
  auto seq_of = [&](uint32_t l) { return (uint32_t*)(scr + lv.off[l]); };  // l >= 1
  for (uint32_t l = 0; l < lv.count; ++l) {
    const bool last = l + 1 == lv.count;
    const uint32_t* in = l == 0 ? (const uint32_t*)d_coeffs : seq_of(l);
    uint32_t* out0 = l == 0 ? (uint32_t*)d_rem : seq_of(l);
    uint32_t* out1 = l == 0 ? (uint32_t*)d_quot : seq_of(l) + 8;
    uint32_t* totals = last ? (store ? nullptr : (uint32_t*)d_rem) : seq_of(l + 1);
    uint32_t* next_root = last ? nullptr : (uint32_t*)(scr + PS_ROOTS + 32 * (l + 1));
    const dim3 grid(Scan::blocks(lv.len[l]));
    if (store)
      hipLaunchKernelGGL(k_poly_scan<true>, grid, dim3(kPolyBlock), 0, s, in, lv.len[l], root_of(l), out0, out1, totals, next_root);
    else
      hipLaunchKernelGGL(k_poly_scan<false>, grid, dim3(kPolyBlock), 0, s, in, lv.len[l], root_of(l), (uint32_t*)nullptr,
                         (uint32_t*)nullptr, totals, next_root);
  }
  SNARKV_HIP(hipGetLastError());
  if (!store) return SNARKV_OK;
  for (uint32_t l = lv.count - 1; l-- > 0;) {  // the carries of level l are the scanned sequence of level l + 1
    uint32_t* out0 = l == 0 ? (uint32_t*)d_rem : seq_of(l);
    uint32_t* out1 = l == 0 ? (uint32_t*)d_quot : seq_of(l) + 8;
    hipLaunchKernelGGL(k_poly_apply, dim3(Scan::blocks(lv.len[l]) - 1), dim3(kPolyBlock), 0, s, out0, out1, root_of(l),
                       (const uint32_t*)seq_of(l + 1));
  }
  SNARKV_HIP(hipGetLastError());
  return SNARKV_OK;
}

}  // namespace

int poly_enqueue_eval(snarkv_ctx* ctx, const void* d_coeffs, size_t n, const void* d_point, void* d_out) {
  return scan_levels(ctx, d_coeffs, n, d_point, nullptr, d_out, false);
}

int poly_enqueue_div_linear(snarkv_ctx* ctx, const void* d_coeffs, size_t n, const void* d_root, void* d_quot, void* d_rem) {
  return scan_levels(ctx, d_coeffs, n, d_root, d_quot, d_rem, true);
}

int poly_enqueue_lincomb(snarkv_ctx* ctx, const void* d_polys, size_t n, const uint32_t* idx, const uint8_t* scalars32,
                         size_t count, void* d_out) {
  void* d_scr;
  SNARKV_TRY(ctx_reserve(ctx, SLOT_POLY, PS_LEVELS, &d_scr));
  uint8_t* scr = (uint8_t*)d_scr;
  for (size_t j0 = 0; j0 < count; j0 += kPolyLincombTerms) {
    const size_t c = std::min<size_t>(kPolyLincombTerms, count - j0);
    // host arrays in pageable memory: the copies have left them when hipMemcpyAsync returns
    SNARKV_HIP(hipMemcpyAsync(scr + PS_LC_IDX, idx + j0, 4 * c, hipMemcpyHostToDevice, ctx->stream));
    SNARKV_HIP(hipMemcpyAsync(scr + PS_LC_SC, scalars32 + 32 * j0, 32 * c, hipMemcpyHostToDevice, ctx->stream));
    hipLaunchKernelGGL(k_poly_lincomb, dim3((uint32_t)((n + 255) / 256)), dim3(256), 0, ctx->stream, (const uint32_t*)d_polys,
                       (uint32_t)n, (const uint32_t*)(scr + PS_LC_IDX), (const uint32_t*)(scr + PS_LC_SC), (uint32_t)c,
                       j0 ? 1u : 0u, (uint32_t*)d_out);
    SNARKV_HIP(hipGetLastError());
  }
  return SNARKV_OK;
}

}  // namespace snarkv

using namespace snarkv;

extern "C" {

int SNARKV_API(poly_lincomb_dev)(snarkv_ctx* ctx, const void* d_polys32, size_t n, size_t n_polys, const uint32_t* idx,
                                 const uint8_t* scalars32, size_t count, void* d_out32) {
  if (!ctx || !idx || !scalars32 || !aligned16(d_polys32) || !aligned16(d_out32)) return SNARKV_ERR_ARG;
  SNARKV_TRY(check_len(n, kPolyMaxLen));
  if (count == 0 || n_polys == 0) return SNARKV_ERR_EMPTY;
  const bool none_ok = false;
  const void* const out = d_out32;
  const size_t out_bytes = 32 * n;
  SNARKV_TRY(check_columns("poly_lincomb", d_polys32, n, n_polys, &idx, 1, &none_ok, count, &out, &out_bytes, 1));
  SNARKV_HIP(hipSetDevice(ctx->device));
  return poly_enqueue_lincomb(ctx, d_polys32, n, idx, scalars32, count, d_out32);
}

int SNARKV_API(poly_eval_dev)(snarkv_ctx* ctx, const void* d_coeffs32, size_t n, const void* d_point32, void* d_out32) {
  if (!ctx || !aligned16(d_coeffs32) || !aligned16(d_point32) || !aligned16(d_out32)) return SNARKV_ERR_ARG;
  SNARKV_TRY(check_len(n, kPolyMaxLen));
  SNARKV_HIP(hipSetDevice(ctx->device));
  return poly_enqueue_eval(ctx, d_coeffs32, n, d_point32, d_out32);
}

int SNARKV_API(poly_div_linear_dev)(snarkv_ctx* ctx, const void* d_coeffs32, size_t n, const void* d_root32, void* d_quot32,
                                    void* d_rem32) {
  if (!ctx || !aligned16(d_coeffs32) || !aligned16(d_root32) || !aligned16(d_rem32)) return SNARKV_ERR_ARG;
  SNARKV_TRY(check_len(n, kPolyMaxLen));
  if (n > 1 && !aligned16(d_quot32)) return SNARKV_ERR_ARG;
  const size_t qn = 32 * (n - 1);
  if (overlap(d_quot32, qn, d_coeffs32, 32 * n) || overlap(d_rem32, 32, d_coeffs32, 32 * n) || overlap(d_rem32, 32, d_quot32, qn) ||
      overlap(d_root32, 32, d_quot32, qn) || overlap(d_root32, 32, d_rem32, 32)) {
    set_last_error("poly_div_linear: the quotient and the remainder may not overlap the coefficients, the root or each other");
    return SNARKV_ERR_ARG;
  }
  SNARKV_HIP(hipSetDevice(ctx->device));
  return poly_enqueue_div_linear(ctx, d_coeffs32, n, d_root32, d_quot32, d_rem32);
}

}  // extern "C"
