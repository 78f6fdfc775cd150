// Products along columns of scalars in device memory (include/snarkv_poly_prod.h): the pointwise product, the product of
// affine terms, the batch inversion, the grand product and the permutation argument's Z made of the four.  Same source for
// both curves, as poly.hip.
//
// The grand product and the batch inversion are the blocked scans of poly_prod.h over levels: 256 lanes per workgroup, four
// elements per lane on the data (level 0, kProdBlock = 1024), one on the totals (kProdLevelBlock = 256), so 2^30 elements
// take four levels.  Bottom up only block totals are written; top down a workgroup recomputes its prefixes (and suffixes)
// from what it reads and writes its block once, after the barriers of its scan: in place is safe by construction.
//   k_prod_up     the total of a block (zeros taken as one for the inversion's level 0) to the level above
//   k_prod_down   out_i = carry_b x_0 .. x_{i-1}; the top level's carry is the start value, its last lane writes the total
//   k_inv_down    out_i = P_{i-1} S_{i+1} w_b; the top level inverts its total (one Fermat chain on one lane per call)
// Values travel between kernels as canonical words, so that a level's totals are a column like any other.
#include <string.h>
#include <algorithm>
#include <vector>
#include "ctx.hpp"
#include "ipa_prover.hpp"
#include "poly_args.hpp"
#include "poly_prod.h"
#include "../../include/snarkv_poly_prod.h"

namespace snarkv {

constexpr uint32_t kProdThreads = 256;
constexpr uint32_t kProdLane = 4;                               // elements per lane at level 0
constexpr uint32_t kProdBlock = kProdThreads * kProdLane;       // elements per workgroup at level 0
constexpr uint32_t kProdLevelBlock = kProdThreads;              // ... at the levels above
constexpr uint32_t kProdAffineTerms = 16;                       // terms per pass of the affine product
constexpr uint32_t kProdLevels = 4;                             // 1024 * 256 * 256 >= 2^30: levels 0..3
constexpr size_t kProdMaxLen = (size_t)1 << 30;

// layout of the context's SLOT_POLY_PROD
enum : size_t {
  PP_IDX_A = 0,      // the staged pass of the affine product: indices        kProdAffineTerms x 4, twice
  PP_IDX_B = 64,
  PP_BETA = 128,     // ... and scalars                                       kProdAffineTerms x 32, twice
  PP_GAMMA = 640,
  PP_LEVELS = 2048,  // the totals of level 1, 2, ...: 32 bytes each
};
static_assert(PP_IDX_B - PP_IDX_A >= 4 * kProdAffineTerms && PP_GAMMA - PP_BETA >= 32 * kProdAffineTerms &&
              PP_LEVELS - PP_GAMMA >= 32 * kProdAffineTerms, "the staged pass fits its places");

// the E elements of lane `lane` of block b; one where the sequence has ended
template <uint32_t T, uint32_t E>
__device__ __forceinline__ void load_lane(const uint32_t* in, uint32_t b, uint32_t lane, uint32_t len, Fr29* x) {
  typedef ProdBlock<T, E> S;
#pragma unroll
  for (uint32_t j = 0; j < E; ++j) x[j] = S::has(lane, j, len) ? ld_fr(in + 8 * (size_t)S::index(b, lane, j)) : fr29_one();
}
template <uint32_t T, uint32_t E>
__device__ __forceinline__ void store_lane(uint32_t* out, uint32_t b, uint32_t lane, uint32_t len, const Fr29* v) {
  typedef ProdBlock<T, E> S;
#pragma unroll
  for (uint32_t j = 0; j < E; ++j)
    if (S::has(lane, j, len)) st_fr(out + 8 * (size_t)S::index(b, lane, j), v[j]);
}
template <uint32_t E>
__device__ __forceinline__ void zeros_to_one(Fr29* x, bool* zero) {
#pragma unroll
  for (uint32_t j = 0; j < E; ++j) {
    zero[j] = prod_is_zero(x[j]);
    if (zero[j]) x[j] = fr29_one();
  }
}

template <uint32_t T, uint32_t E, bool NZ>
__global__ void __launch_bounds__(T) k_prod_up(const uint32_t* __restrict__ in, uint32_t n, uint32_t* __restrict__ totals) {
  typedef ProdBlock<T, E> S;
  __shared__ Fr29 sh[2][T];
  const uint32_t lane = threadIdx.x, b = blockIdx.x, len = S::block_len(b, n);
  Fr29 x[E], p[E], total;
  bool zero[E];
  load_lane<T, E>(in, b, lane, len, x);
  if (NZ) zeros_to_one<E>(x, zero);
  prod_lane_prefix<E>(x, p, total);
  const Fr29 s = wg_scan<ProdStep, false>(sh, total, lane);
  if (lane == T - 1) st_fr(totals + 8 * (size_t)b, s);
}

// `in` may be `out`.  carries: one value per block (stride 1), one for the only block (stride 0), or none (one)
template <uint32_t T, uint32_t E>
__global__ void __launch_bounds__(T) k_prod_down(const uint32_t* in, uint32_t n, const uint32_t* carries, uint32_t stride,
                                                 uint32_t* out, uint32_t* total_out) {
  typedef ProdBlock<T, E> S;
  __shared__ Fr29 sh[2][T];
  const uint32_t lane = threadIdx.x, b = blockIdx.x, len = S::block_len(b, n);
  Fr29 x[E], p[E], total;
  load_lane<T, E>(in, b, lane, len, x);
  const Fr29 carry = carries ? ld_fr(carries + 8 * (size_t)b * stride) : fr29_one();
  prod_lane_prefix<E>(x, p, total);
  const Fr29 s = wg_scan<ProdStep, false>(sh, total, lane);
  wg_publish(sh, s, lane);
  const Fr29 before = lane ? fr29_mul(carry, sh[0][lane - 1]) : carry;
  prod_lane_outputs<E>(before, p, x);
  store_lane<T, E>(out, b, lane, len, x);
  if (total_out && lane == T - 1 && b + 1 == gridDim.x) st_fr(total_out, fr29_mul(carry, s));
}

// `in` may be `out`.  TOP: the only block of the last level, which inverts its own total; otherwise w[b] = 1 / T_b
template <uint32_t T, uint32_t E, bool NZ, bool TOP>
__global__ void __launch_bounds__(T) k_inv_down(const uint32_t* in, uint32_t n, const uint32_t* w, uint32_t* out) {
  typedef ProdBlock<T, E> S;
  __shared__ Fr29 sh[2][T];
  __shared__ Fr29 w_top;
  const uint32_t lane = threadIdx.x, b = blockIdx.x, len = S::block_len(b, n);
  Fr29 x[E], m[E], total;
  bool zero[E];
  load_lane<T, E>(in, b, lane, len, x);
  if (NZ) {
    zeros_to_one<E>(x, zero);
  } else {
#pragma unroll
    for (uint32_t j = 0; j < E; ++j) zero[j] = false;
  }
  prod_lane_others<E>(x, m, total);
  const Fr29 left = wg_scan<ProdStep, false>(sh, total, lane);
  wg_publish(sh, left, lane);
  Fr29 around = lane ? sh[0][lane - 1] : fr29_one();
  if (TOP) {
    if (lane == T - 1) w_top = prod_inv(left);  // the block's total, never zero
  }
  const Fr29 right = wg_scan<ProdStep, true>(sh, total, lane);
  wg_publish(sh, right, lane);  // its barriers also publish w_top
  if (lane + 1 < T) around = fr29_mul(around, sh[0][lane + 1]);
  around = fr29_mul(around, TOP ? w_top : ld_fr(w + 8 * (size_t)b));
  prod_lane_inverses<E>(around, m, zero, x);
  store_lane<T, E>(out, b, lane, len, x);
}

// out[i] = a[i] b[i]; out may be a or b: every element is read by the thread that writes it
__global__ void __launch_bounds__(256) k_prod_mul(const uint32_t* a, const uint32_t* b, uint32_t n, uint32_t* out) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= n) return;
  st_fr(out + 8 * (size_t)i, fr29_mul(ld_fr(a + 8 * (size_t)i), ld_fr(b + 8 * (size_t)i)));
}

__device__ __forceinline__ Fr29 ld_raw(const uint32_t* __restrict__ p) {
  const uint4* s = reinterpret_cast<const uint4*>(p);
  const uint4 a = s[0], b = s[1];
  const uint32_t w[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
  return prod_raw(w);
}

// out[i] (*)= prod_{j < count} (polys[ia[j]][i] + beta_j polys[ib[j]][i] + gamma_j), count <= kProdAffineTerms.  The scalars
// go to LDS in the Montgomery domain (beta as beta R^2, for the raw limbs of its column); the bound of a term is at
// prod_affine_term, the running product is a bare one.
__global__ void __launch_bounds__(256) k_prod_affine(const uint32_t* __restrict__ polys, uint32_t n,
                                                     const uint32_t* __restrict__ idx_a, const uint32_t* __restrict__ idx_b,
                                                     const uint32_t* __restrict__ betas, const uint32_t* __restrict__ gammas,
                                                     uint32_t count, uint32_t accumulate, uint32_t* __restrict__ out) {
  __shared__ Fr29 sb[kProdAffineTerms], sg[kProdAffineTerms];
  __shared__ uint32_t ia[kProdAffineTerms], ib[kProdAffineTerms];
  if (threadIdx.x < count) {
    sb[threadIdx.x] = prod_scalar_for_raw(ld_fr(betas + 8 * threadIdx.x));
    sg[threadIdx.x] = ld_fr(gammas + 8 * threadIdx.x);
    ia[threadIdx.x] = idx_a[threadIdx.x];
    ib[threadIdx.x] = idx_b[threadIdx.x];
  }
  __syncthreads();
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= n) return;
  Fr29 acc = accumulate ? ld_fr(out + 8 * (size_t)i) : fr29_one();
#pragma unroll 1
  for (uint32_t j = 0; j < count; ++j) {
    const Fr29 a = ld_fr(polys + 8 * ((size_t)ia[j] * n + i));
    const Fr29 t = ib[j] == SNARKV_POLY_NONE ? prod_affine_term(a, sg[j])
                                             : prod_affine_term(a, ld_raw(polys + 8 * ((size_t)ib[j] * n + i)), sb[j], sg[j]);
    acc = fr29_mul(acc, t);
  }
  st_fr(out + 8 * (size_t)i, acc);
}

namespace {

uint32_t blocks_at(uint32_t level, uint32_t len) {
  return level == 0 ? ProdBlock<kProdThreads, kProdLane>::blocks(len) : ProdBlock<kProdThreads, 1>::blocks(len);
}

struct Levels {
  uint32_t count;            // levels that run (the last one has a single block)
  uint32_t len[kProdLevels];  // elements of each
  size_t off[kProdLevels];    // where level l >= 1 lies in SLOT_POLY_PROD
  size_t end;
};

Levels levels_of(size_t n) {
  Levels lv;
  lv.count = 0;
  size_t off = PP_LEVELS;
  uint32_t m = (uint32_t)n;
  for (;;) {
    lv.len[lv.count] = m;
    lv.off[lv.count] = off;  // unused for level 0
    if (lv.count > 0) off += 32 * (size_t)m;
    const uint32_t blocks = blocks_at(lv.count, m);
    lv.count += 1;
    if (blocks == 1) break;
    m = blocks;
  }
  lv.end = off;
  return lv;
}

struct Scratch {
  Levels lv;
  uint8_t* scr;
  uint32_t* seq(uint32_t l) const { return (uint32_t*)(scr + lv.off[l]); }  // l >= 1
};

int scratch_of(snarkv_ctx* ctx, size_t n, Scratch* s) {
  s->lv = levels_of(n);
  void* d;
  SNARKV_TRY(ctx_reserve(ctx, SLOT_POLY_PROD, s->lv.end, &d));
  s->scr = (uint8_t*)d;
  return SNARKV_OK;
}

// bottom up: the totals of every level but the last; `nz`: zeros of level 0 count as one
void sweep_up(snarkv_ctx* ctx, const Scratch& s, const void* d_in, bool nz) {
  const dim3 th(kProdThreads);
  for (uint32_t l = 0; l + 1 < s.lv.count; ++l) {
    const dim3 grid(blocks_at(l, s.lv.len[l]));
    if (l > 0)
      hipLaunchKernelGGL((k_prod_up<kProdThreads, 1, false>), grid, th, 0, ctx->stream, (const uint32_t*)s.seq(l), s.lv.len[l],
                         s.seq(l + 1));
    else if (nz)
      hipLaunchKernelGGL((k_prod_up<kProdThreads, kProdLane, true>), grid, th, 0, ctx->stream, (const uint32_t*)d_in, s.lv.len[0],
                         s.seq(1));
    else
      hipLaunchKernelGGL((k_prod_up<kProdThreads, kProdLane, false>), grid, th, 0, ctx->stream, (const uint32_t*)d_in,
                         s.lv.len[0], s.seq(1));
  }
}

}  // namespace

// The enqueue steps; arguments are taken as checked.  Every step reserves the scratch of its own n: inside perm_product the
// first reservation is the largest, so the slot does not move between the steps.

int prod_mul_enqueue(snarkv_ctx* ctx, const void* d_a, const void* d_b, size_t n, void* d_out) {
  hipLaunchKernelGGL(k_prod_mul, dim3((uint32_t)((n + 255) / 256)), dim3(256), 0, ctx->stream, (const uint32_t*)d_a,
                     (const uint32_t*)d_b, (uint32_t)n, (uint32_t*)d_out);
  SNARKV_HIP(hipGetLastError());
  return SNARKV_OK;
}

int prod_affine_enqueue(snarkv_ctx* ctx, const void* d_polys, size_t n, const uint32_t* idx_a, const uint32_t* idx_b,
                        const uint8_t* betas32, const uint8_t* gammas32, size_t count, void* d_out) {
  Scratch s;
  SNARKV_TRY(scratch_of(ctx, n, &s));
  for (size_t j0 = 0; j0 < count; j0 += kProdAffineTerms) {
    const size_t c = std::min<size_t>(kProdAffineTerms, count - j0);
    // host arrays in pageable memory: the copies have left them when hipMemcpyAsync returns
    SNARKV_HIP(hipMemcpyAsync(s.scr + PP_IDX_A, idx_a + j0, 4 * c, hipMemcpyHostToDevice, ctx->stream));
    SNARKV_HIP(hipMemcpyAsync(s.scr + PP_IDX_B, idx_b + j0, 4 * c, hipMemcpyHostToDevice, ctx->stream));
    SNARKV_HIP(hipMemcpyAsync(s.scr + PP_BETA, betas32 + 32 * j0, 32 * c, hipMemcpyHostToDevice, ctx->stream));
    SNARKV_HIP(hipMemcpyAsync(s.scr + PP_GAMMA, gammas32 + 32 * j0, 32 * c, hipMemcpyHostToDevice, ctx->stream));
    hipLaunchKernelGGL(k_prod_affine, dim3((uint32_t)((n + 255) / 256)), dim3(256), 0, ctx->stream, (const uint32_t*)d_polys,
                       (uint32_t)n, (const uint32_t*)(s.scr + PP_IDX_A), (const uint32_t*)(s.scr + PP_IDX_B),
                       (const uint32_t*)(s.scr + PP_BETA), (const uint32_t*)(s.scr + PP_GAMMA), (uint32_t)c, j0 ? 1u : 0u,
                       (uint32_t*)d_out);
    SNARKV_HIP(hipGetLastError());
  }
  return SNARKV_OK;
}

int prod_batch_invert_enqueue(snarkv_ctx* ctx, const void* d_in, size_t n, void* d_out) {
  Scratch s;
  SNARKV_TRY(scratch_of(ctx, n, &s));
  sweep_up(ctx, s, d_in, true);
  const dim3 th(kProdThreads);
  for (uint32_t l = s.lv.count; l-- > 0;) {
    const bool top = l + 1 == s.lv.count;
    const dim3 grid(blocks_at(l, s.lv.len[l]));
    const uint32_t* w = top ? nullptr : s.seq(l + 1);
    const uint32_t len = s.lv.len[l];
    if (l > 0 && top)
      hipLaunchKernelGGL((k_inv_down<kProdThreads, 1, false, true>), grid, th, 0, ctx->stream, (const uint32_t*)s.seq(l), len, w,
                         s.seq(l));
    else if (l > 0)
      hipLaunchKernelGGL((k_inv_down<kProdThreads, 1, false, false>), grid, th, 0, ctx->stream, (const uint32_t*)s.seq(l), len, w,
                         s.seq(l));
    else if (top)
      hipLaunchKernelGGL((k_inv_down<kProdThreads, kProdLane, true, true>), grid, th, 0, ctx->stream, (const uint32_t*)d_in, len,
                         w, (uint32_t*)d_out);
    else
      hipLaunchKernelGGL((k_inv_down<kProdThreads, kProdLane, true, false>), grid, th, 0, ctx->stream, (const uint32_t*)d_in, len,
                         w, (uint32_t*)d_out);
  }
  SNARKV_HIP(hipGetLastError());
  return SNARKV_OK;
}

int prod_grand_product_enqueue(snarkv_ctx* ctx, const void* d_f, size_t n, const void* d_start, void* d_out, void* d_total) {
  Scratch s;
  SNARKV_TRY(scratch_of(ctx, n, &s));
  sweep_up(ctx, s, d_f, false);
  const dim3 th(kProdThreads);
  for (uint32_t l = s.lv.count; l-- > 0;) {
    const bool top = l + 1 == s.lv.count;
    const dim3 grid(blocks_at(l, s.lv.len[l]));
    const uint32_t* carries = top ? (const uint32_t*)d_start : s.seq(l + 1);
    uint32_t* total = top ? (uint32_t*)d_total : nullptr;
    if (l > 0)
      hipLaunchKernelGGL((k_prod_down<kProdThreads, 1>), grid, th, 0, ctx->stream, (const uint32_t*)s.seq(l), s.lv.len[l],
                         carries, top ? 0u : 1u, s.seq(l), total);
    else
      hipLaunchKernelGGL((k_prod_down<kProdThreads, kProdLane>), grid, th, 0, ctx->stream, (const uint32_t*)d_f, s.lv.len[0],
                         carries, top ? 0u : 1u, (uint32_t*)d_out, total);
  }
  SNARKV_HIP(hipGetLastError());
  return SNARKV_OK;
}

}  // namespace snarkv

using namespace snarkv;

extern "C" {

int SNARKV_API(poly_mul_dev)(snarkv_ctx* ctx, const void* d_a32, const void* d_b32, size_t n, void* d_out32) {
  if (!ctx || !aligned16(d_a32) || !aligned16(d_b32) || !aligned16(d_out32)) return SNARKV_ERR_ARG;
  if (partial_overlap(d_out32, d_a32, bytes_of(n)) || partial_overlap(d_out32, d_b32, bytes_of(n)))
    return refuse_overlap("poly_mul", "out is an operand itself or disjoint from it");
  SNARKV_TRY(check_len(n, kProdMaxLen));
  SNARKV_HIP(hipSetDevice(ctx->device));
  return prod_mul_enqueue(ctx, d_a32, d_b32, n, d_out32);
}

int SNARKV_API(poly_prod_affine_dev)(snarkv_ctx* ctx, const void* d_polys32, size_t n, size_t n_polys, const uint32_t* idx_a,
                                     const uint32_t* idx_b, const uint8_t* betas32, const uint8_t* gammas32, size_t count,
                                     void* d_out32) {
  if (!ctx || !aligned16(d_polys32) || !aligned16(d_out32) || !idx_a || !idx_b || !betas32 || !gammas32) return SNARKV_ERR_ARG;
  const uint32_t* idx[2] = {idx_a, idx_b};
  const bool none_ok[2] = {false, true};
  const void* outs[1] = {d_out32};
  const size_t out_bytes[1] = {bytes_of(n)};
  SNARKV_TRY(check_columns("poly_prod_affine", d_polys32, n, n_polys, idx, 2, none_ok, count, outs, out_bytes, 1));
  if (!all_below_r(betas32, count) || !all_below_r(gammas32, count)) return SNARKV_ERR_ENCODING;
  if (count == 0 || n_polys == 0) return SNARKV_ERR_EMPTY;
  SNARKV_TRY(check_len(n, kProdMaxLen));
  SNARKV_HIP(hipSetDevice(ctx->device));
  return prod_affine_enqueue(ctx, d_polys32, n, idx_a, idx_b, betas32, gammas32, count, d_out32);
}

int SNARKV_API(poly_batch_invert_dev)(snarkv_ctx* ctx, const void* d_in32, size_t n, void* d_out32) {
  if (!ctx || !aligned16(d_in32) || !aligned16(d_out32)) return SNARKV_ERR_ARG;
  if (partial_overlap(d_out32, d_in32, bytes_of(n)))
    return refuse_overlap("poly_batch_invert", "out is the input itself or disjoint from it");
  SNARKV_TRY(check_len(n, kProdMaxLen));
  SNARKV_HIP(hipSetDevice(ctx->device));
  return prod_batch_invert_enqueue(ctx, d_in32, n, d_out32);
}

int SNARKV_API(poly_grand_product_dev)(snarkv_ctx* ctx, const void* d_f32, size_t n, const void* d_start32, void* d_out32,
                                       void* d_total32) {
  if (!ctx || !aligned16(d_f32) || !aligned16(d_out32)) return SNARKV_ERR_ARG;
  if ((d_start32 && !aligned16(d_start32)) || (d_total32 && !aligned16(d_total32))) return SNARKV_ERR_ARG;
  const size_t bytes = bytes_of(n);
  if (partial_overlap(d_out32, d_f32, bytes)) return refuse_overlap("poly_grand_product", "out is the factors themselves or disjoint from them");
  if (d_total32 && (overlap(d_total32, 32, d_out32, bytes) || overlap(d_total32, 32, d_f32, bytes)))
    return refuse_overlap("poly_grand_product", "the total lies in the factors or in out");
  if (d_start32 && (overlap(d_start32, 32, d_out32, bytes) || (d_total32 && overlap(d_start32, 32, d_total32, 32))))
    return refuse_overlap("poly_grand_product", "the start value lies in memory the call writes");
  SNARKV_TRY(check_len(n, kProdMaxLen));
  SNARKV_HIP(hipSetDevice(ctx->device));
  return prod_grand_product_enqueue(ctx, d_f32, n, d_start32, d_out32, d_total32);
}

int SNARKV_API(poly_perm_product_dev)(snarkv_ctx* ctx, const void* d_polys32, size_t n, size_t n_polys, const uint32_t* idx_v,
                                      const uint32_t* idx_id, const uint32_t* idx_sigma, size_t count, const uint8_t* beta32,
                                      const uint8_t* gamma32, const void* d_start32, void* d_work32, void* d_z32,
                                      void* d_total32) {
  if (!ctx || !aligned16(d_polys32) || !aligned16(d_work32) || !aligned16(d_z32) || !idx_v || !idx_id || !idx_sigma || !beta32 ||
      !gamma32)
    return SNARKV_ERR_ARG;
  if ((d_start32 && !aligned16(d_start32)) || (d_total32 && !aligned16(d_total32))) return SNARKV_ERR_ARG;
  const size_t bytes = bytes_of(n);
  const uint32_t* idx[3] = {idx_v, idx_id, idx_sigma};
  const bool none_ok[3] = {false, false, false};
  const void* outs[3] = {d_work32, d_z32, d_total32};
  const size_t out_bytes[3] = {2 * bytes, bytes, d_total32 ? (size_t)32 : 0};
  SNARKV_TRY(check_columns("poly_perm_product", d_polys32, n, n_polys, idx, 3, none_ok, count, outs, out_bytes, 3));
  if (overlap(d_work32, 2 * bytes, d_z32, bytes) || overlap(d_total32, out_bytes[2], d_work32, 2 * bytes) ||
      overlap(d_total32, out_bytes[2], d_z32, bytes))
    return refuse_overlap("poly_perm_product", "work, z and the total are disjoint");
  if (d_start32 && (overlap(d_start32, 32, d_work32, 2 * bytes) || overlap(d_start32, 32, d_z32, bytes) ||
                    overlap(d_start32, 32, d_total32, out_bytes[2])))
    return refuse_overlap("poly_perm_product", "the start value lies in memory the call writes");
  if (!below_r(beta32) || !below_r(gamma32)) return SNARKV_ERR_ENCODING;
  if (count == 0 || n_polys == 0) return SNARKV_ERR_EMPTY;
  SNARKV_TRY(check_len(n, kProdMaxLen));
  SNARKV_HIP(hipSetDevice(ctx->device));
  std::vector<uint8_t> betas(32 * count), gammas(32 * count);
  for (size_t j = 0; j < count; ++j) {
    memcpy(betas.data() + 32 * j, beta32, 32);
    memcpy(gammas.data() + 32 * j, gamma32, 32);
  }
  uint8_t* num = (uint8_t*)d_work32;
  uint8_t* den = num + 32 * n;
  // the four public calls, back to back
  SNARKV_TRY(prod_affine_enqueue(ctx, d_polys32, n, idx_v, idx_id, betas.data(), gammas.data(), count, num));
  SNARKV_TRY(prod_affine_enqueue(ctx, d_polys32, n, idx_v, idx_sigma, betas.data(), gammas.data(), count, den));
  SNARKV_TRY(prod_batch_invert_enqueue(ctx, den, n, den));
  SNARKV_TRY(prod_mul_enqueue(ctx, num, den, n, num));
  return prod_grand_product_enqueue(ctx, num, n, d_start32, d_z32, d_total32);
}

}  // extern "C"
