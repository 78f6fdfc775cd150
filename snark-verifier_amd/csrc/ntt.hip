// Forward, inverse and coset number-theoretic transforms of polynomials in device memory (include/snarkv_ntt.h).  Same
// source for both curves, as poly.hip.
//
// ntt_plan.h splits the k levels into passes over tiles of at most 2^9 elements and ntt_tile.h holds the arithmetic; here is
// the kernel that runs one pass (one workgroup per tile, 256 threads, one butterfly per thread and level, the tile as 512 Fr29
// = 18 KiB of LDS next to the 256 in-tile factors, 9 KiB), the kernel that fills the tables of powers, and the host side.
//   k_ntt_pass    load (words -> Montgomery domain, times s^j in the first pass of a shifted forward transform), the levels
//                 with one barrier each, store (times the factor between passes, or n^-1 s^j in the last pass of an inverse
//                 one, -> canonical words).  Passes before the last store where they loaded; the last one stores in natural
//                 order, out of the working buffer.
//   k_ntt_table   out[j] = (base^(2^pre))^j in the wanted form: the in-tile factors, the two-level tables of w_n and of the
//                 shift
// Values cross passes as canonical words.
#include <string.h>
#include "ctx.hpp"
#include "poly_args.hpp"
#include "ntt_plan.h"
#include "ntt_tile.h"
#include "../../include/snarkv_ntt.h"

namespace snarkv {

constexpr uint32_t kNttTileBits = 9, kNttColBits = 2;
using Plan = NttPlan<kNttTileBits, kNttColBits>;
constexpr uint32_t kNttThreads = 1u << (kNttTileBits - 1);
constexpr uint32_t kNttMaxK = SNARKV_FR_TWO_ADICITY < 30 ? SNARKV_FR_TWO_ADICITY : 30;
constexpr size_t kNttMaxCount = 65535;  // the batch is the grid's y

// where a pass takes its per-element factors from (device addresses; see ntt_factor)
struct NttFactors {
  const Fr29* ld_lo;  // null: the constant 2^522
  const Fr29* ld_hi;
  const Fr29* st_lo;  // null: the integer 1
  const Fr29* st_hi;  // null: the constant *st_lo
  uint32_t h;
};

__global__ void __launch_bounds__(kNttThreads) k_ntt_pass(Plan plan, uint32_t p, const uint32_t* in, uint32_t* out,
                                                          const Fr29* __restrict__ tile_tw, NttFactors f) {
  __shared__ Fr29 buf[1u << kNttTileBits];
  __shared__ Fr29 tw[kNttThreads];
  const uint32_t lane = threadIdx.x, g = blockIdx.x, slots = plan.slots(p);
  const size_t poly = (size_t)blockIdx.y << plan.k;
  tw[lane] = tile_tw[lane];
#pragma unroll 1
  for (uint32_t slot = lane; slot < slots; slot += kNttThreads) {
    const uint32_t j = plan.load_index(p, g, slot);
    const uint4* src = reinterpret_cast<const uint4*>(in + 8 * (poly + j));
    const uint4 a = src[0], b = src[1];
    const uint32_t w[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
    buf[plan.load_lds(p, slot)] = ntt_load(w, f.ld_lo ? ntt_factor(f.ld_lo, f.ld_hi, j, f.h) : ntt_factor_in());
  }
  __syncthreads();
#pragma unroll 1
  for (uint32_t level = 0; level < plan.t[p]; ++level) {
    if (lane < slots / 2)
      ntt_butterfly(buf, plan.bfly_top(p, level, lane), plan.bfly_distance(p, level), tw[plan.bfly_twiddle(p, level, lane)], level);
    __syncthreads();
  }
#pragma unroll 1
  for (uint32_t slot = lane; slot < slots; slot += kNttThreads) {
    const uint32_t i = plan.store_index(p, g, slot);
    Fr29 fac = ntt_factor_out();
    if (f.st_lo) {
      const uint32_t e = plan.last(p) ? i : plan.twiddle_exp(p, g, slot);
      fac = f.st_hi ? ntt_factor(f.st_lo, f.st_hi, e, f.h) : f.st_lo[0];
    }
    uint32_t w[8];
    ntt_store(buf[plan.store_lds(p, slot)], fac, w);
    uint4* dst = reinterpret_cast<uint4*>(out + 8 * (poly + i));
    dst[0] = make_uint4(w[0], w[1], w[2], w[3]);
    dst[1] = make_uint4(w[4], w[5], w[6], w[7]);
  }
}

__global__ void __launch_bounds__(256) k_ntt_table(Fr29 base, uint32_t pre, uint32_t count, Fr29 scale, Fr29* __restrict__ out) {
  const uint32_t j = blockIdx.x * 256u + threadIdx.x;
  if (j < count) out[j] = ntt_table_entry(base, pre, j, scale);
}

namespace {

// layout of the context's SLOT_NTT for a transform of 2^k: the tables, then the working buffer of the passes
struct Layout {
  uint32_t h, n_lo, n_hi;
  size_t tile_tw, n_inv, w_lo, w_hi, s_lo, s_hi, work, end;
};

Layout layout_of(const Plan& plan, size_t count) {
  Layout l;
  l.h = plan.split_bits();
  l.n_lo = 1u << l.h;
  l.n_hi = 1u << (plan.k - l.h);
  size_t off = 0;
  auto take = [&](size_t entries) {
    const size_t at = off;
    off += sizeof(Fr29) * entries;
    return at;
  };
  l.tile_tw = take(kNttThreads);
  l.n_inv = take(1);
  l.w_lo = take(l.n_lo);
  l.w_hi = take(l.n_hi);
  l.s_lo = take(l.n_lo);
  l.s_hi = take(l.n_hi);
  l.work = (off + 255) & ~(size_t)255;
  l.end = l.work + (plan.passes > 1 ? (count << plan.k) * 32 : 0);
  return l;
}

void table(snarkv_ctx* ctx, const Fr29& base, uint32_t pre, uint32_t count, const Fr29& scale, void* out) {
  hipLaunchKernelGGL(k_ntt_table, dim3((count + 255) / 256), dim3(256), 0, ctx->stream, base, pre, count, scale, (Fr29*)out);
}

}  // namespace

int ntt_enqueue(snarkv_ctx* ctx, const void* d_in, void* d_out, uint32_t k, size_t count, bool inverse, const uint32_t* shift) {
  const Plan plan(k);
  const Layout l = layout_of(plan, count);
  void* d_scr;
  const size_t cap_before = ctx->cap[SLOT_NTT];
  SNARKV_TRY(ctx_reserve(ctx, SLOT_NTT, l.end, &d_scr));
  if (ctx->cap[SLOT_NTT] != cap_before) ctx->ntt_key = 0;  // the slot has grown: a new buffer, at the old address or not
  uint8_t* scr = (uint8_t*)d_scr;
  const uint32_t key = 1u + (k << 1 | (inverse ? 1u : 0u));
  if (ctx->ntt_tables != d_scr || ctx->ntt_key != key) {  // the first use of (k, direction) since the slot was allocated
    table(ctx, ntt_root_squared(inverse, SNARKV_FR_TWO_ADICITY - kNttTileBits), 0, kNttThreads, fr29_one(), scr + l.tile_tw);
    table(ctx, fr29_one(), 0, 1, ntt_n_inverse(k), scr + l.n_inv);
    if (plan.passes > 1) {
      const Fr29 w = ntt_root_squared(inverse, SNARKV_FR_TWO_ADICITY - k);
      table(ctx, w, 0, l.n_lo, ntt_factor_out(), scr + l.w_lo);
      table(ctx, w, l.h, l.n_hi, fr29_one(), scr + l.w_hi);
    }
    SNARKV_HIP(hipGetLastError());
    ctx->ntt_tables = d_scr;
    ctx->ntt_key = key;
  }
  if (shift) {  // s^j, for the loads of a forward transform or, with n^-1, for the stores of an inverse one
    const Fr29 s = fr29_from_canonical(shift);
    table(ctx, s, 0, l.n_lo, inverse ? ntt_n_inverse(k) : ntt_factor_in(), scr + l.s_lo);
    table(ctx, s, l.h, l.n_hi, fr29_one(), scr + l.s_hi);
  }
  uint32_t* work = (uint32_t*)(scr + l.work);
  for (uint32_t p = 0; p < plan.passes; ++p) {
    NttFactors f = {nullptr, nullptr, nullptr, nullptr, l.h};
    if (p == 0 && shift && !inverse) f.ld_lo = (const Fr29*)(scr + l.s_lo), f.ld_hi = (const Fr29*)(scr + l.s_hi);
    if (!plan.last(p)) f.st_lo = (const Fr29*)(scr + l.w_lo), f.st_hi = (const Fr29*)(scr + l.w_hi);
    else if (inverse && shift) f.st_lo = (const Fr29*)(scr + l.s_lo), f.st_hi = (const Fr29*)(scr + l.s_hi);
    else if (inverse) f.st_lo = (const Fr29*)(scr + l.n_inv);
    hipLaunchKernelGGL(k_ntt_pass, dim3(plan.tiles(p), (uint32_t)count), dim3(kNttThreads), 0, ctx->stream, plan, p,
                       p == 0 ? (const uint32_t*)d_in : (const uint32_t*)work, plan.last(p) ? (uint32_t*)d_out : work,
                       (const Fr29*)(scr + l.tile_tw), f);
  }
  SNARKV_HIP(hipGetLastError());
  return SNARKV_OK;
}

}  // namespace snarkv

using namespace snarkv;

extern "C" {

uint32_t SNARKV_API(ntt_max_k)(void) { return kNttMaxK; }

int SNARKV_API(ntt_dev)(snarkv_ctx* ctx, const void* d_in32, void* d_out32, uint32_t k, size_t count, uint32_t direction,
                        const uint8_t* shift32) {
  if (!ctx || !aligned16(d_in32) || !aligned16(d_out32)) return SNARKV_ERR_ARG;
  if (direction > SNARKV_NTT_INVERSE) return SNARKV_ERR_ARG;
  if (count == 0) return SNARKV_ERR_EMPTY;
  if (k > kNttMaxK || count > kNttMaxCount) return SNARKV_ERR_LENGTH;
  uint32_t shift[8];
  if (shift32) {
    if (is_zero32(shift32)) {
      set_last_error("ntt: a shift of zero");
      return SNARKV_ERR_ARG;
    }
    if (!below_r(shift32)) return SNARKV_ERR_ENCODING;
    memcpy(shift, shift32, 32);
  }
  if (partial_overlap(d_in32, d_out32, (count << k) * 32))
    return refuse_overlap("ntt", "in and out are the same buffer or disjoint");
  // a buffer the runtime knows to live on another device (what it does not know is the caller's to answer for)
  hipPointerAttribute_t attr;
  if (hipPointerGetAttributes(&attr, d_in32) == hipSuccess && attr.type == hipMemoryTypeDevice && attr.device != ctx->device) {
    set_last_error("ntt: the data is on device %d, the context on %d", attr.device, ctx->device);
    return SNARKV_ERR_ARG;
  }
  (void)hipGetLastError();  // an address the runtime does not know leaves an error behind
  SNARKV_HIP(hipSetDevice(ctx->device));
  return ntt_enqueue(ctx, d_in32, d_out32, k, count, direction == SNARKV_NTT_INVERSE, shift32 ? shift : nullptr);
}

}  // extern "C"
