// The transform of ntt.hip over group elements (include/snarkv_g1_ntt.h): a commitment key's points to its Lagrange basis and
// back.  Same source for both curves.
//
// g1_ntt.h holds the pass structure (Stockham radix-2: k passes between two buffers, natural order at both ends) and the
// arithmetic of a lane; here are the kernels and the host side.  A pass is the two stages of the segmented MSM (msm_naive.hip),
// in a transform's access pattern:
//   k_g1_ntt_twiddles  tw[j] = w^j, j < n/2, as canonical words for the GLV split, and n^-1 behind them
//   k_g1_ntt_mul       two lanes per butterfly, one per GLV half of t = w^e * b: the half's signed 3-bit window (tables of 2Q,
//                      3Q, 4Q limb-major in a global scratch, a slice per wavefront, digits in LDS: k_term_scalar_mul's
//                      layout), an XYZZ partial per lane
//   k_g1_ntt_combine   one lane per output: t from its two partials, a + t or a - t in XYZZ with the careful adders, to affine
//                      by an inversion of its own, canonical words out.  Pass 0 (every twiddle 1) runs this stage alone, on b
//                      as it is; the pass that multiplies by n^-1 runs it without an `a`.
// A pass runs in chunks of 2^16 multiplications: 2 048 wavefronts, what 256 compute units hold at 2 per SIMD, so that the
// partials (144 bytes per lane) and the tables (27 648 bytes per wavefront) are sized by the chunk and not by the transform.
// Tried and dropped, by the compiler's figures alone: both stages in one kernel, the halves crossing by a shuffle (256 VGPRs
// and 178 spilled at 2 wavefronts per SIMD), and k_g1_ntt_mul as a block that walks its share of the lanes in a loop (256 and
// 156 spilled); as it stands it is k_term_scalar_mul's budget.
#include "ctx.hpp"
#include "poly_args.hpp"
#include "g1_ntt.h"
#include "../../include/snarkv_g1_ntt.h"
#include <algorithm>

namespace snarkv {

namespace {

constexpr int kG1NttWaves = 2;                   // wavefronts per SIMD k_g1_ntt_mul is compiled for, as k_term_scalar_mul
constexpr uint32_t kG1NttChunk = 1u << 16;       // multiplications per launch
enum { G1_NTT_PASS = 0, G1_NTT_PASS0 = 1, G1_NTT_SCALE = 2 };

// a lane's scratch: its column of this wavefront's table slice [entry 0..2][limb 0..35][lane] and of the digits
struct DevScratch {
  int32_t (*tab)[36][64];
  int8_t (*dig)[64];
  uint32_t lane;
  __device__ __forceinline__ void col_put(int e, int row0, const Fq29& v) {
#pragma unroll
    for (int l = 0; l < 9; ++l) tab[e][row0 + l][lane] = v.v[l];
  }
  __device__ __forceinline__ Fq29 col_get(int e, int row0) const {
    Fq29 v;
#pragma unroll
    for (int l = 0; l < 9; ++l) v.v[l] = tab[e][row0 + l][lane];
    return v;
  }
  __device__ __forceinline__ void tab_put(int e, const G1Xyzz29& v) {
    col_put(e, 0, v.x), col_put(e, 9, v.y), col_put(e, 18, v.zz), col_put(e, 27, v.zzz);
  }
  __device__ __forceinline__ G1Xyzz29 tab_get(int e) const {
    G1Xyzz29 v;
    v.x = col_get(e, 0), v.y = col_get(e, 9), v.zz = col_get(e, 18), v.zzz = col_get(e, 27);
    return v;
  }
  __device__ __forceinline__ void dig_put(int i, int d) { dig[i][lane] = (int8_t)d; }
  __device__ __forceinline__ int dig_get(int i) const { return dig[i][lane]; }
};

__device__ __forceinline__ void load_words(const uint32_t* __restrict__ src, uint32_t* dst, int n16) {
  const uint4* s = reinterpret_cast<const uint4*>(src);
#pragma unroll
  for (int i = 0; i < n16; ++i) {
    const uint4 v = s[i];
    dst[4 * i + 0] = v.x, dst[4 * i + 1] = v.y, dst[4 * i + 2] = v.z, dst[4 * i + 3] = v.w;
  }
}

struct Scalar8 {
  uint32_t w[8];
};

__global__ void __launch_bounds__(256) k_g1_ntt_twiddles(Fr29 w, uint32_t count, Scalar8 n_inv, uint32_t* __restrict__ out) {
  const uint32_t j = blockIdx.x * 256u + threadIdx.x;
  if (j > count) return;
  uint32_t e[8];
  if (j < count) g1_ntt_twiddle(w, j, e);
  else
    for (int i = 0; i < 8; ++i) e[i] = n_inv.w[i];
  uint4* dst = reinterpret_cast<uint4*>(out + 8 * (size_t)j);
  dst[0] = make_uint4(e[0], e[1], e[2], e[3]);
  dst[1] = make_uint4(e[4], e[5], e[6], e[7]);
}

// multiplications m0 .. m0 + count of pass s (mode G1_NTT_PASS: m a butterfly) or of the scaling (G1_NTT_SCALE: m a point,
// times the entry behind the twiddles): parts[2 (m - m0) + h] = half h
__global__ void __launch_bounds__(64, kG1NttWaves) k_g1_ntt_mul(const uint32_t* __restrict__ in, const uint32_t* __restrict__ tw,
                                                                uint32_t k, uint32_t s, uint32_t mode, uint32_t m0, uint32_t count,
                                                                G1Xyzz29* __restrict__ parts, int32_t* __restrict__ tabg) {
  __shared__ int8_t dig[kWinDigits][64];
  DevScratch scr;
  scr.tab = reinterpret_cast<int32_t(*)[36][64]>(tabg + (size_t)blockIdx.x * 3 * 36 * 64);
  scr.dig = dig;
  scr.lane = threadIdx.x;
  const uint32_t g = blockIdx.x * 64u + threadIdx.x;
  if (g >= 2 * count) return;
  const uint32_t m = m0 + (g >> 1);
  uint32_t b = m, e = 1u << (k - 1);
  if (mode == G1_NTT_PASS) {
    const G1NttBfly f = g1_ntt_bfly(k, s, m);
    b = f.b, e = f.e;
  }
  uint32_t bw[16], ew[8];
  load_words(in + 16 * (size_t)b, bw, 4);
  load_words(tw + 8 * (size_t)e, ew, 2);
  parts[g] = g1_ntt_lane_mul(bw, ew, g & 1u, scr);
}

// the outputs of the same multiplications: two per butterfly, one per scaled point.  G1_NTT_PASS0: no partials, t = b.
__global__ void __launch_bounds__(256) k_g1_ntt_combine(const uint32_t* __restrict__ in, uint32_t* __restrict__ out, uint32_t k,
                                                        uint32_t s, uint32_t mode, uint32_t m0, uint32_t count,
                                                        const G1Xyzz29* __restrict__ parts) {
  const uint32_t g = blockIdx.x * 256u + threadIdx.x;
  if (g >= (mode == G1_NTT_SCALE ? count : 2 * count)) return;
  uint32_t ow[16], o;
  if (mode == G1_NTT_SCALE) {
    o = m0 + g;
    g1_ntt_lane_out(nullptr, parts[2 * (size_t)g], parts[2 * (size_t)g + 1], false, ow);
  } else {
    const uint32_t h = g & 1u;
    const G1NttBfly f = g1_ntt_bfly(k, s, m0 + (g >> 1));
    o = h ? f.hi : f.lo;
    uint32_t aw[16];
    load_words(in + 16 * (size_t)f.a, aw, 4);
    G1Xyzz29 r0, r1 = xyzz29_identity();
    if (mode == G1_NTT_PASS0) {
      uint32_t bw[16];
      load_words(in + 16 * (size_t)f.b, bw, 4);
      r0 = xyzz29_from_affine(g1a29_from_canonical(bw));
    } else {
      r0 = parts[g & ~1u], r1 = parts[g | 1u];
    }
    g1_ntt_lane_out(aw, r0, r1, h != 0, ow);
  }
  uint4* dst = reinterpret_cast<uint4*>(out + 16 * (size_t)o);
#pragma unroll
  for (int i = 0; i < 4; ++i) dst[i] = make_uint4(ow[4 * i], ow[4 * i + 1], ow[4 * i + 2], ow[4 * i + 3]);
}

}  // namespace

// the transform of 2^k points, 1 <= k <= kG1NttMaxK, arguments taken as checked; d_out may be d_in
int g1_ntt_enqueue(snarkv_ctx* ctx, const void* d_in, void* d_out, uint32_t k, bool inverse) {
  const size_t n = (size_t)1 << k, bytes = 64 * n;
  const uint32_t steps = k + (inverse ? 1u : 0u);
  const uint32_t chunk = (uint32_t)std::min<size_t>(kG1NttChunk, n);  // multiplications per launch: n/2 butterflies, or n points
  const uint32_t grid = (2 * chunk + 63) / 64;  // wavefronts of the largest launch of k_g1_ntt_mul
  // the slot: twiddles and n^-1 | two working buffers | a chunk's partials | the window tables
  const size_t tw_bytes = ((n / 2 + 1) * 32 + 255) & ~(size_t)255, part_bytes = 2 * (size_t)chunk * sizeof(G1Xyzz29),
               tab_bytes = (size_t)grid * 3 * 36 * 64 * 4;
  void* d_scr;
  SNARKV_TRY(ctx_reserve(ctx, SLOT_G1_NTT, tw_bytes + 2 * bytes + part_bytes + tab_bytes, &d_scr));
  uint8_t* scr = (uint8_t*)d_scr;
  uint32_t* tw = (uint32_t*)scr;
  uint32_t* work[2] = {(uint32_t*)(scr + tw_bytes), (uint32_t*)(scr + tw_bytes + bytes)};
  G1Xyzz29* parts = (G1Xyzz29*)(scr + tw_bytes + 2 * bytes);
  int32_t* tab = (int32_t*)(scr + tw_bytes + 2 * bytes + part_bytes);
  Scalar8 n_inv;
  g1_ntt_n_inverse(k, n_inv.w);
  const uint32_t half = (uint32_t)(n / 2);
  hipLaunchKernelGGL(k_g1_ntt_twiddles, dim3(half / 256 + 1), dim3(256), 0, ctx->stream,
                     ntt_root_squared(inverse, SNARKV_FR_TWO_ADICITY - k), half, n_inv, tw);
  const uint32_t* src = (const uint32_t*)d_in;
  for (uint32_t step = 0; step < steps; ++step) {
    // no step writes where it reads: the last one writes d_out unless it would read it (one step, in place)
    const bool last = step + 1 == steps;
    uint32_t* dst = last && src != (const uint32_t*)d_out ? (uint32_t*)d_out : work[step & 1u];
    const uint32_t mode = step == k ? G1_NTT_SCALE : (step == 0 ? G1_NTT_PASS0 : G1_NTT_PASS);
    const uint32_t total = mode == G1_NTT_SCALE ? (uint32_t)n : half;
    const uint32_t per = mode == G1_NTT_PASS0 ? total : chunk;  // pass 0 has no partials to hold
    for (uint32_t m0 = 0; m0 < total; m0 += per) {
      const uint32_t count = std::min(per, total - m0), outs = mode == G1_NTT_SCALE ? count : 2 * count;
      if (mode != G1_NTT_PASS0)
        hipLaunchKernelGGL(k_g1_ntt_mul, dim3((2 * count + 63) / 64), dim3(64), 0, ctx->stream, src,
                           (const uint32_t*)tw, k, step, mode, m0, count, parts, tab);
      hipLaunchKernelGGL(k_g1_ntt_combine, dim3((outs + 255) / 256), dim3(256), 0, ctx->stream, src, dst, k, step, mode, m0, count,
                         (const G1Xyzz29*)parts);
    }
    src = dst;
  }
  SNARKV_HIP(hipGetLastError());
  if (src != (const uint32_t*)d_out) SNARKV_HIP(hipMemcpyAsync(d_out, src, bytes, hipMemcpyDeviceToDevice, ctx->stream));
  return SNARKV_OK;
}

}  // namespace snarkv

using namespace snarkv;

namespace {

int g1_ntt_checked(snarkv_ctx* ctx, const void* d_in64, void* d_out64, uint32_t k, uint32_t direction) {
  // a buffer the runtime knows to live on another device (what it does not know is the caller's to answer for)
  hipPointerAttribute_t attr;
  if (hipPointerGetAttributes(&attr, d_in64) == hipSuccess && attr.type == hipMemoryTypeDevice && attr.device != ctx->device) {
    set_last_error("g1_ntt: the data is on device %d, the context on %d", attr.device, ctx->device);
    return SNARKV_ERR_ARG;
  }
  (void)hipGetLastError();  // an address the runtime does not know leaves an error behind
  SNARKV_HIP(hipSetDevice(ctx->device));
  if (k == 0) {
    if (d_in64 != d_out64) SNARKV_HIP(hipMemcpyAsync(d_out64, d_in64, 64, hipMemcpyDeviceToDevice, ctx->stream));
    return SNARKV_OK;
  }
  return g1_ntt_enqueue(ctx, d_in64, d_out64, k, direction == SNARKV_NTT_INVERSE);
}

}  // namespace

extern "C" {

uint32_t SNARKV_API(g1_ntt_max_k)(void) { return kG1NttMaxK; }

int SNARKV_API(g1_ntt_dev)(snarkv_ctx* ctx, const void* d_in64, void* d_out64, uint32_t k, uint32_t direction) {
  if (!ctx || !aligned16(d_in64) || !aligned16(d_out64)) return SNARKV_ERR_ARG;
  if (direction > SNARKV_NTT_INVERSE) return SNARKV_ERR_ARG;
  if (k > kG1NttMaxK) return SNARKV_ERR_LENGTH;
  if (partial_overlap(d_in64, d_out64, (size_t)64 << k)) return refuse_overlap("g1_ntt", "in and out are the same buffer or disjoint");
  return g1_ntt_checked(ctx, d_in64, d_out64, k, direction);
}

int SNARKV_API(ipa_dk_lagrange_dev)(snarkv_ctx* ctx, const snarkv_ipa_dk* dk, void* d_out64) {
  if (!ctx || !dk || !aligned16(d_out64)) return SNARKV_ERR_ARG;
  if (dk->device != ctx->device) {
    set_last_error("ipa_dk_lagrange: the key is on device %d, the context on %d", dk->device, ctx->device);
    return SNARKV_ERR_ARG;
  }
  if (dk->first != 0 || dk->count != ((size_t)1 << dk->k)) {
    set_last_error("ipa_dk_lagrange: the key is a shard (%zu points from %zu of 2^%u)", dk->count, dk->first, dk->k);
    return SNARKV_ERR_LENGTH;
  }
  if (dk->k > kG1NttMaxK) return SNARKV_ERR_LENGTH;
  if (overlap(dk->d_points, (size_t)64 << dk->k, d_out64, (size_t)64 << dk->k))
    return refuse_overlap("ipa_dk_lagrange", "the output and the key's points");
  return g1_ntt_checked(ctx, dk->d_points, d_out64, dk->k, SNARKV_NTT_INVERSE);
}

}  // extern "C"
