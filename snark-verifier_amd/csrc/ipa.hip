// `IpaAs::decide` on the device (reference snark-verifier/src/pcs/ipa/decider.rs:47-55):
//     U == multi_scalar_multiplication(h_coeffs(xi, 1), dk.g).to_affine()
// The committing key G (2^k points) is uploaded ONCE into a deciding-key object -- the
// reference re-reads it from memory on every decide, a PCIe copy of 64 * 2^k bytes here --
// and the 2^k coefficients of h(X) = prod_i (1 + xi_{k-1-i} X^(2^i)) (pcs/ipa.rs:405-421)
// are produced by a kernel straight into the scalar buffer of the Pippenger, so a decide
// moves k scalars in and 64 bytes out.  A batch of accumulators runs as ONE shared-key MSM over the key's window table
// (msm_shared.hip) from the thresholds below on, one Pippenger per accumulator otherwise.
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include <vector>
#include "ctx.hpp"
#include "fr29.h"
#include "../../include/snarkv_ipa_batch.h"

namespace snarkv {

// coeff[j] = prod over the set bits i of j of xi[k-1-i]   (h_coeffs with scalar = 1: the
// doubling loop `coeffs[len + j] = coeffs[j] * xi` unrolled per index).  One lane per
// coefficient, <= k products; canonical little-endian out.  blockIdx.y = the accumulator: its k challenges, its `count`
// coefficients (one vector of the shared-key MSM's batch; a single accumulator launches one row).
__global__ void __launch_bounds__(256)
    k_h_coeffs(const uint32_t* __restrict__ xi_canon, uint32_t k, uint32_t first, uint32_t count,
               uint32_t* __restrict__ out) {
  __shared__ Fr29 sx[32];
  xi_canon += 8 * (size_t)blockIdx.y * k;
  out += 8 * (size_t)blockIdx.y * count;
  if (threadIdx.x < k) sx[threadIdx.x] = fr29_from_canonical(xi_canon + 8 * (size_t)(k - 1 - threadIdx.x));
  __syncthreads();
  uint32_t t = blockIdx.x * 256u + threadIdx.x;
  if (t >= count) return;
  const uint32_t j = first + t;  // coefficient index in the full 2^k vector; out[] is shard-local
  Fr29 acc = fr29_one();
#pragma unroll 1
  for (uint32_t i = 0; i < k; ++i)
    if ((j >> i) & 1u) acc = fr29_mul(acc, sx[i]);
  uint32_t w[8];
  fr29_to_canonical(acc, w);
  uint4* o = reinterpret_cast<uint4*>(out + 8 * (size_t)t);
  o[0] = make_uint4(w[0], w[1], w[2], w[3]);
  o[1] = make_uint4(w[4], w[5], w[6], w[7]);
}

// SNARKV_IPA_SHARED, read once: 0 = never the shared-key MSM, 1 = whenever the table fits, unset = by the thresholds
static int shared_mode() {
  static const int v = [] {
    const char* e = getenv("SNARKV_IPA_SHARED");
    return e && *e ? (atoi(e) ? 1 : 0) : -1;
  }();
  return v;
}

// When decide_batch takes the shared-key MSM, from profiles/ipa_batch_bench.txt (both curves alike):
//   k <= 14   the table route wins at every m measured, m = 1 included (k = 8: 0.37 against 0.83 ms, k = 14: 0.71 against
//             1.12); a lone accumulator does not BUILD the table, though -- the build costs one to three calls, and a caller
//             that makes a key for one decide would pay it every time -- it uses the table once a batch or prepare() built it
//   k >  14   at k = 16 a lone accumulator loses on the table (1.25 against 1.10 ms), m = 4 ties within the parent's spread
//             and m = 64 wins by 15 %: the table serves batches of kSharedMinMLargeKey or more, between the tie and the win
constexpr uint32_t kSharedSmallKeyMaxK = 14;
constexpr size_t kSharedBuildMinM = 2;      // k <= kSharedSmallKeyMaxK: smallest batch that builds the table
constexpr size_t kSharedMinMLargeKey = 8;   // above: smallest batch on the table route
constexpr size_t kDecideHCap = (size_t)64 << 20;  // coefficient vectors of one group of accumulators
// does a batch of m accumulators take the table route without the override? (`built`: the key has its table already)
static bool shared_by_threshold(uint32_t k, size_t m, bool built) {
  if (k > kSharedSmallKeyMaxK) return m >= kSharedMinMLargeKey;
  return built || m >= kSharedBuildMinM;
}

}  // namespace snarkv

using namespace snarkv;

extern "C" {

static int ipa_dk_make(snarkv_ctx* ctx, const uint8_t* g_points64, uint32_t k, size_t first, size_t count,
                       snarkv_ipa_dk** out) {
  SNARKV_HIP(hipSetDevice(ctx->device));
  snarkv_ipa_dk* dk = new snarkv_ipa_dk();
  dk->device = ctx->device;
  dk->k = k;
  dk->first = first;
  dk->count = count;
  dk->d_points = nullptr;
  dk->table_state = 0;
  dk->d_table = nullptr;
  dk->table_bytes = 0;
  if (hipMalloc(&dk->d_points, count * 64) != hipSuccess) {
    delete dk;
    set_last_error("ipa_dk_create: hipMalloc of %zu bytes failed", count * 64);
    return SNARKV_ERR_DEVICE;
  }
  SNARKV_HIP(hipMemcpyAsync(dk->d_points, g_points64, count * 64, hipMemcpyHostToDevice, ctx->stream));
  SNARKV_HIP(hipStreamSynchronize(ctx->stream));
  *out = dk;
  return SNARKV_OK;
}

int SNARKV_API(ipa_dk_create)(snarkv_ctx* ctx, const uint8_t* g_points64, size_t n, snarkv_ipa_dk** out) {
  if (!ctx || !g_points64 || !out) return SNARKV_ERR_ARG;
  if (n == 0) return SNARKV_ERR_EMPTY;
  uint32_t k = 0;
  while (((size_t)1 << k) < n) ++k;
  if (((size_t)1 << k) != n || k < 1 || k > 28) return SNARKV_ERR_LENGTH;  // committing keys have 2^k points
  return ipa_dk_make(ctx, g_points64, k, 0, n, out);
}

// Multi-GPU: this rank holds points [first, first + count) of the 2^k-point key.
int SNARKV_API(ipa_dk_create_shard)(snarkv_ctx* ctx, const uint8_t* g_shard64, size_t count, uint32_t k, size_t first,
                                    snarkv_ipa_dk** out) {
  if (!ctx || !g_shard64 || !out) return SNARKV_ERR_ARG;
  if (count == 0) return SNARKV_ERR_EMPTY;
  if (k < 1 || k > 28 || first + count > ((size_t)1 << k)) return SNARKV_ERR_LENGTH;
  return ipa_dk_make(ctx, g_shard64, k, first, count, out);
}

// The shard's part of commit(G, h(xi)) as a projective partial (SNARKV_G1_PARTIAL_BYTES), device to device:
// all-gather the partials and fold them (snarkv_g1_fold_partials_dev) to get the point `decide` compares with U.
int SNARKV_API(ipa_commit_partial_dev)(snarkv_ctx* ctx, const snarkv_ipa_dk* dk, const uint8_t* xi32, void* d_partial) {
  if (!ctx || !dk || !xi32 || !d_partial) return SNARKV_ERR_ARG;
  if (dk->device != ctx->device) return SNARKV_ERR_ARG;
  SNARKV_HIP(hipSetDevice(ctx->device));
  SNARKV_WIRE_FORM(ctx);  // the IPA speaks the wire form whatever the context's default flags say (include/snarkv_amd.h)
  const uint32_t k = dk->k;
  void *d_xi, *d_h;
  SNARKV_TRY(ctx_reserve(ctx, SLOT_IPA_XI, (size_t)k * 32, &d_xi));
  SNARKV_TRY(ctx_reserve(ctx, SLOT_IPA_H, dk->count * 32, &d_h));
  SNARKV_HIP(hipMemcpyAsync(d_xi, xi32, (size_t)k * 32, hipMemcpyHostToDevice, ctx->stream));
  hipLaunchKernelGGL(k_h_coeffs, dim3((uint32_t)((dk->count + 255) / 256)), dim3(256), 0, ctx->stream,
                     (const uint32_t*)d_xi, k, (uint32_t)dk->first, (uint32_t)dk->count, (uint32_t*)d_h);
  SNARKV_HIP(hipGetLastError());
  return launch_msm_pippenger(ctx, d_h, dk->d_points, dk->count, 0, d_partial, true);
}

void SNARKV_API(ipa_dk_destroy)(snarkv_ipa_dk* dk) {
  if (!dk) return;
  (void)hipSetDevice(dk->device);
  if (dk->d_points) (void)hipFree(dk->d_points);
  if (dk->d_table) (void)hipFree(dk->d_table);
  delete dk;
}

int SNARKV_API(ipa_dk_prepare)(snarkv_ctx* ctx, snarkv_ipa_dk* dk) {
  if (!ctx || !dk) return SNARKV_ERR_ARG;
  if (dk->device != ctx->device) return SNARKV_ERR_ARG;
  SNARKV_HIP(hipSetDevice(ctx->device));
  bool have;
  return ipa_dk_table_prepare(ctx, dk, &have);  // a shard or a key over the cap: nothing to build, still OK
}

size_t SNARKV_API(ipa_dk_table_bytes)(const snarkv_ipa_dk* dk) {
  if (!dk) return 0;
  std::lock_guard<std::mutex> lk(dk->table_mu);
  return dk->table_bytes;
}

uint32_t SNARKV_API(ipa_dk_k)(const snarkv_ipa_dk* dk) { return dk ? dk->k : 0; }

int SNARKV_API(ipa_decide_batch)(snarkv_ctx* ctx, const snarkv_ipa_dk* dk, const uint8_t* xi32, const uint8_t* u64, size_t m,
                            uint8_t* ok) {
  if (!ctx || !dk || !xi32 || !u64 || !ok) return SNARKV_ERR_ARG;
  if (m == 0) return SNARKV_ERR_EMPTY;
  if (dk->device != ctx->device) return SNARKV_ERR_ARG;
  if (dk->first != 0 || dk->count != ((size_t)1 << dk->k)) return SNARKV_ERR_LENGTH;  // a shard cannot decide alone
  SNARKV_HIP(hipSetDevice(ctx->device));
  SNARKV_WIRE_FORM(ctx);  // (the lanes take the call's encoding at the fork: ctx_lanes_fork)
  const uint32_t k = dk->k;
  const size_t n = (size_t)1 << k;
  void *d_xi, *d_out;
  SNARKV_TRY(ctx_reserve(ctx, SLOT_IPA_XI, m * k * 32, &d_xi));
  SNARKV_TRY(ctx_reserve(ctx, SLOT_IPA_OUT, m * 64, &d_out));
  SNARKV_HIP(hipMemcpyAsync(d_xi, xi32, m * k * 32, hipMemcpyHostToDevice, ctx->stream));
  // the shared-key MSM: the coefficients of a group of accumulators into one buffer, one launch for the group
  bool shared = false;
  if (shared_mode() != 0 && ipa_dk_table_fits(dk) &&
      (shared_mode() == 1 || shared_by_threshold(k, m, SNARKV_API(ipa_dk_table_bytes)(dk) != 0)))
    SNARKV_TRY(ipa_dk_table_prepare(ctx, dk, &shared));
  if (shared) {
    const size_t group = std::min<size_t>({m, (size_t)32768, std::max<size_t>(1, kDecideHCap / (n * 32))});
    void* d_h;
    SNARKV_TRY(ctx_reserve(ctx, SLOT_IPA_H, group * n * 32, &d_h));
    for (size_t a0 = 0; a0 < m; a0 += group) {
      const size_t g = std::min(group, m - a0);
      hipLaunchKernelGGL(k_h_coeffs, dim3((uint32_t)((n + 255) / 256), (uint32_t)g), dim3(256), 0, ctx->stream,
                         (const uint32_t*)d_xi + a0 * k * 8, k, 0u, (uint32_t)n, (uint32_t*)d_h);
      SNARKV_HIP(hipGetLastError());
      SNARKV_TRY(launch_msm_shared(ctx, dk, d_h, n, g, 0, (uint8_t*)d_out + 64 * a0));
    }
    std::vector<uint8_t> got(m * 64);
    SNARKV_HIP(hipMemcpyAsync(got.data(), d_out, m * 64, hipMemcpyDeviceToHost, ctx->stream));
    SNARKV_HIP(hipStreamSynchronize(ctx->stream));
    for (size_t a = 0; a < m; ++a) ok[a] = memcmp(&got[64 * a], u64 + 64 * a, 64) == 0 ? 1 : 0;
    return SNARKV_OK;
  }
  // accumulators are independent: up to four in flight (the tail of one Pippenger -- bucket reduce,
  // shift chains -- overlaps the accumulation of the next), each lane with its own h buffer
  const bool lanes = m >= 2;
  if (lanes) {
    SNARKV_TRY(ctx_lanes(ctx));
    SNARKV_TRY(ctx_lanes_fork(ctx));
  }
  // an error between fork and join must not leave the sub-streams unjoined: remember it, join, then return it
  int rc = SNARKV_OK;
  const bool was_throughput = ctx->throughput_mode;
  if (lanes) ctx->throughput_mode = true;  // four accumulators in flight: the caller's lane runs like the others
  for (size_t a = 0; a < m && rc == SNARKV_OK; ++a) {
    snarkv_ctx* lane = lanes ? ctx_lane(ctx, a) : ctx;
    void* d_h;
    rc = ctx_reserve(lane, SLOT_IPA_H, n * 32, &d_h);
    if (rc != SNARKV_OK) break;
    hipLaunchKernelGGL(k_h_coeffs, dim3((uint32_t)((n + 255) / 256)), dim3(256), 0, lane->stream,
                       (const uint32_t*)d_xi + a * k * 8, k, 0u, (uint32_t)n, (uint32_t*)d_h);
    if (hipGetLastError() != hipSuccess) {
      set_last_error("ipa_decide_batch: k_h_coeffs launch failed");
      rc = SNARKV_ERR_DEVICE;
      break;
    }
    rc = launch_msm_pippenger(lane, d_h, dk->d_points, n, 0, (uint8_t*)d_out + 64 * a, false);
  }
  ctx->throughput_mode = was_throughput;
  if (lanes) {
    int jrc = ctx_lanes_join(ctx);
    if (rc == SNARKV_OK) rc = jrc;
  }
  if (rc != SNARKV_OK) return rc;
  std::vector<uint8_t> got(m * 64);
  SNARKV_HIP(hipMemcpyAsync(got.data(), d_out, m * 64, hipMemcpyDeviceToHost, ctx->stream));
  SNARKV_HIP(hipStreamSynchronize(ctx->stream));
  for (size_t a = 0; a < m; ++a) ok[a] = memcmp(&got[64 * a], u64 + 64 * a, 64) == 0 ? 1 : 0;
  return SNARKV_OK;
}

}  // extern "C"
