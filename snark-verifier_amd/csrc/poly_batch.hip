// Many evaluations of resident polynomials in one call (include/snarkv_poly_batch.h).  Same source for both curves, as poly.hip.
//
// The evaluation of poly.hip is phase 1 of the blocked scan of poly_scan.h, level by level: a block of 256 coefficients gives
// its total T_b, the totals are a polynomial in a^256 one level up, p(a) = sum_b T_b (a^256)^b.  Here the same levels run over
// a second grid dimension that names the query:
//   k_pb_scan   workgroup (b, q): block b of query q's row at this level, under query q's root; the total goes to query q's
//               row of the level above, a^256 to query q's root there (block 0 writes it)
// At level 0 a query's row is the polynomial q_poly[q] and its root the point q_point[q], both read through the index arrays
// staged in the slot; above, row and root are the query's own.  The last level has one block per query and writes out[q].
// One launch per level whatever the count.
#include <algorithm>
#include "poly.hpp"
#include "poly_args.hpp"
#include "ipa_prover.hpp"
#include "poly_scan.h"
#include "../../include/snarkv_poly_batch.h"

namespace snarkv {

using Scan = PolyScan<kPolyBlock>;
constexpr uint32_t kBatchLevels = 5;            // as poly.hip: 256^4 >= 2^30
constexpr size_t kBatchGridY = 65535;            // queries per launch: the grid's second dimension
constexpr size_t kBatchScratch = (size_t)256 << 20;  // ... and the cap on a chunk's totals

// in: the rows of this level, `row_stride` values apart; row_idx / root_idx: which row and root query q reads (null: its own)
__global__ void __launch_bounds__(kPolyBlock) k_pb_scan(const uint32_t* __restrict__ in, uint32_t n, size_t row_stride,
                                                        const uint32_t* __restrict__ row_idx, const uint32_t* __restrict__ roots,
                                                        const uint32_t* __restrict__ root_idx, uint32_t* __restrict__ totals,
                                                        size_t totals_stride, uint32_t* __restrict__ next_roots) {
  __shared__ Fr29 sh[2][kPolyBlock];
  const uint32_t lane = threadIdx.x, b = blockIdx.x, q = blockIdx.y, i = b * kPolyBlock + lane;
  const uint32_t len = Scan::block_len(b, n);
  const uint32_t* row = in + 8 * row_stride * (size_t)(row_idx ? row_idx[q] : q);
  Fr29 a_pow = ld_fr(roots + 8 * (size_t)(root_idx ? root_idx[q] : q));
  Fr29 s = lane < len ? ld_fr(row + 8 * (size_t)i) : fr29_zero();
#pragma unroll 1
  for (uint32_t step = 0; step < Scan::steps(); ++step) {
    sh[step & 1u][lane] = s;
    __syncthreads();
    if (Scan::has_partner(lane, step, len)) s = poly_scan_step(s, sh[step & 1u][lane + Scan::distance(step)], a_pow, step);
    a_pow = fr29_mul(a_pow, a_pow);
  }
  if (lane == 0) {
    st_fr(totals + 8 * (totals_stride * (size_t)q + b), s);
    if (b == 0 && next_roots) st_fr(next_roots + 8 * (size_t)q, a_pow);  // a^256
  }
}

namespace {

struct BatchLevels {
  uint32_t count;              // levels that run (the last one has a single block per query)
  uint32_t len[kBatchLevels];  // values per query of each
};

BatchLevels batch_levels_of(size_t n) {
  BatchLevels lv;
  lv.count = 0;
  for (size_t m = n;; m = Scan::blocks((uint32_t)m)) {
    lv.len[lv.count++] = (uint32_t)m;
    if (Scan::blocks((uint32_t)m) == 1) break;
  }
  return lv;
}

size_t round32(size_t b) { return (b + 31) / 32 * 32; }

}  // namespace

int poly_enqueue_eval_many(snarkv_ctx* ctx, const void* d_polys, size_t n, const void* d_points, const uint32_t* q_poly,
                           const uint32_t* q_point, size_t count, void* d_out) {
  const BatchLevels lv = batch_levels_of(n);
  size_t per_query = 0;  // bytes of one query's roots and totals above level 0
  for (uint32_t l = 1; l < lv.count; ++l) per_query += 32 * ((size_t)lv.len[l] + 1);
  const size_t chunk = std::min(count, std::max<size_t>(1, std::min(kBatchGridY, kBatchScratch / std::max<size_t>(per_query, 1))));
  // the slot: q_poly | q_point of the chunk, then per level l >= 1 the roots (chunk x 32) and the totals (chunk x len[l] x 32)
  const size_t idx_bytes = round32(4 * chunk);
  size_t off_root[kBatchLevels], off_tot[kBatchLevels], off = 2 * idx_bytes;
  for (uint32_t l = 1; l < lv.count; ++l) {
    off_root[l] = off;
    off += 32 * chunk;
    off_tot[l] = off;
    off += 32 * chunk * (size_t)lv.len[l];
  }
  void* d_scr;
  SNARKV_TRY(ctx_reserve(ctx, SLOT_POLY_BATCH, off, &d_scr));
  uint8_t* scr = (uint8_t*)d_scr;
  hipStream_t s = ctx->stream;
  for (size_t q0 = 0; q0 < count; q0 += chunk) {
    const size_t c = std::min(chunk, count - q0);
    // host arrays in pageable memory: the copies have left them when hipMemcpyAsync returns
    SNARKV_HIP(hipMemcpyAsync(scr, q_poly + q0, 4 * c, hipMemcpyHostToDevice, s));
    SNARKV_HIP(hipMemcpyAsync(scr + idx_bytes, q_point + q0, 4 * c, hipMemcpyHostToDevice, s));
    for (uint32_t l = 0; l < lv.count; ++l) {
      const bool last = l + 1 == lv.count;
      const uint32_t* in = l == 0 ? (const uint32_t*)d_polys : (const uint32_t*)(scr + off_tot[l]);
      const size_t stride = l == 0 ? n : lv.len[l];
      const uint32_t* row_idx = l == 0 ? (const uint32_t*)scr : nullptr;
      const uint32_t* roots = l == 0 ? (const uint32_t*)d_points : (const uint32_t*)(scr + off_root[l]);
      const uint32_t* root_idx = l == 0 ? (const uint32_t*)(scr + idx_bytes) : nullptr;
      uint32_t* totals = last ? (uint32_t*)d_out + 8 * q0 : (uint32_t*)(scr + off_tot[l + 1]);
      const size_t tstride = last ? 1 : lv.len[l + 1];
      uint32_t* next_roots = last ? nullptr : (uint32_t*)(scr + off_root[l + 1]);
      hipLaunchKernelGGL(k_pb_scan, dim3(Scan::blocks(lv.len[l]), (uint32_t)c), dim3(kPolyBlock), 0, s, in, lv.len[l], stride,
                         row_idx, roots, root_idx, totals, tstride, next_roots);
    }
    SNARKV_HIP(hipGetLastError());
  }
  return SNARKV_OK;
}

}  // namespace snarkv

using namespace snarkv;

extern "C" {

int SNARKV_API(poly_eval_many_dev)(snarkv_ctx* ctx, const void* d_polys32, size_t n, size_t n_polys, const void* d_points32,
                                   size_t n_points, const uint32_t* q_poly, const uint32_t* q_point, size_t count,
                                   void* d_out32) {
  if (!ctx || !q_poly || !q_point || !aligned16(d_polys32) || !aligned16(d_points32) || !aligned16(d_out32)) return SNARKV_ERR_ARG;
  SNARKV_TRY(check_len(n, kPolyMaxLen));
  if (count == 0 || n_polys == 0 || n_points == 0) return SNARKV_ERR_EMPTY;
  const bool none_ok = false;
  const void* const out = d_out32;
  const size_t out_bytes = bytes_of(count);
  SNARKV_TRY(check_columns("poly_eval_many", d_polys32, n, n_polys, &q_poly, 1, &none_ok, count, &out, &out_bytes, 1));
  for (size_t i = 0; i < count; ++i)
    if (q_point[i] >= n_points) {
      set_last_error("poly_eval_many: point index %u at %zu, there are %zu points", q_point[i], i, n_points);
      return SNARKV_ERR_ARG;
    }
  if (overlap(d_out32, out_bytes, d_points32, bytes_of(n_points))) return refuse_overlap("poly_eval_many", "the results and the points");
  SNARKV_HIP(hipSetDevice(ctx->device));
  return poly_enqueue_eval_many(ctx, d_polys32, n, d_points32, q_poly, q_point, count, d_out32);
}

}  // extern "C"
