// The lookup argument on resident columns (include/snarkv_lookup.h): the sort of scalars, halo2's permute_expression_pair
// and the lookup product Z.  Same source for both curves, as poly_prod.hip; the comparison, the merge-path partition, the
// flags and the tie rule are in lookup.h.
//
// The sort is a merge sort, so its cost does not depend on the data: kLkTile = 1024 elements per workgroup, 256 lanes of 4.
//   k_lk_tile_sort   a tile is reduced to canonical words on its way into LDS and sorted there: log2(1024) rounds that merge
//                    runs in pairs by ranks (lk_tile_dest: an element's place is its index in its run plus a binary search
//                    in the other run); a lane holds its four keys over the barrier between the reads and the writes of a
//                    round, so one buffer does
//   k_lk_partition   one lane per output chunk of a merge pass: the merge-path search on the chunk's diagonal, in global
//                    memory, into the slot
//   k_lk_merge       one workgroup per chunk: the two input ranges between its partition point and the next are staged in
//                    LDS, every lane finds the diagonal of its four outputs there (the same lk_merge_path) and merges them
//                    serially (lk_take_a); the odd run at the end of a pass has an empty partner and is copied by the same
//                    code
// LDS holds keys word-major: word k of key i at sh[k * 1024 + i], so lanes that read consecutive keys read consecutive
// banks, where a 32-byte stride would put them 8 ways on the same ones.  32 KiB per workgroup.
// The passes ping-pong between `out` and `work`; the tiles go to the one that makes the last pass land in `out`.
//
// The permuted columns: A' = sort(A) into perm_input, sort(S) into work[0, u), then
//   k_lk_flag        the flags of every row (lk_flags: repeated row of A', leftover of the sorted table; the membership test
//                    is a binary search in A' for the first of each table value) as one byte per row, and the block's counts
//   k_lk_up, k_lk_down   the additive scan of the counts over the levels; the top block writes the totals and the status
//   k_lk_compact     the leftovers in order into work[u, 2u)
//   k_lk_gather      perm_table[i] = A'[i] on a first row, the leftover lk_leftover_of(R, rank_i) on a repeated one
#include <string.h>
#include "ctx.hpp"
#include "ipa_prover.hpp"
#include "poly_args.hpp"
#include "lookup.h"
#include "../../include/snarkv_lookup.h"
#include "../../include/snarkv_poly_prod.h"

namespace snarkv {

constexpr uint32_t kLkThreads = 256;
constexpr uint32_t kLkLane = 4;                          // elements per lane
constexpr uint32_t kLkTile = kLkThreads * kLkLane;       // elements per sort tile and per merge chunk
constexpr uint32_t kLkScanBlock = kLkThreads * kLkLane;  // rows per block of the count scans, at every level
constexpr uint32_t kLkLevels = 3;                        // 1024^3 >= 2^30
constexpr size_t kLkMaxLen = (size_t)1 << 30;
static_assert(kLkTile == SNARKV_LOOKUP_TILE && kLkScanBlock == SNARKV_LOOKUP_SCAN_BLOCK, "the sizes the header states");
typedef ProdBlock<kLkThreads, kLkLane> LkBlock;

// keys in global memory: two 16-byte loads / stores
struct LkGlobal {
  const uint32_t* p;
  __device__ __forceinline__ LkKey operator()(uint32_t i) const {
    const uint4* s = reinterpret_cast<const uint4*>(p + 8 * (size_t)i);
    const uint4 a = s[0], b = s[1];
    LkKey k;
    k.w[0] = a.x, k.w[1] = a.y, k.w[2] = a.z, k.w[3] = a.w, k.w[4] = b.x, k.w[5] = b.y, k.w[6] = b.z, k.w[7] = b.w;
    return k;
  }
};
__device__ __forceinline__ void lk_store(uint32_t* p, size_t i, const LkKey& k) {
  uint4* o = reinterpret_cast<uint4*>(p + 8 * i);
  o[0] = make_uint4(k.w[0], k.w[1], k.w[2], k.w[3]);
  o[1] = make_uint4(k.w[4], k.w[5], k.w[6], k.w[7]);
}
// keys in LDS, word-major, from key `off` on
struct LkShared {
  const uint32_t* sh;
  uint32_t off;
  __device__ __forceinline__ LkKey operator()(uint32_t i) const {
    LkKey k;
#pragma unroll
    for (int w = 0; w < 8; ++w) k.w[w] = sh[w * kLkTile + off + i];
    return k;
  }
};
__device__ __forceinline__ void lk_put(uint32_t* sh, uint32_t i, const LkKey& k) {
#pragma unroll
  for (int w = 0; w < 8; ++w) sh[w * kLkTile + i] = k.w[w];
}

// `in` may be `out`: a workgroup reads its whole tile before it writes any of it, and touches no other
__global__ void __launch_bounds__(kLkThreads) k_lk_tile_sort(const uint32_t* in, uint32_t n, uint32_t* out) {
  __shared__ uint32_t sh[8 * kLkTile];
  const uint32_t lane = threadIdx.x, base = blockIdx.x * kLkTile, len = n - base < kLkTile ? n - base : kLkTile;
  const LkGlobal src = {in};
  const LkShared tile = {sh, 0};
#pragma unroll
  for (uint32_t j = 0; j < kLkLane; ++j) {
    const uint32_t i = lane + j * kLkThreads;
    if (i < len) lk_put(sh, i, lk_canon(src(base + i).w));
  }
  __syncthreads();
#pragma unroll 1
  for (uint32_t run = 1; run < len; run *= 2) {
    LkKey key[kLkLane];
    uint32_t dest[kLkLane];
#pragma unroll
    for (uint32_t j = 0; j < kLkLane; ++j) {
      const uint32_t i = lane + j * kLkThreads;
      if (i < len) {
        key[j] = tile(i);
        dest[j] = lk_tile_dest(tile, len, run, i, key[j]);
      }
    }
    __syncthreads();
#pragma unroll
    for (uint32_t j = 0; j < kLkLane; ++j)
      if (lane + j * kLkThreads < len) lk_put(sh, dest[j], key[j]);
    __syncthreads();
  }
#pragma unroll
  for (uint32_t j = 0; j < kLkLane; ++j) {
    const uint32_t i = lane + j * kLkThreads;
    if (i < len) lk_store(out, (size_t)base + i, tile(i));
  }
}

// part[c] = how many elements of run a lie before output chunk c of the pass
__global__ void __launch_bounds__(kLkThreads) k_lk_partition(const uint32_t* __restrict__ src, uint32_t n, uint32_t run,
                                                             uint32_t chunks, uint32_t* __restrict__ part) {
  const uint32_t c = blockIdx.x * kLkThreads + threadIdx.x;
  if (c >= chunks) return;
  const LkMergeGeom g = lk_merge_geom(n, run, kLkTile, c);
  const LkGlobal a = {src + 8 * (size_t)g.a0}, b = {src + 8 * (size_t)g.b0};
  part[c] = lk_merge_path(a, g.na, b, g.nb, g.diag);
}

__global__ void __launch_bounds__(kLkThreads) k_lk_merge(const uint32_t* __restrict__ src, uint32_t n, uint32_t run,
                                                         const uint32_t* __restrict__ part, uint32_t* __restrict__ dst) {
  __shared__ uint32_t sh[8 * kLkTile];
  const uint32_t lane = threadIdx.x, c = blockIdx.x, start = c * kLkTile;
  const LkMergeGeom g = lk_merge_geom(n, run, kLkTile, c);
  const uint32_t total = g.na + g.nb, count = total - g.diag < kLkTile ? total - g.diag : kLkTile;
  // the chunk's ranges: from its own partition point to the next chunk's, or to the ends of the runs
  const uint32_t a_lo = part[c], a_hi = g.diag + count == total ? g.na : part[c + 1];
  const uint32_t b_lo = g.diag - a_lo, b_hi = g.diag + count - a_hi;
  const uint32_t ca = a_hi - a_lo, cb = b_hi - b_lo;  // ca + cb = count <= kLkTile
  const LkGlobal ga = {src + 8 * ((size_t)g.a0 + a_lo)}, gb = {src + 8 * ((size_t)g.b0 + b_lo)};
#pragma unroll
  for (uint32_t j = 0; j < kLkLane; ++j) {
    const uint32_t i = lane + j * kLkThreads;
    if (i < count) lk_put(sh, i, i < ca ? ga(i) : gb(i - ca));
  }
  __syncthreads();
  const LkShared a = {sh, 0}, b = {sh, ca};
  const uint32_t d0 = lane * kLkLane;
  if (d0 >= count) return;
  const uint32_t d1 = d0 + kLkLane < count ? d0 + kLkLane : count;
  uint32_t ai = lk_merge_path(a, ca, b, cb, d0), bi = d0 - ai;
#pragma unroll 1
  for (uint32_t d = d0; d < d1; ++d) {
    const bool has_a = ai < ca, has_b = bi < cb;
    // a range that is used up is not read past its end: key 0 of the stage exists (count >= 1) and lk_take_a ignores it
    const LkKey ka = a(has_a ? ai : 0u), kb = has_b ? b(bi) : ka;
    const bool take = lk_take_a(has_a, has_b, ka, kb);
    lk_store(dst, (size_t)start + d, take ? ka : kb);
    ai += take ? 1u : 0u;
    bi += take ? 0u : 1u;
  }
}

// the exclusive scan of one count per lane over the workgroup (poly_prod.h's wg_scan), the block's total through `total`
__device__ __forceinline__ LkCount lk_wg_exclusive(LkCount (&sh)[2][kLkThreads], const LkCount& mine, uint32_t lane, LkCount* total) {
  wg_publish(sh, wg_scan<LkAdd, false>(sh, mine, lane), lane);
  LkCount before;
  before.rep = 0, before.left = 0;
  if (lane) before = sh[0][lane - 1];
  if (total) *total = sh[0][kLkThreads - 1];
  return before;
}

// flags[i] for every i < u, totals[b] = the counts of block b
__global__ void __launch_bounds__(kLkThreads) k_lk_flag(const uint32_t* __restrict__ a, const uint32_t* __restrict__ s, uint32_t u,
                                                        uint8_t* __restrict__ flags, LkCount* __restrict__ totals) {
  __shared__ LkCount sh[2][kLkThreads];
  const uint32_t lane = threadIdx.x, b = blockIdx.x, len = LkBlock::block_len(b, u);
  const LkGlobal ga = {a}, gs = {s};
  LkCount mine;
  mine.rep = 0, mine.left = 0;
#pragma unroll 1
  for (uint32_t j = 0; j < kLkLane; ++j)
    if (LkBlock::has(lane, j, len)) {
      const uint32_t i = LkBlock::index(b, lane, j), f = lk_flags(ga, gs, u, i);
      flags[i] = (uint8_t)f;
      mine = lk_add(mine, lk_count_of(f));
    }
  const LkCount sum = wg_scan<LkAdd, false>(sh, mine, lane);
  if (lane == kLkThreads - 1) totals[b] = sum;
}

__device__ __forceinline__ void lk_load_counts(const LkCount* in, uint32_t b, uint32_t lane, uint32_t len, LkCount* x) {
#pragma unroll
  for (uint32_t j = 0; j < kLkLane; ++j) {
    x[j].rep = 0, x[j].left = 0;
    if (LkBlock::has(lane, j, len)) x[j] = in[LkBlock::index(b, lane, j)];
  }
}

__global__ void __launch_bounds__(kLkThreads) k_lk_up(const LkCount* __restrict__ in, uint32_t n, LkCount* __restrict__ totals) {
  __shared__ LkCount sh[2][kLkThreads];
  const uint32_t lane = threadIdx.x, b = blockIdx.x, len = LkBlock::block_len(b, n);
  LkCount x[kLkLane], p[kLkLane], mine;
  lk_load_counts(in, b, lane, len, x);
  lk_lane_prefix<kLkLane>(x, p, mine);
  const LkCount sum = wg_scan<LkAdd, false>(sh, mine, lane);
  if (lane == kLkThreads - 1) totals[b] = sum;
}

// seq[i] = carry of the block + the counts before i, in place.  The top level has one block and no carries: one lane
// writes the totals and the status, with plain stores.
__global__ void __launch_bounds__(kLkThreads) k_lk_down(LkCount* seq, uint32_t n, const LkCount* __restrict__ carries,
                                                        LkCount* __restrict__ grand, uint32_t* __restrict__ status, uint32_t u) {
  __shared__ LkCount sh[2][kLkThreads];
  const uint32_t lane = threadIdx.x, b = blockIdx.x, len = LkBlock::block_len(b, n);
  LkCount x[kLkLane], p[kLkLane], mine, total;
  lk_load_counts(seq, b, lane, len, x);
  lk_lane_prefix<kLkLane>(x, p, mine);
  LkCount before = lk_wg_exclusive(sh, mine, lane, &total);
  if (carries) before = lk_add(before, carries[b]);
#pragma unroll
  for (uint32_t j = 0; j < kLkLane; ++j)
    if (LkBlock::has(lane, j, len)) seq[LkBlock::index(b, lane, j)] = lk_add(before, p[j]);
  if (grand && lane == 0) {
    *grand = total;
    lk_status(total, u, status);
  }
}

// GATHER false: the leftovers of the sorted table s, in order, into `out` (work[u, 2u)).
// GATHER true:  out[i] = a[i] on a first row, leftovers[lk_leftover_of(R, rank_i)] on a repeated one (src = a = A').
template <bool GATHER>
__global__ void __launch_bounds__(kLkThreads) k_lk_place(const uint32_t* __restrict__ src, const uint8_t* __restrict__ flags,
                                                         uint32_t u, const LkCount* __restrict__ carries,
                                                         const LkCount* __restrict__ grand, const uint32_t* __restrict__ leftovers,
                                                         uint32_t* __restrict__ out) {
  __shared__ LkCount sh[2][kLkThreads];
  const uint32_t lane = threadIdx.x, b = blockIdx.x, len = LkBlock::block_len(b, u);
  LkCount x[kLkLane], p[kLkLane], mine;
#pragma unroll
  for (uint32_t j = 0; j < kLkLane; ++j) {
    x[j].rep = 0, x[j].left = 0;
    if (LkBlock::has(lane, j, len)) x[j] = lk_count_of(flags[LkBlock::index(b, lane, j)]);
  }
  lk_lane_prefix<kLkLane>(x, p, mine);
  const LkCount before = lk_add(lk_wg_exclusive(sh, mine, lane, nullptr), carries[b]);
  const LkGlobal g = {src}, l = {leftovers};
  const uint32_t repeated = GATHER ? grand->rep : 0u;
#pragma unroll
  for (uint32_t j = 0; j < kLkLane; ++j) {
    if (!LkBlock::has(lane, j, len)) continue;
    const uint32_t i = LkBlock::index(b, lane, j);
    const LkCount at = lk_add(before, p[j]);
    if (GATHER) lk_store(out, i, x[j].rep ? l(lk_leftover_of(repeated, at.rep)) : g(i));
    else if (x[j].left) lk_store(out, at.left, g(i));  // at.left < the number of leftovers <= u
  }
}

namespace {

size_t round256(size_t v) { return (v + 255) & ~(size_t)255; }
uint32_t chunks_of(size_t n) { return (uint32_t)((n + kLkTile - 1) / kLkTile); }

// layout of the context's SLOT_LOOKUP: the partition points of the sort's passes; for the permuted columns (rows = u) also
// the flags, the counts of each level of the scan and the totals
struct Layout {
  size_t part, flags, seq[kLkLevels], grand, end;
  uint32_t len[kLkLevels], levels;
};
Layout layout_of(size_t n, size_t rows) {
  Layout l;
  l.part = 0;
  l.flags = round256(4 * ((size_t)chunks_of(n) + 1));
  size_t off = l.flags + round256(rows);
  l.levels = 0;
  uint32_t m = rows ? LkBlock::blocks((uint32_t)rows) : 0;
  while (m) {
    l.len[l.levels] = m;
    l.seq[l.levels] = off;
    off += round256(sizeof(LkCount) * (size_t)m);
    l.levels += 1;
    if (m == 1) break;
    m = LkBlock::blocks(m);
  }
  l.grand = off;
  l.end = off + 256;
  return l;
}

// The enqueue steps; arguments are taken as checked.

int sort_enqueue(snarkv_ctx* ctx, const void* d_in, size_t n, void* d_work, void* d_out) {
  const Layout l = layout_of(n, 0);
  void* scr;
  SNARKV_TRY(ctx_reserve(ctx, SLOT_LOOKUP, l.end, &scr));
  uint32_t* part = (uint32_t*)((uint8_t*)scr + l.part);
  const uint32_t len = (uint32_t)n, chunks = chunks_of(n);
  // the last pass lands in out: the tiles go to out for an even number of passes, to work for an odd one
  uint32_t* cur = (uint32_t*)(lk_passes(len, kLkTile) % 2 ? d_work : d_out);
  hipLaunchKernelGGL(k_lk_tile_sort, dim3(chunks), dim3(kLkThreads), 0, ctx->stream, (const uint32_t*)d_in, len, cur);
  SNARKV_HIP(hipGetLastError());
  for (uint64_t run = kLkTile; run < n; run *= 2) {
    uint32_t* other = cur == (uint32_t*)d_out ? (uint32_t*)d_work : (uint32_t*)d_out;
    hipLaunchKernelGGL(k_lk_partition, dim3((chunks + kLkThreads - 1) / kLkThreads), dim3(kLkThreads), 0, ctx->stream,
                       (const uint32_t*)cur, len, (uint32_t)run, chunks, part);
    hipLaunchKernelGGL(k_lk_merge, dim3(chunks), dim3(kLkThreads), 0, ctx->stream, (const uint32_t*)cur, len, (uint32_t)run,
                       (const uint32_t*)part, other);
    SNARKV_HIP(hipGetLastError());
    cur = other;
  }
  return SNARKV_OK;
}

int permute_enqueue(snarkv_ctx* ctx, const void* d_input, const void* d_table, size_t u, void* d_work, void* d_perm_input,
                    void* d_perm_table, void* d_status) {
  // the largest reservation first: the slot does not move between the steps
  const Layout l = layout_of(u, u);
  void* d;
  SNARKV_TRY(ctx_reserve(ctx, SLOT_LOOKUP, l.end, &d));
  uint8_t* scr = (uint8_t*)d;
  uint32_t* sorted_table = (uint32_t*)d_work;
  uint32_t* leftovers = sorted_table + 8 * u;
  SNARKV_TRY(sort_enqueue(ctx, d_input, u, leftovers, d_perm_input));
  SNARKV_TRY(sort_enqueue(ctx, d_table, u, d_perm_table, sorted_table));
  uint8_t* flags = scr + l.flags;
  LkCount* seq[kLkLevels];
  for (uint32_t i = 0; i < l.levels; ++i) seq[i] = (LkCount*)(scr + l.seq[i]);
  LkCount* grand = (LkCount*)(scr + l.grand);
  const dim3 th(kLkThreads);
  const uint32_t rows = (uint32_t)u, blocks = l.len[0];
  hipLaunchKernelGGL(k_lk_flag, dim3(blocks), th, 0, ctx->stream, (const uint32_t*)d_perm_input, (const uint32_t*)sorted_table,
                     rows, flags, seq[0]);
  for (uint32_t i = 0; i + 1 < l.levels; ++i)
    hipLaunchKernelGGL(k_lk_up, dim3(l.len[i + 1]), th, 0, ctx->stream, (const LkCount*)seq[i], l.len[i], seq[i + 1]);
  for (uint32_t i = l.levels; i-- > 0;) {
    const bool top = i + 1 == l.levels;
    hipLaunchKernelGGL(k_lk_down, dim3(top ? 1u : l.len[i + 1]), th, 0, ctx->stream, seq[i], l.len[i],
                       top ? (const LkCount*)nullptr : (const LkCount*)seq[i + 1], top ? grand : (LkCount*)nullptr,
                       (uint32_t*)d_status, rows);
  }
  hipLaunchKernelGGL(k_lk_place<false>, dim3(blocks), th, 0, ctx->stream, (const uint32_t*)sorted_table, (const uint8_t*)flags,
                     rows, (const LkCount*)seq[0], (const LkCount*)grand, (const uint32_t*)nullptr, leftovers);
  hipLaunchKernelGGL(k_lk_place<true>, dim3(blocks), th, 0, ctx->stream, (const uint32_t*)d_perm_input, (const uint8_t*)flags,
                     rows, (const LkCount*)seq[0], (const LkCount*)grand, (const uint32_t*)leftovers, (uint32_t*)d_perm_table);
  SNARKV_HIP(hipGetLastError());
  return SNARKV_OK;
}

}  // namespace

}  // namespace snarkv

using namespace snarkv;

extern "C" {

int SNARKV_API(poly_sort_dev)(snarkv_ctx* ctx, const void* d_in32, size_t n, void* d_work32, void* d_out32) {
  if (!ctx || !aligned16(d_in32) || !aligned16(d_work32) || !aligned16(d_out32)) return SNARKV_ERR_ARG;
  const size_t bytes = bytes_of(n);
  if (partial_overlap(d_out32, d_in32, bytes))
    return refuse_overlap("poly_sort", "out is the input itself or disjoint from it");
  if (overlap(d_work32, bytes, d_in32, bytes) || overlap(d_work32, bytes, d_out32, bytes))
    return refuse_overlap("poly_sort", "work is disjoint from the input and from out");
  SNARKV_TRY(check_len(n, kLkMaxLen));
  SNARKV_HIP(hipSetDevice(ctx->device));
  return sort_enqueue(ctx, d_in32, n, d_work32, d_out32);
}

int SNARKV_API(lookup_permute_dev)(snarkv_ctx* ctx, const void* d_input32, const void* d_table32, size_t u, void* d_work32,
                                   void* d_perm_input32, void* d_perm_table32, void* d_status) {
  if (!ctx || !aligned16(d_input32) || !aligned16(d_table32) || !aligned16(d_work32) || !aligned16(d_perm_input32) ||
      !aligned16(d_perm_table32) || !aligned16(d_status))
    return SNARKV_ERR_ARG;
  const size_t bytes = bytes_of(u);
  const void* bufs[5] = {d_input32, d_table32, d_work32, d_perm_input32, d_perm_table32};
  const size_t size[5] = {bytes, bytes, 2 * bytes, bytes, bytes};
  for (int i = 0; i < 5; ++i)
    for (int j = i + 1; j < 5; ++j)
      if (overlap(bufs[i], size[i], bufs[j], size[j]))
        return refuse_overlap("lookup_permute", "the input, the table, work and the two outputs are pairwise disjoint");
  for (int i = 2; i < 5; ++i)
    if (overlap(d_status, 16, bufs[i], size[i])) return refuse_overlap("lookup_permute", "the status lies in memory the call writes");
  SNARKV_TRY(check_len(u, kLkMaxLen));
  SNARKV_HIP(hipSetDevice(ctx->device));
  return permute_enqueue(ctx, d_input32, d_table32, u, d_work32, d_perm_input32, d_perm_table32, d_status);
}

int SNARKV_API(lookup_product_dev)(snarkv_ctx* ctx, const void* d_polys32, size_t n, size_t n_polys, uint32_t idx_input,
                                   uint32_t idx_table, uint32_t idx_perm_input, uint32_t idx_perm_table, const uint8_t* beta32,
                                   const uint8_t* gamma32, const void* d_start32, void* d_work32, void* d_z32, void* d_total32) {
  if (!ctx || !aligned16(d_polys32) || !aligned16(d_work32) || !aligned16(d_z32) || !beta32 || !gamma32) return SNARKV_ERR_ARG;
  if ((d_start32 && !aligned16(d_start32)) || (d_total32 && !aligned16(d_total32))) return SNARKV_ERR_ARG;
  const size_t bytes = bytes_of(n), total_bytes = d_total32 ? 32 : 0;
  const uint32_t num_idx[2] = {idx_input, idx_table}, den_idx[2] = {idx_perm_input, idx_perm_table};
  const uint32_t* idx[4] = {num_idx, num_idx + 1, den_idx, den_idx + 1};
  const bool none_ok[4] = {false, false, false, false};
  const void* outs[3] = {d_work32, d_z32, d_total32};
  const size_t out_bytes[3] = {2 * bytes, bytes, total_bytes};
  SNARKV_TRY(check_columns("lookup_product", d_polys32, n, n_polys, idx, 4, none_ok, 1, outs, out_bytes, 3));
  if (overlap(d_work32, 2 * bytes, d_z32, bytes) || overlap(d_total32, total_bytes, d_work32, 2 * bytes) ||
      overlap(d_total32, total_bytes, d_z32, bytes))
    return refuse_overlap("lookup_product", "work, z and the total are disjoint");
  if (d_start32 && (overlap(d_start32, 32, d_work32, 2 * bytes) || overlap(d_start32, 32, d_z32, bytes) ||
                    overlap(d_start32, 32, d_total32, total_bytes)))
    return refuse_overlap("lookup_product", "the start value lies in memory the call writes");
  if (!below_r(beta32) || !below_r(gamma32)) return SNARKV_ERR_ENCODING;
  if (n_polys == 0) return SNARKV_ERR_EMPTY;
  SNARKV_TRY(check_len(n, kLkMaxLen));
  SNARKV_HIP(hipSetDevice(ctx->device));
  // (A + beta)(S + gamma): two affine terms without a beta part, the challenges as their constants
  const uint32_t none[2] = {SNARKV_POLY_NONE, SNARKV_POLY_NONE};
  uint8_t betas[64], gammas[64];
  memset(betas, 0, sizeof betas);
  memcpy(gammas, beta32, 32);
  memcpy(gammas + 32, gamma32, 32);
  uint8_t* num = (uint8_t*)d_work32;
  uint8_t* den = num + 32 * n;
  // the four public calls of snarkv_poly_prod.h, back to back
  SNARKV_TRY(prod_affine_enqueue(ctx, d_polys32, n, num_idx, none, betas, gammas, 2, num));
  SNARKV_TRY(prod_affine_enqueue(ctx, d_polys32, n, den_idx, none, betas, gammas, 2, den));
  SNARKV_TRY(prod_batch_invert_enqueue(ctx, den, n, den));
  SNARKV_TRY(prod_mul_enqueue(ctx, num, den, n, num));
  return prod_grand_product_enqueue(ctx, num, n, d_start32, d_z32, d_total32);
}

}  // extern "C"
