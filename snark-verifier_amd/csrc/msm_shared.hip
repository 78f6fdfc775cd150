// Many scalar vectors against ONE resident key:  out[a] = sum_{j < n} s[a][j] G[j],  a < m.
//
// Every base is fixed and shared by all the vectors, so the key keeps its shifted copies on the device,
//     T[w][j] = 2^(8 w) G[j],  w < 32   (affine, the packed Montgomery form the Pippenger gathers; identity rows stay zero)
// and with the signed 8-bit digits of msm_shared.h
//     sum_j s_j G[j] = sum_j sum_w d_{j,w} T[w][j]
// is an MSM of 32 n entries into ONE set of 128 buckets per vector: no doublings, no per-window reduce, no shift chains
// and no per-vector launch.  (The Pippenger of msm_pippenger.hip pays a chain of about ten dependent launches per vector,
// of the order of a millisecond at any size: DESIGN.md section 3d.)
//
//   k_shared_table   one lane per base: a chain of 8 x 31 Jacobian doublings, the 32 points of the chain normalised with
//                    ONE inversion per workgroup (Montgomery's trick along the lane's chain, then across the 64 lanes)
//   k_shared_msm     one 64-lane workgroup per (vector, slice of its terms):
//                      recode the slice's scalars, counting sort of the non-zero digits by bucket in LDS;
//                      cut every bucket's list into pieces of at most L = ceil(entries / 64) entries: at most
//                      128 + 64 pieces, three per lane, so the time of a slice does not depend on how the digits fall
//                      (the all-ones polynomial puts every entry into bucket 1);
//                      every lane walks its pieces with the fast mixed addition, a degenerate result is redone carefully
//                      (equal and opposite points, a piece that sums to the identity); identity rows are skipped;
//                      the pieces of a bucket are stitched by a segmented suffix scan (steps without work are skipped);
//                      sum_b b B_b by the running-sum identity over 64 lanes x 2 buckets -> one XYZZ partial per slice
//   k_shared_blind   (blinded commitments) one wavefront per vector: blind * S against the 32 rows 2^(8 w) S, one digit of
//                    the blind per lane (msm_blind.h) -> one more XYZZ partial per vector, beside k_shared_msm on a lane
//   k_final          (msm_pippenger.hip, launch_fold_partials_many) folds the slices of every vector to its affine point
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include "ctx.hpp"
#include "g1_29.h"
#include "msm_shared.h"
#include "msm_blind.h"

namespace snarkv {

constexpr uint32_t kShLanes = 64;
constexpr uint32_t kShMaxTerms = 128;                        // terms of a slice
constexpr uint32_t kShMaxEntries = kShMaxTerms * kSharedW;   // 4096 digits: 16 KiB of LDS
constexpr uint32_t kShSlots = kSharedBuckets + kShLanes;     // pieces of a slice: sum_b ceil(c_b / L) <= 128 + E / L
constexpr uint32_t kShRounds = kShSlots / kShLanes;          // pieces per lane
constexpr uint32_t kShNoBucket = 0xFFFFu;
constexpr uint32_t kShNeg = 0x80000000u;                     // entry: bit 31 = negate, low bits = w * nkey + j
constexpr uint32_t kTableChunk = 16384;                      // bases per k_shared_table launch (bounds its staging)
constexpr size_t kShPartialsCap = (size_t)64 << 20;          // partials of one group of vectors
constexpr uint32_t kShMaxGroup = 32768;                      // vectors per launch (grid.y)
constexpr uint32_t kShFillWorkgroups = 2048;                 // slices = 0: 256 CUs x several workgroups

// a chain point before normalisation, and the product of the Z of the chain points before it
struct ShTableTmp {
  Fq29 x, y, z, pre;
};

__global__ void __launch_bounds__(64)
    k_shared_table(const uint32_t* __restrict__ key, uint32_t j0, uint32_t count, uint32_t nkey, ShTableTmp* __restrict__ tmp,
                   G1Packed* __restrict__ table) {
  __shared__ Fq29 sh_tot[64], sh_pre[64], sh_inv[64];
  const uint32_t lane = threadIdx.x, t = blockIdx.x * 64u + lane;
  const bool live = t < count;
  G1Affine29 p;
  p.x = fq29_zero();
  p.y = fq29_zero();
  if (live) {
    uint32_t w[16];
    const uint4* src = reinterpret_cast<const uint4*>(key + 16 * (size_t)(j0 + t));
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const uint4 v = src[q];
      w[4 * q] = v.x, w[4 * q + 1] = v.y, w[4 * q + 2] = v.z, w[4 * q + 3] = v.w;
    }
    p = g1a29_from_canonical(w);
  }
  // windows >= dead_from are identity rows: the whole chain of an identity base; a point whose chain reaches Z = 0 cannot
  // be on the curve (the group has odd order) and must not poison the workgroup's shared inversion
  int dead_from = (!live || g1a29_is_identity(p)) ? 0 : kSharedW;
  Fq29 x = p.x, y = p.y, z = fq29_one(), pre = fq29_one();
#pragma unroll 1
  for (int w = 0; w < kSharedW; ++w) {
    if (w < dead_from && w > 0) {
#pragma unroll 1
      for (int d = 0; d < kSharedC; ++d) jac29_double(x, y, z);
      if (fq29_is_zero_mod_p(z)) dead_from = w;
    }
    if (live) {
      ShTableTmp q;
      q.x = x;
      q.y = y;
      q.z = w < dead_from ? z : fq29_one();
      q.pre = pre;
      tmp[(size_t)w * count + t] = q;
      pre = fq29_mul(pre, q.z);
    }
  }
  // one inversion for the workgroup: prefix products over the lanes' totals, invert, walk back
  sh_tot[lane] = pre;
  __syncthreads();
  if (lane == 0) {
    Fq29 acc = fq29_one();
#pragma unroll 1
    for (int i = 0; i < 64; ++i) {
      sh_pre[i] = acc;
      acc = fq29_mul(acc, sh_tot[i]);
    }
    Fq29 inv = fq29_inv(acc);
#pragma unroll 1
    for (int i = 63; i >= 0; --i) {
      sh_inv[i] = fq29_mul(inv, sh_pre[i]);
      inv = fq29_mul(inv, sh_tot[i]);
    }
  }
  __syncthreads();
  if (!live) return;
  Fq29 inv = sh_inv[lane];  // 1 / (Z_0 ... Z_31) of this lane's chain
#pragma unroll 1
  for (int w = kSharedW - 1; w >= 0; --w) {
    const ShTableTmp q = tmp[(size_t)w * count + t];
    const Fq29 iz = fq29_mul(inv, q.pre);  // 1 / Z_w
    inv = fq29_mul(inv, q.z);
    G1Packed out;
    if (w < dead_from) {
      const Fq29 iz2 = fq29_sqr(iz);
      const Fq29 iz3 = fq29_mul(iz2, iz);
      G1Affine29 a;
      a.x = fq29_canon_residue(fq29_mul(q.x, iz2));
      a.y = fq29_canon_residue(fq29_mul(q.y, iz3));
      out = g1a29_pack(a);
    } else {
#pragma unroll
      for (int i = 0; i < 16; ++i) out.w[i] = 0u;
    }
    table[(size_t)w * nkey + j0 + t] = out;
  }
}

__device__ __forceinline__ bool packed_is_identity(const G1Packed& k) {
  uint32_t o = 0;
#pragma unroll
  for (int i = 0; i < 16; ++i) o |= k.w[i];
  return o == 0;
}

__device__ __forceinline__ G1Affine29 shared_entry_point(const G1Packed& k, uint32_t e) {
  G1Affine29 p = g1a29_unpack(k);
  if (e & kShNeg) p.y = fq29_neg(p.y);
  return p;
}

// the careful recomputation of one piece (a fast addition met P = +-Q, or the piece sums to the identity); the result goes
// to memory, not back by value (msm_pippenger.hip, bucket_from_entries_careful)
__device__ __noinline__ void shared_piece_careful(const uint32_t* ent, const G1Packed* __restrict__ table, uint32_t first,
                                                  uint32_t len, G1Xyzz29* out) {
  G1Xyzz29 acc = xyzz29_identity();
  for (uint32_t e = 0; e < len; ++e) {
    const uint32_t v = ent[first + e];
    xyzz29_madd_careful(acc, shared_entry_point(table[v & ~kShNeg], v));
  }
  *out = xyzz29_sanitize(acc);
}

__device__ __forceinline__ void load_scalar(const uint32_t* __restrict__ p, uint32_t s[8]) {
  const uint4* q = reinterpret_cast<const uint4*>(p);
  const uint4 a = q[0], b = q[1];
  s[0] = a.x, s[1] = a.y, s[2] = a.z, s[3] = a.w, s[4] = b.x, s[5] = b.y, s[6] = b.z, s[7] = b.w;
  shared_reduce_mod_r(s);
}

// grid (slices, vectors).  Slice s of vector a holds terms [s tps, min(n, (s + 1) tps)), tps <= kShMaxTerms; its partial
// goes to partials[a * pstride + s]  (pstride = slices, or slices + 1 when k_shared_blind fills one more).
__global__ void __launch_bounds__(64)
    k_shared_msm(const uint32_t* __restrict__ scalars, uint32_t n, uint32_t tps, const G1Packed* __restrict__ table,
                 uint32_t nkey, uint32_t pstride, G1Xyzz29* __restrict__ partials) {
  __shared__ uint32_t ent[kShMaxEntries];
  __shared__ G1Xyzz29 part[kShSlots];
  __shared__ uint32_t cnt[kSharedBuckets], cur[kSharedBuckets], off[kSharedBuckets + 1], pbase[kSharedBuckets + 1];
  __shared__ uint32_t sbucket[kShSlots];
  __shared__ uint32_t piece_len;
  const uint32_t lane = threadIdx.x;
  const uint32_t j_lo = blockIdx.x * tps, j_hi = min(n, j_lo + tps);
  const uint32_t* vec = scalars + 8 * (size_t)blockIdx.y * n;

  // ---- digits -> counting sort by bucket
  for (uint32_t b = lane; b < (uint32_t)kSharedBuckets; b += kShLanes) cnt[b] = 0;
  __syncthreads();
  for (uint32_t j = j_lo + lane; j < j_hi; j += kShLanes) {
    uint32_t s[8];
    load_scalar(vec + 8 * (size_t)j, s);
    shared_recode_each(s, [&](int, int d) {
      if (d != 0) atomicAdd(&cnt[(d < 0 ? -d : d) - 1], 1u);
    });
  }
  __syncthreads();
  if (lane == 0) {
    uint32_t total = 0;
    for (int b = 0; b < kSharedBuckets; ++b) {
      off[b] = total;
      cur[b] = total;
      total += cnt[b];
    }
    off[kSharedBuckets] = total;
    const uint32_t L = max(1u, (total + kShLanes - 1) / kShLanes);
    piece_len = L;
    uint32_t np = 0;
    for (int b = 0; b < kSharedBuckets; ++b) {
      pbase[b] = np;
      np += (cnt[b] + L - 1) / L;
    }
    pbase[kSharedBuckets] = np;  // <= 128 + total / L <= kShSlots
  }
  __syncthreads();
  for (uint32_t j = j_lo + lane; j < j_hi; j += kShLanes) {
    uint32_t s[8];
    load_scalar(vec + 8 * (size_t)j, s);
    shared_recode_each(s, [&](int w, int d) {
      if (d != 0) {
        const uint32_t pos = atomicAdd(&cur[(d < 0 ? -d : d) - 1], 1u);
        if (pos < kShMaxEntries) ent[pos] = (d < 0 ? kShNeg : 0u) | ((uint32_t)w * nkey + j);
      }
    });
  }
  __syncthreads();

  // ---- accumulate: piece `slot` = entries [off[b] + i L, ...) of bucket b, i = slot - pbase[b]
  const uint32_t L = piece_len, npieces = min(pbase[kSharedBuckets], kShSlots);
#pragma unroll 1
  for (uint32_t r = 0; r < kShRounds; ++r) {
    const uint32_t slot = r * kShLanes + lane;
    uint32_t first = 0, len = 0, b = kShNoBucket;
    if (slot < npieces) {
      uint32_t lo = 0, hi = kSharedBuckets;  // the largest b with pbase[b] <= slot
      while (hi - lo > 1) {
        const uint32_t mid = (lo + hi) >> 1;
        if (pbase[mid] <= slot) lo = mid;
        else hi = mid;
      }
      b = lo;
      const uint32_t i = slot - pbase[b];
      first = off[b] + i * L;
      len = min(L, cnt[b] - i * L);
    }
    G1Xyzz29 acc = xyzz29_identity();
    bool started = false;
    G1Packed nxt;
    if (len) nxt = table[ent[first] & ~kShNeg];
#pragma unroll 1
    for (uint32_t e = 0; e < len; ++e) {
      const G1Packed pk = nxt;
      const uint32_t v = ent[first + e];
      if (e + 1 < len) nxt = table[ent[first + e + 1] & ~kShNeg];  // the next gather is issued before this addition
      if (!packed_is_identity(pk)) {
        const G1Affine29 q = shared_entry_point(pk, v);
        if (!started) {
          acc = xyzz29_from_affine(q);
          started = true;
        } else {
          xyzz29_madd_fast(acc, q);
        }
      }
    }
    if (started && xyzz29_is_degenerate(acc)) shared_piece_careful(ent, table, first, len, &part[slot]);
    else part[slot] = acc;
    sbucket[slot] = b;
  }
  __syncthreads();

  // ---- stitch the pieces of every bucket: segmented suffix scan over the slots (the pieces of a bucket are contiguous).
  // Rounds ascend, so what a round reads (slots above its own) has not been written in this step.
#pragma unroll 1
  for (uint32_t step = 0; (1u << step) < kShSlots; ++step) {
    const uint32_t d = 1u << step;
#pragma unroll 1
    for (uint32_t r = 0; r < kShRounds; ++r) {
      const uint32_t slot = r * kShLanes + lane;
      const bool has = slot + d < kShSlots && sbucket[slot] != kShNoBucket && sbucket[slot + d] == sbucket[slot];
      if (__any(has)) {  // uniform: the workgroup is one wavefront
        G1Xyzz29 y = xyzz29_identity();
        if (has) y = part[slot + d];
        __syncthreads();
        G1Xyzz29 x = part[slot];
        xyzz29_add_careful(x, y);
        part[slot] = x;
        __syncthreads();
      }
    }
  }

  // ---- sum_b b B_b: lane l holds magnitudes 2l + 1 and 2l + 2;  run = B_lo + B_hi,  acc = B_lo + 2 B_hi,
  //      sum = sum_l acc_l + 2 sum_{l >= 1} Sfx_l,  Sfx_l = sum_{k >= l} run_k   (msm_pippenger.hip, wave_weighted_fold)
  G1Xyzz29 run = xyzz29_identity(), hi_b = xyzz29_identity(), acc;
  if (cnt[2 * lane]) run = part[pbase[2 * lane]];
  if (cnt[2 * lane + 1]) hi_b = part[pbase[2 * lane + 1]];
  __syncthreads();
  G1Xyzz29* sh = part;  // the buckets are in registers: the fold's exchange buffer takes their place
#pragma unroll 1
  for (int k = 0; k < 2; ++k) {
    G1Xyzz29 x = run;
    xyzz29_add_careful(x, hi_b);
    if (k == 0) run = x;
    else acc = x;
  }
  G1Xyzz29 x = run;
#pragma unroll 1
  for (int step = 0; step < 13; ++step) {
    sh[lane] = x;
    __syncthreads();
    G1Xyzz29 y = xyzz29_identity();
    if (step == 6) {
      if (lane == 0) x = xyzz29_identity();
      else if (!xyzz29_is_identity(x)) x = xyzz29_double(x);
      y = acc;
    } else {
      const uint32_t d = 1u << (step < 6 ? step : step - 7);
      if (lane + d < kShLanes) y = sh[lane + d];
    }
    __syncthreads();
    xyzz29_add_careful(x, y);
  }
  if (lane == 0) partials[(size_t)blockIdx.y * pstride + blockIdx.x] = xyzz29_sanitize(x);
}

// grid (vectors), one wavefront each: partials[a * pstride + slot] = blinds[a] * S from rows[w] = 2^(8 w) S.  Lane w < 32
// takes digit w of the blind (reduced mod r first, so no carry leaves window 31); the arithmetic is msm_blind.h's.
__global__ void __launch_bounds__(64)
    k_shared_blind(const uint32_t* __restrict__ blinds, const G1Packed* __restrict__ rows, uint32_t pstride, uint32_t slot,
                   G1Xyzz29* __restrict__ partials) {
  __shared__ G1Xyzz29 sh[kSharedW];
  const uint32_t lane = threadIdx.x;
  if (lane < (uint32_t)kSharedW) {
    uint32_t s[8];
    load_scalar(blinds + 8 * (size_t)blockIdx.x, s);
    sh[lane] = blind_lane_point(rows[lane], blind_digit(s, (int)lane));
  }
  __syncthreads();
#pragma unroll 1
  for (uint32_t half = kSharedW / 2; half >= 1; half >>= 1) {
    blind_fold_level(sh, lane, half);
    __syncthreads();
  }
  if (lane == 0) partials[(size_t)blockIdx.x * pstride + slot] = sh[0];
}

bool ipa_dk_table_fits(const snarkv_ipa_dk* dk) {
  if (dk->first != 0 || dk->count != ((size_t)1 << dk->k)) return false;  // a shard keeps the per-vector route
  return dk->count * kSharedW * sizeof(G1Packed) <= kSharedTableCap;
}

int ipa_dk_table_prepare(snarkv_ctx* ctx, const snarkv_ipa_dk* dk, bool* have) {
  std::lock_guard<std::mutex> lk(dk->table_mu);
  *have = dk->table_state == 1;
  if (dk->table_state != 0) return SNARKV_OK;
  if (!ipa_dk_table_fits(dk)) {
    dk->table_state = 2;
    return SNARKV_OK;
  }
  const size_t n = dk->count, bytes = n * kSharedW * sizeof(G1Packed);
  const size_t chunk = std::min<size_t>(n, kTableChunk);
  void *d_table = nullptr, *d_tmp = nullptr;
  if (hipMalloc(&d_table, bytes) != hipSuccess || hipMalloc(&d_tmp, chunk * kSharedW * sizeof(ShTableTmp)) != hipSuccess) {
    (void)hipGetLastError();
    if (d_table) (void)hipFree(d_table);
    dk->table_state = 2;  // no room for the table: the per-vector route serves this key
    return SNARKV_OK;
  }
  hipError_t e = hipSuccess;
  for (size_t j0 = 0; j0 < n && e == hipSuccess; j0 += chunk) {
    const uint32_t cnt = (uint32_t)std::min(chunk, n - j0);
    hipLaunchKernelGGL(k_shared_table, dim3((cnt + 63) / 64), dim3(64), 0, ctx->stream, (const uint32_t*)dk->d_points,
                       (uint32_t)j0, cnt, (uint32_t)n, (ShTableTmp*)d_tmp, (G1Packed*)d_table);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);  // other threads read the table from their own streams
  (void)hipFree(d_tmp);
  if (e != hipSuccess) {
    (void)hipFree(d_table);
    set_last_error("ipa_dk_prepare: %s", hipGetErrorString(e));
    return SNARKV_ERR_DEVICE;
  }
  dk->d_table = d_table;
  dk->table_bytes = bytes;
  dk->table_state = 1;
  *have = true;
  return SNARKV_OK;
}

// slices of a vector of n terms when m vectors share the launch
static uint32_t shared_slices(size_t n, size_t m, uint32_t slices) {
  const size_t s_min = (n + kShMaxTerms - 1) / kShMaxTerms;
  size_t s = slices ? std::min<size_t>(slices, n) : s_min;
  if (!slices)
    while (m * s < kShFillWorkgroups && (n + s - 1) / s > 16) s *= 2;  // no slice below 16 terms: its fold costs as much
  return (uint32_t)std::max(s, s_min);
}

// The rows 2^(8 w) S of the blind term, kept with the context: built on its stream when S differs from the one they were built
// for (k_shared_table over the one-point key {S}: a chain of 248 doublings on one lane, once per S and not per call), read by
// this stream and by the lane forked from it only.  Layout of the slot: rows | S | the table kernel's staging.
constexpr size_t kBlindRowsBytes = kSharedW * sizeof(G1Packed);

static int shared_blind_rows(snarkv_ctx* ctx, const uint8_t* s64, const G1Packed** rows) {
  void* d;
  SNARKV_TRY(ctx_reserve(ctx, SLOT_BLIND_ROWS, kBlindRowsBytes + 64 + kSharedW * sizeof(ShTableTmp), &d));  // never grows
  uint8_t* base = (uint8_t*)d;
  *rows = (const G1Packed*)base;
  if (ctx->blind_rows_ready && memcmp(ctx->blind_s, s64, 64) == 0) return SNARKV_OK;
  ctx->blind_rows_ready = false;
  memcpy(ctx->blind_s, s64, 64);
  // from the context's own copy: it outlives the transfer
  SNARKV_HIP(hipMemcpyAsync(base + kBlindRowsBytes, ctx->blind_s, 64, hipMemcpyHostToDevice, ctx->stream));
  hipLaunchKernelGGL(k_shared_table, dim3(1), dim3(64), 0, ctx->stream, (const uint32_t*)(base + kBlindRowsBytes), 0u, 1u, 1u,
                     (ShTableTmp*)(base + kBlindRowsBytes + 64), (G1Packed*)base);
  SNARKV_HIP(hipGetLastError());
  ctx->blind_rows_ready = true;
  return SNARKV_OK;
}

// d_blinds = m canonical scalars and s64 = the point S (host), or both null: no blind term
static int msm_shared_run(snarkv_ctx* ctx, const snarkv_ipa_dk* dk, const void* d_scalars, size_t n, size_t m, uint32_t slices,
                          const void* d_blinds, const uint8_t* s64, void* d_out64s) {
  if (!dk->d_table || n == 0 || n > dk->count || m == 0) return SNARKV_ERR_ARG;
  const uint32_t tps = (uint32_t)((n + shared_slices(n, m, slices) - 1) / shared_slices(n, m, slices));
  const uint32_t S = (uint32_t)((n + tps - 1) / tps);  // no empty slice
  const uint32_t P = S + (d_blinds ? 1u : 0u);         // partials of a vector: its slices, then the blind term
  const size_t group = std::min<size_t>({m, (size_t)kShMaxGroup, std::max<size_t>(1, kShPartialsCap / (P * sizeof(G1Xyzz29)))});
  void* d_parts;
  SNARKV_TRY(ctx_reserve(ctx, SLOT_TERM_PARTIALS, group * P * sizeof(G1Xyzz29), &d_parts));
  const G1Packed* rows = nullptr;
  // the blind kernel runs beside k_shared_msm on the first lane (a lane has none of its own: there it goes first)
  const bool beside = d_blinds && !ctx->is_lane;
  if (d_blinds) SNARKV_TRY(shared_blind_rows(ctx, s64, &rows));
  if (beside) SNARKV_TRY(ctx_lanes(ctx));
  for (size_t a0 = 0; a0 < m; a0 += group) {
    const size_t g = std::min(group, m - a0);
    if (d_blinds) {
      hipStream_t bs = ctx->stream;
      if (beside) {  // after everything enqueued so far: the rows, the blinds, the last fold that read these partials
        bs = ctx->sub[0]->stream;
        SNARKV_HIP(hipEventRecord(ctx->sub_ev[4], ctx->stream));
        SNARKV_HIP(hipStreamWaitEvent(bs, ctx->sub_ev[4], 0));
      }
      hipLaunchKernelGGL(k_shared_blind, dim3((uint32_t)g), dim3(kShLanes), 0, bs, (const uint32_t*)d_blinds + 8 * a0, rows, P, S,
                         (G1Xyzz29*)d_parts);
      SNARKV_HIP(hipGetLastError());
      if (beside) SNARKV_HIP(hipEventRecord(ctx->sub_ev[0], bs));
    }
    hipLaunchKernelGGL(k_shared_msm, dim3(S, (uint32_t)g), dim3(kShLanes), 0, ctx->stream,
                       (const uint32_t*)d_scalars + 8 * a0 * n, (uint32_t)n, tps, (const G1Packed*)dk->d_table,
                       (uint32_t)dk->count, P, (G1Xyzz29*)d_parts);
    SNARKV_HIP(hipGetLastError());
    if (beside) SNARKV_HIP(hipStreamWaitEvent(ctx->stream, ctx->sub_ev[0], 0));
    SNARKV_TRY(launch_fold_partials_many(ctx, d_parts, P, g, (uint8_t*)d_out64s + 64 * a0));
  }
  return SNARKV_OK;
}

int launch_msm_shared(snarkv_ctx* ctx, const snarkv_ipa_dk* dk, const void* d_scalars, size_t n, size_t m, uint32_t slices,
                      void* d_out64s) {
  return msm_shared_run(ctx, dk, d_scalars, n, m, slices, nullptr, nullptr, d_out64s);
}

int launch_msm_shared_blinded(snarkv_ctx* ctx, const snarkv_ipa_dk* dk, const void* d_scalars, size_t n, size_t m,
                              uint32_t slices, const void* d_blinds, const uint8_t* s64, void* d_out64s) {
  if (!d_blinds || !s64) return SNARKV_ERR_ARG;
  return msm_shared_run(ctx, dk, d_scalars, n, m, slices, d_blinds, s64, d_out64s);
}

}  // namespace snarkv
