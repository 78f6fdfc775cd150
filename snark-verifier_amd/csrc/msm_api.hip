// The MSM entry layer of both libraries (BN254: snarkv_*, the pasta build: snarkv_pallas_*; SNARKV_API, ctx.hpp):
// the route of a large MSM (single launch or chunk pipeline), the batch scheduler, and the MSM entry points both
// headers declare.  Where the builds differ is data in ctx.hpp (SNARKV_CHUNK_PIPELINE, SNARKV_API_FLAGS).
#include <stdlib.h>
#include <algorithm>
#include "ctx.hpp"
#include "../../include/snarkv_pallas.h"

namespace snarkv {

// THE decision "does an n-point MSM run as the chunk pipeline over shared bucket grids?" -- one rule for the single
// call (launch_msm_pippenger_auto), the batch (launch_msm_pippenger_many hands such jobs to the single call) and
// snarkv_g1_msm_launch_points (what bench.py divides its per-launch roofline by).  *chunk = points per chunk.
//   SNARKV_PIP_SPLIT   0 never, 1 (default) from three chunks, 2 from two
// An explicit window size or a lane context (a worker of a pipeline already) keeps the single launch, and so does
// every MSM of the pasta build (SNARKV_CHUNK_PIPELINE, ctx.hpp).
bool pip_chunk_pipeline(size_t n, int window_bits, bool is_lane, size_t* chunk) {
  const size_t c = (size_t)1 << 20;  // chunk size: the 2^20-point MSM's window geometry, point table inside the Infinity Cache
  const char* e = getenv("SNARKV_PIP_SPLIT");
  const int mode = e ? atoi(e) : 1;
  const size_t min_chunks = mode == 2 ? 2 : 3;
  if (chunk) *chunk = c;
  return SNARKV_CHUNK_PIPELINE && mode != 0 && (n + c - 1) / c >= min_chunks && window_bits == 0 && !is_lane;
}

// LARGE MSMs as a chunk pipeline over ONE bucket grid.
//
// Beyond ~2^21 points the single-launch Pippenger degrades: the Montgomery point table (64 B x 2n) outgrows the
// 256 MiB Infinity Cache, so every bucket-accumulate gather goes to HBM (k_accumulate +11 % per point at 2^24), the
// level-1 partition scatters 8-byte entries into thousands of streams (k_sort_scatter_staged: 3.5x write amplification), and
// level-2 slices no longer fit LDS.  MSM is linear (the reference's own chunking, util/msm.rs:311-336), so n points are
// cut into 2^20-point chunks that all use the window size of a 2^20-point MSM; every chunk runs the efficient small-n
// stages (prepare, partition, sort, bucket accumulate, combine) on one of three worker lanes (private sub-contexts: one
// HIP stream + scratch each) and ADDS its bucket sums into its worker's grid (windows x 2^(c-1) XYZZ points, 36 MiB).
// Chunks on different lanes overlap -- the memory-bound partition of one under the VALU-bound accumulation of another --
// and the latency-bound tail (bucket reduce, 2^(cw) shift chains, to_affine: 0.65 ms) is paid ONCE on the sum of the
// three grids instead of once per chunk.  Same group element, same bytes as the single launch.
// Measured (MI355X, one MSM at a time): 2^22 / 2^24 points, see DESIGN.md section 4.
int launch_msm_pippenger_auto(snarkv_ctx* ctx, const void* d_s, const void* d_p, size_t n, int window_bits, void* d_out,
                              bool partial_out) {
  size_t kChunk = 0;
  const bool split = pip_chunk_pipeline(n, window_bits, ctx->is_lane, &kChunk);
  const size_t chunks = (n + kChunk - 1) / kChunk;
  ctx->last_split_workers = 0;
  ctx->last_many_jobs = 0;
  if (!split) return launch_msm_pippenger(ctx, d_s, d_p, n, window_bits, d_out, partial_out);
  SNARKV_TRY(ctx_lanes(ctx));
  const bool tm = ctx->stage_timing;  // per-stage events: on the worker lanes (their LAST chunk); total on this stream
  if (tm && !ctx->ev_ready) {
    for (int i = 0; i <= SNARKV_PIP_STAGES; ++i) SNARKV_HIP(hipEventCreate(&ctx->ev[i]));
    ctx->ev_ready = true;
  }
  if (tm) SNARKV_HIP(hipEventRecord(ctx->ev[0], ctx->stream));
  uint32_t c = 0, windows = 0, bpw = 0;
  SNARKV_TRY(pip_geometry(kChunk, 0, &c, &windows, &bpw));
  const size_t nb = (size_t)windows * bpw, grid_bytes = nb * SNARKV_G1_PARTIAL_BYTES;
  const int kWorkers = 2;  // 2 vs 3 measured level (2^24: 24.7 vs 25.3 ms); two keep the footprint at ~2 GiB
  void *grid[3], *tmp[3];
  bool started[3] = {false, false, false};
  for (int w = 0; w < kWorkers; ++w) {
    SNARKV_TRY(ctx_reserve(ctx->sub[w], SLOT_MGPU_GRID, grid_bytes, &grid[w]));
    SNARKV_TRY(ctx_reserve(ctx->sub[w], SLOT_MGPU_RECV, grid_bytes, &tmp[w]));
  }
  // inputs may still be in flight on the caller's stream
  SNARKV_TRY(ctx_lanes_fork(ctx));
  for (size_t k = 0; k < chunks; ++k) {
    size_t lo = k * kChunk, len = std::min(kChunk, n - lo);
    int w = (int)(k % kWorkers);
    snarkv_ctx* lane = ctx->sub[w];
    lane->mont = ctx->mont;
    lane->stage_timing = tm;
    // the chunk's bucket sums (sanitised XYZZ, zero = identity): straight into the worker's grid the first time, added to it after
    SNARKV_TRY(launch_msm_pippenger(lane, (const char*)d_s + 32 * lo, (const char*)d_p + 64 * lo, len, (int)c, nullptr, false,
                                    started[w] ? tmp[w] : grid[w]));
    if (started[w]) SNARKV_TRY(launch_buckets_add(lane, grid[w], tmp[w], nb));
    started[w] = true;
  }
  for (int w = 0; w < kWorkers; ++w) ctx->sub[w]->stage_timing = false;
  SNARKV_TRY(ctx_lanes_join(ctx));
  for (int w = 1; w < kWorkers; ++w)
    if (started[w]) SNARKV_TRY(launch_buckets_add(ctx, grid[0], grid[w], nb));
  void* d_part;
  SNARKV_TRY(ctx_reserve(ctx, SLOT_SPLIT_PARTIALS, SNARKV_G1_PARTIAL_BYTES, &d_part));
  ctx->last_split_workers = kWorkers;
  int rc = SNARKV_OK;
  if (partial_out) {
    rc = launch_buckets_reduce(ctx, grid[0], c, 0, windows, d_out);
  } else {
    rc = launch_buckets_reduce(ctx, grid[0], c, 0, windows, d_part);
    if (rc == SNARKV_OK) rc = launch_fold_partials(ctx, d_part, 1, d_out, false);
  }
  if (tm && rc == SNARKV_OK) SNARKV_HIP(hipEventRecord(ctx->ev[SNARKV_PIP_STAGES - 1], ctx->stream));
  return rc;
}

// ---- many MSMs in one call --------------------------------------------------------------------------------------
// Several MSMs kept in flight on their own streams time-share the GPU kernel by kernel: a resident k_accumulate owns
// nearly every VGPR (3 waves x 168 registers per SIMD), so the kernels of the other MSMs (prepare, the sorts, the
// tails) wait for wave slots 5-20x longer than they run alone (rocprofv3 trace of 4 in flight at 2^20: k_prepare
// 0.1 -> 2 ms), and every stream's next MSM waits for its own tail.  A batch knows all its MSMs up front:
//   * every prepare + sort goes to two HIGH-PRIORITY streams (memory-bound kernels: they take the wave slots first as
//     accumulation wavefronts retire, and give the VALU back while they wait for memory);
//   * the accumulations (+ combine) run on three normal-priority streams, each waiting only for its own sort -- the
//     next accumulation's wavefronts fill the slots the previous one drains;
//   * ONE tail per round for all jobs (their bucket grids lie end to end): three launches, and no stream waits for it.
// Measured (MI355X, 2^20 points each): 8 / 20 MSMs 1.67 / 1.53 ms per MSM against 1.74 / 1.60 with four single calls
// in flight; level from 40 on (the machine is issue-bound on the total work either way).  Strict
// phase order (all sorts, then all accumulations) measured 6 % slower than this pipeline, tails in groups of 2-10 under
// the later accumulations level, an occupancy cap on k_accumulate (LDS allocation) 3-9 % slower.
// Job j's scratch is a private context (ctx->jobs[j]); results are the bytes of the single-MSM entry point.
// (Measured and removed, round 3: the batch captured and replayed as ONE hipGraph -- 1.2 % slower than this eager
// enqueue, whose host side runs 1.5 ms ahead of a 30 ms batch anyway: profiles/r03_ab_scheduling.txt, git tag exp/many-graph.)
int launch_msm_pippenger_many(snarkv_ctx* ctx, size_t count, const void* const* d_s, const void* const* d_p,
                              const size_t* n, int window_bits, void* d_out, bool partial_out, hipEvent_t* ready) {
  const size_t ostride = partial_out ? SNARKV_G1_PARTIAL_BYTES : 64;
  ctx->last_many_jobs = 0;
  ctx->last_split_workers = 0;
  if (count == 0) return SNARKV_OK;
  uint32_t c0 = 0, w0 = 0, b0 = 0;
  bool uniform = true, large = false;
  size_t nmax = 0, sig = count * 1000003u + (size_t)(uint32_t)window_bits;
  for (size_t i = 0; i < count; ++i) {
    if (n[i] == 0) return SNARKV_ERR_EMPTY;
    uint32_t c, w, b;
    SNARKV_TRY(pip_geometry(n[i], window_bits, &c, &w, &b));
    if (i == 0) c0 = c, w0 = w, b0 = b;
    uniform = uniform && c == c0;
    large = large || pip_chunk_pipeline(n[i], window_bits, false, nullptr);  // the same rule as the single call
    nmax = std::max(nmax, n[i]);
    sig = sig * 31 + n[i];
  }
  const char* em = getenv("SNARKV_MANY_MODE");  // 0: one MSM after the other through the single-call path (A/B knob)
  if (count == 1 || large || (em && atoi(em) == 0) || ctx->is_lane) {
    for (size_t i = 0; i < count; ++i) {
      if (ready) SNARKV_HIP(hipStreamWaitEvent(ctx->stream, ready[i], 0));
      SNARKV_TRY(launch_msm_pippenger_auto(ctx, d_s[i], d_p[i], n[i], window_bits, (uint8_t*)d_out + ostride * i, partial_out));
    }
    return SNARKV_OK;
  }
  // jobs per round: bounded by the scratch footprint (~560 B per point + two bucket grids)
  const size_t per_job = nmax * 600 + (size_t)w0 * b0 * SNARKV_G1_PARTIAL_BYTES * 2 + (1u << 20);
  size_t G = std::min<size_t>(count, SNARKV_MANY_MAX_JOBS);
  G = std::max<size_t>(1, std::min<size_t>(G, ((size_t)48 << 30) / per_job));
  if (const char* eg = getenv("SNARKV_MANY_JOBS")) G = std::max<size_t>(1, std::min<size_t>(G, (size_t)atoi(eg)));
  const size_t rounds = (count + G - 1) / G;
  G = (count + rounds - 1) / rounds;  // even rounds
  SNARKV_TRY(ctx_lanes(ctx));
  while ((size_t)ctx->njobs < G) {
    snarkv_ctx* j = nullptr;
    // a job context is scratch + events only (its phases are enqueued on the scheduler's streams): it borrows this
    // context's stream handle instead of creating a stream of its own -- the runtime maps streams onto its hardware
    // queues in creation order, and dozens of idle streams would shift the mapping of every stream created after them
    SNARKV_TRY(SNARKV_API(ctx_create)(ctx->device, (void*)ctx->stream, &j));
    j->is_lane = true;
    j->throughput_mode = true;  // long runs: other accumulations are always resident next to a job's
    SNARKV_HIP(hipEventCreateWithFlags(&j->sorted_ev, hipEventDisableTiming));  // the job's sort is done (its accumulation waits for it)
    j->sorted_ev_ready = true;
    ctx->jobs[ctx->njobs++] = j;
  }
  if (!ctx->hi_ready) {
    int least = 0, greatest = 0;
    SNARKV_HIP(hipDeviceGetStreamPriorityRange(&least, &greatest));
    for (int i = 0; i < 2; ++i) SNARKV_HIP(hipStreamCreateWithPriority(&ctx->hi_stream[i], hipStreamNonBlocking, greatest));
    for (int i = 0; i < 2; ++i) SNARKV_HIP(hipEventCreateWithFlags(&ctx->many_ev[i], hipEventDisableTiming));
    ctx->hi_ready = true;
  }
  const bool tm = ctx->stage_timing;
  if (tm && !ctx->ev_ready) {
    for (int i = 0; i <= SNARKV_PIP_STAGES; ++i) SNARKV_HIP(hipEventCreate(&ctx->ev[i]));
    ctx->ev_ready = true;
  }
  if (sig != ctx->many_sig) {  // a new shape may grow (free + reallocate) scratch that queued work still uses
    SNARKV_HIP(hipDeviceSynchronize());
    ctx->many_sig = sig;
  }
  hipStream_t S[3] = {ctx->stream, ctx->sub[0]->stream, ctx->sub[1]->stream};  // the accumulation streams
  constexpr int nS = 3;  // three of them: 2 / 4 measured level or worse (profiles/r02_sweep_many.txt)
  // the context's stream waits for everything queued on the other four streams (join), then they wait for it (fork)
  auto join_and_fork = [&]() -> int {
    for (int k = 0; k < 2; ++k) {
      SNARKV_HIP(hipEventRecord(ctx->many_ev[k], ctx->hi_stream[k]));
      SNARKV_HIP(hipStreamWaitEvent(ctx->stream, ctx->many_ev[k], 0));
    }
    for (int k = 0; k + 1 < nS; ++k) {
      SNARKV_HIP(hipEventRecord(ctx->sub_ev[k], S[k + 1]));
      SNARKV_HIP(hipStreamWaitEvent(ctx->stream, ctx->sub_ev[k], 0));
    }
    SNARKV_HIP(hipEventRecord(ctx->sub_ev[4], ctx->stream));
    for (int k = 0; k < 2; ++k) SNARKV_HIP(hipStreamWaitEvent(ctx->hi_stream[k], ctx->sub_ev[4], 0));
    for (int k = 0; k + 1 < nS; ++k) SNARKV_HIP(hipStreamWaitEvent(S[k + 1], ctx->sub_ev[4], 0));
    return SNARKV_OK;
  };
  void* d_grids = nullptr;
  const size_t grid_bytes = (size_t)w0 * b0 * SNARKV_G1_PARTIAL_BYTES;
  if (uniform) SNARKV_TRY(ctx_reserve(ctx, SLOT_MGPU_GRID, grid_bytes * G, &d_grids));
  if (tm) SNARKV_HIP(hipEventRecord(ctx->ev[0], ctx->stream));
  SNARKV_TRY(join_and_fork());  // inputs may still be in flight on the caller's stream
  for (size_t lo = 0; lo < count; lo += G) {
    const size_t hi = std::min(count, lo + G);
    const bool last = hi == count;
    for (size_t i = lo; i < hi; ++i) {
      snarkv_ctx* job = ctx->jobs[i - lo];
      job->mont = ctx->mont;
      job->stage_timing = tm && last;
      void* grid = uniform ? (uint8_t*)d_grids + grid_bytes * (i - lo) : nullptr;
      hipStream_t sa = ctx->hi_stream[(i - lo) % 2], sb = S[(i - lo) % nS];
      if (ready) SNARKV_HIP(hipStreamWaitEvent(sa, ready[i], 0));
      SNARKV_TRY(launch_msm_pippenger_phases(job, sa, PIP_PHASE_SORT, d_s[i], d_p[i], n[i], window_bits, nullptr, false,
                                             nullptr, grid));
      SNARKV_HIP(hipEventRecord(job->sorted_ev, sa));
      SNARKV_HIP(hipStreamWaitEvent(sb, job->sorted_ev, 0));
      SNARKV_TRY(launch_msm_pippenger_phases(job, sb, PIP_PHASE_ACC, d_s[i], d_p[i], n[i], window_bits, nullptr, false,
                                             nullptr, grid));
      // a ragged batch (different window sizes) cannot share one tail: each job's own, behind its accumulation
      if (!uniform)
        SNARKV_TRY(launch_msm_pippenger_phases(job, sb, PIP_PHASE_TAIL, d_s[i], d_p[i], n[i], window_bits,
                                               (uint8_t*)d_out + ostride * i, partial_out, nullptr, nullptr));
      job->stage_timing = false;
    }
    SNARKV_TRY(join_and_fork());
    if (uniform) {
      SNARKV_TRY(launch_buckets_reduce_many(ctx, ctx->stream, d_grids, c0, w0, (uint32_t)(hi - lo),
                                            (uint8_t*)d_out + ostride * lo, partial_out));
      if (!last) SNARKV_TRY(join_and_fork());  // the next round overwrites the grids
    }
    if (last) ctx->last_many_jobs = (int)(hi - lo);
  }
  if (tm) SNARKV_HIP(hipEventRecord(ctx->ev[SNARKV_PIP_STAGES - 1], ctx->stream));
  return SNARKV_OK;
}

// the host-staged Pippenger; each library exports it under its own signature (capi.hip / pallas.hip)
int msm_pippenger_staged(snarkv_ctx* ctx, const uint8_t* scalars32, const uint8_t* points64, size_t n, uint32_t flags,
                         uint8_t out64[64]) {
  if (!ctx || !scalars32 || !points64 || !out64) return SNARKV_ERR_ARG;
  if (n == 0) return SNARKV_ERR_EMPTY;  // reference panics: msm.rs:265
  SNARKV_HIP(hipSetDevice(ctx->device));
  SNARKV_CALL_FLAGS(ctx, flags & SNARKV_API_FLAGS);
  void *d_s, *d_p, *d_out;
  SNARKV_TRY(stage_in(ctx, SLOT_IN_SCALARS, scalars32, n * 32, &d_s));
  SNARKV_TRY(stage_in(ctx, SLOT_IN_POINTS, points64, n * 64, &d_p));
  SNARKV_TRY(ctx_reserve(ctx, SLOT_OUT, 64, &d_out));
  SNARKV_TRY(check_validate(ctx, d_s, d_p, n, flags));
  SNARKV_TRY(launch_msm_pippenger_auto(ctx, d_s, d_p, n, 0, d_out, false));
  return fetch_out(ctx, d_out, out64, 64);
}

}  // namespace snarkv

using namespace snarkv;

extern "C" {

// `NativeLoader::multi_scalar_multiplication` (loader/native.rs:61-71): n_msm independent MSMs in one launch
// (segment k = terms offsets[k] .. offsets[k+1])
int SNARKV_API(g1_msm_batched)(snarkv_ctx* ctx, const uint8_t* scalars32, const uint8_t* points64,
                               const uint32_t* offsets, size_t n_msm, uint32_t flags, uint8_t* out) {
  if (!ctx || !scalars32 || !points64 || !offsets || !out) return SNARKV_ERR_ARG;
  if (n_msm == 0) return SNARKV_ERR_EMPTY;
  if (offsets[0] != 0) return SNARKV_ERR_LENGTH;
  for (size_t k = 0; k < n_msm; ++k) {
    if (offsets[k + 1] < offsets[k]) return SNARKV_ERR_LENGTH;
    if (offsets[k + 1] == offsets[k]) return SNARKV_ERR_EMPTY;  // reference panics: native.rs:69
  }
  size_t n = offsets[n_msm];
  SNARKV_HIP(hipSetDevice(ctx->device));
  SNARKV_CALL_FLAGS(ctx, flags & SNARKV_API_FLAGS);
  void *d_s, *d_p, *d_o, *d_out;
  SNARKV_TRY(stage_in(ctx, SLOT_IN_SCALARS, scalars32, n * 32, &d_s));
  SNARKV_TRY(stage_in(ctx, SLOT_IN_POINTS, points64, n * 64, &d_p));
  SNARKV_TRY(stage_in(ctx, SLOT_IN_OFFSETS, offsets, (n_msm + 1) * 4, &d_o));
  SNARKV_TRY(ctx_reserve(ctx, SLOT_OUT, n_msm * 64, &d_out));
  SNARKV_TRY(check_validate(ctx, d_s, d_p, n, flags));
  SNARKV_TRY(launch_msm_batched(ctx, d_s, d_p, d_o, n_msm, n, d_out));
  return fetch_out(ctx, d_out, out, n_msm * 64);
}

int SNARKV_API(g1_msm_naive)(snarkv_ctx* ctx, const uint8_t* scalars32, const uint8_t* points64, size_t n,
                             uint32_t flags, uint8_t out64[64]) {
  if (n == 0) return SNARKV_ERR_EMPTY;
  if (n > 0xFFFFFFFFull) return SNARKV_ERR_LENGTH;
  uint32_t offsets[2] = {0, (uint32_t)n};
  return SNARKV_API(g1_msm_batched)(ctx, scalars32, points64, offsets, 1, flags, out64);
}

int SNARKV_API(g1_msm_pippenger_dev)(snarkv_ctx* ctx, const void* d_scalars32, const void* d_points64, size_t n,
                                     int window_bits, void* d_out64) {
  if (!ctx || !d_scalars32 || !d_points64 || !d_out64) return SNARKV_ERR_ARG;
  if (n == 0) return SNARKV_ERR_EMPTY;
  SNARKV_HIP(hipSetDevice(ctx->device));
  return launch_msm_pippenger_auto(ctx, d_scalars32, d_points64, n, window_bits, d_out64, false);
}

}  // extern "C"
