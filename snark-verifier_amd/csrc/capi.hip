// C ABI glue of the BN254 library (include/snarkv_amd.h): what the pasta build does not share -- flags, hints and stage
// timing, the batch and bucket-grid entry points, decompression, the decider, sampling, and the context-free bn254_*
// forms over a pool of default contexts.  The context itself is ctx.hip, the MSM entry layer of both libraries
// msm_api.hip.  No arithmetic happens on the host; every entry point stages bytes to HBM, enqueues the HIP kernels and
// copies the (tiny) result back.
#include <string.h>
#include <algorithm>
#include <atomic>
#include <condition_variable>
#include <memory>
#include <mutex>
#include <vector>
#include <stdlib.h>
#include "ctx.hpp"
#include "../../include/snarkv_ipa_batch.h"
#include "../../include/snarkv_ipa_fold.h"
#include "../../include/snarkv_ipa_create.h"
#include "../../include/snarkv_ipa_multiopen.h"

namespace snarkv {

// ---- the context-free entry points' contexts ------------------------------------------------------------------------
// `EcPointLoader::multi_scalar_multiplication` has no `&self` (loader.rs:108), so a trait-bound Rust caller can only reach
// the `bn254_*` forms -- and round 4 gave them ONE context behind one mutex: a rayon-parallel caller got one job at a
// time, a sixteenth of what sixteen explicit contexts deliver.  Now they draw from a POOL of default
// contexts (a stream + scratch each), checked out per call:
//   * size: SNARKV_DEFAULT_CONTEXTS, else 4 (the runtime's default hardware-queue count); contexts are created on
//     demand, never destroyed;
//   * affinity: a thread comes back to the context it used last when that one is free (warm scratch), else any free
//     one, else a new one while the pool may grow, else it waits;
//   * nesting: bn254_kzg_decide -> bn254_kzg_decide_batch runs on the context the outer call holds;
//   * flags: the process default (bn254_set_flags) or the calling thread's override (bn254_set_thread_flags) is applied
//     to the context at check-out, and so is the throughput hint (on while eight or more contexts are checked out);
//   * pinned host buffers (bn254_host_buffer) belong to the calling THREAD, not to a context: what a thread packs is
//     its own until it asks again, whatever context its next call lands on.
struct DefaultPool {
  std::mutex mu;
  std::condition_variable cv;
  std::vector<snarkv_ctx*> ctx;
  std::vector<char> busy;
  int cap = 0;
  std::atomic<uint32_t> flags{0};
};
static DefaultPool g_pool;
static thread_local int tl_slot = -1, tl_depth = 0;
static thread_local snarkv_ctx* tl_held = nullptr;
static thread_local int64_t tl_flags = -1;  // -1: the process default

static int pool_cap() {
  if (const char* e = getenv("SNARKV_DEFAULT_CONTEXTS")) {
    int v = atoi(e);
    if (v > 0) return std::min(v, 64);
  }
  return 4;
}

struct DefaultLease {
  snarkv_ctx* c = nullptr;
  int rc = SNARKV_OK;
  DefaultLease() {
    if (tl_depth > 0) {  // nested context-free call: the context the outer call holds
      c = tl_held;
      ++tl_depth;
      return;
    }
    std::unique_lock<std::mutex> lk(g_pool.mu);
    if (g_pool.cap == 0) g_pool.cap = pool_cap();
    int slot = -1;
    for (;;) {
      if (tl_slot >= 0 && tl_slot < (int)g_pool.ctx.size() && !g_pool.busy[tl_slot]) slot = tl_slot;
      for (int i = 0; slot < 0 && i < (int)g_pool.ctx.size(); ++i)
        if (!g_pool.busy[i]) slot = i;
      if (slot >= 0) break;
      if ((int)g_pool.ctx.size() < g_pool.cap) {
        snarkv_ctx* fresh = nullptr;
        rc = snarkv_ctx_create(0, nullptr, &fresh);  // (under the pool lock: at most `cap` times per process)
        if (rc < 0) return;
        g_pool.ctx.push_back(fresh);
        g_pool.busy.push_back(0);
        slot = (int)g_pool.ctx.size() - 1;
        break;
      }
      g_pool.cv.wait(lk);
    }
    g_pool.busy[slot] = 1;
    c = g_pool.ctx[slot];
    int in_use = 0;
    for (char b : g_pool.busy) in_use += b ? 1 : 0;
    lk.unlock();
    // the throughput hint, by what the pool sees: with eight or more calls in flight the GPU is shared and the forms that
    // do less work on a longer chain pay (1 024-proof jobs: 0.83 -> 0.75 ms per job at 8 in flight, 0.70 -> 0.49 at 16);
    // below that they lose (1.35 -> 2.06 at 2, 1.04 -> 1.22 at 4: tools/aggregate_inflight.py --hint-from)
    c->throughput_mode = in_use >= 8;
    c->throughput_peers = in_use;  // the pool KNOWS how many calls share the GPU (not a fixed sixteenth)
    tl_slot = slot;
    tl_held = c;
    tl_depth = 1;
    const uint32_t f = tl_flags >= 0 ? (uint32_t)tl_flags : g_pool.flags.load();
    c->flags = f;
    c->mont = (f & SNARKV_FLAG_MONTGOMERY) != 0;
  }
  ~DefaultLease() {
    if (!c) return;
    if (--tl_depth > 0) return;
    tl_held = nullptr;
    {
      std::lock_guard<std::mutex> lk(g_pool.mu);
      g_pool.busy[tl_slot] = 0;
    }
    g_pool.cv.notify_one();
  }
};
#define SNARKV_DEFAULT_LEASE(c)   \
  DefaultLease _lease;            \
  if (_lease.rc < 0) return _lease.rc; \
  snarkv_ctx* c = _lease.c

// pinned host buffers of the context-free callers, one set per THREAD (slots reused when a thread ends; the memory is
// never returned: like the contexts, it lives as long as the process)
struct ThreadHostBufs {
  void* buf[SNARKV_HOST_BUFFERS] = {};
  size_t cap[SNARKV_HOST_BUFFERS] = {};
};
static std::mutex g_hb_mu;
static std::vector<ThreadHostBufs*> g_hb_free;
struct ThreadHostBufsRef {
  ThreadHostBufs* p = nullptr;
  ~ThreadHostBufsRef() {
    if (!p) return;
    std::lock_guard<std::mutex> lk(g_hb_mu);
    g_hb_free.push_back(p);  // no HIP call at thread exit: the set goes to the next thread that asks
  }
};
static thread_local ThreadHostBufsRef tl_hb;

// line tables of the last DK_CACHE deciding keys of bn254_kzg_decide[_batch] (file scope: bn254_shutdown releases them)
enum { DK_CACHE = 4 };
struct DkCacheEntry {
  std::shared_ptr<snarkv_dk> dk;
  uint8_t tag[321];
  uint64_t used;
};
static std::mutex g_dk_cache_mu;
static DkCacheEntry g_dk_cache[DK_CACHE];
static uint64_t g_dk_tick = 0;

}  // namespace snarkv

using namespace snarkv;

extern "C" {

int snarkv_set_stage_timing(snarkv_ctx* ctx, int enabled) {
  if (!ctx) return SNARKV_ERR_ARG;
  ctx->stage_timing = enabled != 0;
  return SNARKV_OK;
}

int snarkv_ctx_set_flags(snarkv_ctx* ctx, uint32_t flags) {
  if (!ctx || (flags & ~(SNARKV_FLAG_VALIDATE | SNARKV_FLAG_MONTGOMERY))) return SNARKV_ERR_ARG;
  ctx->flags = flags;
  ctx->mont = (flags & SNARKV_FLAG_MONTGOMERY) != 0;
  return SNARKV_OK;
}

uint32_t snarkv_ctx_get_flags(const snarkv_ctx* ctx) { return ctx ? ctx->flags : 0u; }

int snarkv_ctx_set_throughput_hint(snarkv_ctx* ctx, int enabled) {
  if (!ctx) return SNARKV_ERR_ARG;
  ctx->throughput_mode = enabled != 0;
  ctx->throughput_peers = enabled > 1 ? enabled : 0;  // n >= 2: that many contexts in flight; 1: unknown (16 assumed)
  return SNARKV_OK;
}

int snarkv_g1_msm_launch_points_ex(size_t n, int window_bits, size_t* per_launch) {
  if (!per_launch) return SNARKV_ERR_ARG;
  size_t chunk = 0;
  *per_launch = snarkv::pip_chunk_pipeline(n, window_bits, false, &chunk) ? chunk : n;
  return SNARKV_OK;
}

int snarkv_g1_msm_launch_points(size_t n, size_t* per_launch) { return snarkv_g1_msm_launch_points_ex(n, 0, per_launch); }

int snarkv_get_stage_timing(snarkv_ctx* ctx, float ms[SNARKV_PIP_STAGES]) {
  if (!ctx || !ctx->ev_ready) return SNARKV_ERR_ARG;
  SNARKV_HIP(hipStreamSynchronize(ctx->stream));
  if (ctx->last_many_jobs > 0) {
    // batch (snarkv_g1_msm_pippenger_many_dev): [0] the whole call; [4] / [5] ONE k_accumulate / combine launch of its
    // last round, averaged over the jobs' own events (launches of up to three jobs overlap); the rest is not broken down
    for (int i = 0; i < SNARKV_PIP_STAGES; ++i) ms[i] = 0.f;
    SNARKV_HIP(hipEventElapsedTime(&ms[0], ctx->ev[0], ctx->ev[SNARKV_PIP_STAGES - 1]));
    const float jobs = (float)ctx->last_many_jobs;
    for (int j = 0; j < ctx->last_many_jobs; ++j) {
      snarkv_ctx* job = ctx->jobs[j];
      if (!job->ev_ready) continue;
      float t = 0.f;
      SNARKV_HIP(hipEventElapsedTime(&t, job->ev[3], job->ev[4]));
      ms[4] += t / jobs;
      SNARKV_HIP(hipEventElapsedTime(&t, job->ev[4], job->ev[5]));
      ms[5] += t / jobs;
    }
    return SNARKV_OK;
  }
  if (ctx->last_split_workers > 0) {
    // chunk pipeline: total = the whole MSM on this stream; stages 1..5 = ONE 2^20-point chunk (the last one of every
    // worker lane, averaged): what a single launch of each kernel took; the shared tail is not broken down
    SNARKV_HIP(hipEventElapsedTime(&ms[0], ctx->ev[0], ctx->ev[SNARKV_PIP_STAGES - 1]));
    for (int i = 1; i < SNARKV_PIP_STAGES; ++i) ms[i] = 0.f;
    int used = 0;
    for (int w = 0; w < ctx->last_split_workers; ++w) {
      snarkv_ctx* lane = ctx->sub[w];
      if (!lane || !lane->ev_ready) continue;
      SNARKV_HIP(hipStreamSynchronize(lane->stream));
      for (int i = 1; i <= 5; ++i) {
        float t = 0.f;
        SNARKV_HIP(hipEventElapsedTime(&t, lane->ev[i - 1], lane->ev[i]));
        ms[i] += t;
      }
      ++used;
    }
    for (int i = 1; i <= 5 && used; ++i) ms[i] /= (float)used;
    return SNARKV_OK;
  }
  SNARKV_HIP(hipEventElapsedTime(&ms[0], ctx->ev[0], ctx->ev[SNARKV_PIP_STAGES - 1]));
  for (int i = 1; i < SNARKV_PIP_STAGES; ++i) SNARKV_HIP(hipEventElapsedTime(&ms[i], ctx->ev[i - 1], ctx->ev[i]));
  return SNARKV_OK;
}

int snarkv_g1_decompress(snarkv_ctx* ctx, const uint8_t* in32, size_t n, uint8_t* out64, uint8_t* ok) {
  if (!ctx || (n && (!in32 || !out64 || !ok))) return SNARKV_ERR_ARG;
  if (n == 0) return SNARKV_OK;
  if (n > 0xFFFFFFFFull) return SNARKV_ERR_LENGTH;
  SNARKV_HIP(hipSetDevice(ctx->device));
  void *d_in, *d_out;
  SNARKV_TRY(stage_in(ctx, SLOT_IN_POINTS, in32, n * 32, &d_in));
  SNARKV_TRY(ctx_reserve(ctx, SLOT_OUT, n * 64 + n, &d_out));  // the points, then one validity byte each
  SNARKV_TRY(launch_g1_decompress(ctx, d_in, n, d_out, (uint8_t*)d_out + n * 64));
  SNARKV_HIP(hipMemcpyAsync(ok, (const uint8_t*)d_out + n * 64, n, hipMemcpyDeviceToHost, ctx->stream));
  return fetch_out(ctx, d_out, out64, n * 64);
}

int snarkv_g1_msm_batched_dev(snarkv_ctx* ctx, const void* d_scalars32, const void* d_points64,
                              const void* d_offsets, size_t n_msm, size_t n_terms, void* d_out) {
  if (!ctx || !d_scalars32 || !d_points64 || !d_offsets || !d_out) return SNARKV_ERR_ARG;
  if (n_msm == 0 || n_terms == 0) return SNARKV_ERR_EMPTY;
  SNARKV_HIP(hipSetDevice(ctx->device));
  return launch_msm_batched(ctx, d_scalars32, d_points64, d_offsets, n_msm, n_terms, d_out);
}

int snarkv_g1_msm_pippenger_many_dev(snarkv_ctx* ctx, size_t count, const void* const* d_scalars32,
                                     const void* const* d_points64, const size_t* n, int window_bits, void* d_out64s) {
  if (!ctx || (count && (!d_scalars32 || !d_points64 || !n || !d_out64s))) return SNARKV_ERR_ARG;
  for (size_t i = 0; i < count; ++i)
    if (!d_scalars32[i] || !d_points64[i]) return SNARKV_ERR_ARG;
  SNARKV_HIP(hipSetDevice(ctx->device));
  return launch_msm_pippenger_many(ctx, count, d_scalars32, d_points64, n, window_bits, d_out64s, false);
}

int snarkv_g1_msm_pippenger_many_partial_dev(snarkv_ctx* ctx, size_t count, const void* const* d_scalars32,
                                             const void* const* d_points64, const size_t* n, int window_bits,
                                             void* d_partials) {
  if (!ctx || (count && (!d_scalars32 || !d_points64 || !n || !d_partials))) return SNARKV_ERR_ARG;
  for (size_t i = 0; i < count; ++i)
    if (!d_scalars32[i] || !d_points64[i]) return SNARKV_ERR_ARG;
  SNARKV_HIP(hipSetDevice(ctx->device));
  return launch_msm_pippenger_many(ctx, count, d_scalars32, d_points64, n, window_bits, d_partials, true);
}

// HOST-resident batch: job i's scalars / points are uploaded on a copy stream of their own, one event per job, and the
// batch scheduler makes a job's first kernel wait for ITS event only -- the uploads of jobs i + 1 .. run under the
// kernels of jobs .. i.  A 2^20-point job is 96 MiB: ~1.8 ms over PCIe Gen5 x16 against ~1.5 ms of kernels, so a batch
// runs at the link's rate (bench.py `host_resident`).  Pinned sources (snarkv_ctx_host_buffer, snarkv_host_register) are
// DMA reads; pageable ones go through the runtime's bounce buffer at about a third of the rate.
int snarkv_g1_msm_pippenger_many(snarkv_ctx* ctx, size_t count, const uint8_t* const* scalars32,
                                 const uint8_t* const* points64, const size_t* n, uint32_t flags, uint8_t* out64s) {
  if (!ctx || (count && (!scalars32 || !points64 || !n || !out64s))) return SNARKV_ERR_ARG;
  if (count == 0) return SNARKV_OK;
  size_t total = 0;
  for (size_t i = 0; i < count; ++i) {
    if (!scalars32[i] || !points64[i]) return SNARKV_ERR_ARG;
    if (n[i] == 0) return SNARKV_ERR_EMPTY;
    total += n[i];
  }
  SNARKV_HIP(hipSetDevice(ctx->device));
  SNARKV_CALL_FLAGS(ctx, flags);
  // staging for as many jobs at a time as fit 12 GiB (a 2^20-point job is 96 MiB); more run as successive sub-batches
  const size_t kStageCap = (size_t)12 << 30;
  if (!ctx->copy_ready) {
    SNARKV_HIP(hipStreamCreateWithFlags(&ctx->copy_stream, hipStreamNonBlocking));
    ctx->copy_ready = true;
  }
  std::vector<hipEvent_t> evs(count, nullptr);
  auto drop_events = [&]() {
    for (auto e : evs)
      if (e) (void)hipEventDestroy(e);
  };
  int rc = SNARKV_OK;
  for (size_t lo = 0; lo < count && rc == SNARKV_OK;) {
    size_t hi = lo, pts = 0;
    while (hi < count && (hi == lo || (pts + n[hi]) * 96 <= kStageCap)) pts += n[hi++];
    void *d_s = nullptr, *d_p = nullptr, *d_out = nullptr;
    rc = ctx_reserve(ctx, SLOT_IN_SCALARS, pts * 32, &d_s);
    if (rc == SNARKV_OK) rc = ctx_reserve(ctx, SLOT_IN_POINTS, pts * 64, &d_p);
    if (rc == SNARKV_OK) rc = ctx_reserve(ctx, SLOT_OUT, (hi - lo) * 64, &d_out);
    if (rc != SNARKV_OK) break;
    std::vector<const void*> ps(hi - lo), pp(hi - lo);
    // the staging buffers may still be read by work queued on the context's stream: the uploads start behind it
    hipEvent_t& fence = evs[lo];  // (re-recorded below as job lo's own event)
    if (!fence && hipEventCreateWithFlags(&fence, hipEventDisableTiming) != hipSuccess) { rc = SNARKV_ERR_DEVICE; break; }
    (void)hipEventRecord(fence, ctx->stream);
    (void)hipStreamWaitEvent(ctx->copy_stream, fence, 0);
    size_t off = 0;
    for (size_t i = lo; i < hi && rc == SNARKV_OK; ++i) {
      ps[i - lo] = (const uint8_t*)d_s + 32 * off;
      pp[i - lo] = (const uint8_t*)d_p + 64 * off;
      if (hipMemcpyAsync((void*)ps[i - lo], scalars32[i], n[i] * 32, hipMemcpyHostToDevice, ctx->copy_stream) != hipSuccess ||
          hipMemcpyAsync((void*)pp[i - lo], points64[i], n[i] * 64, hipMemcpyHostToDevice, ctx->copy_stream) != hipSuccess ||
          (!evs[i] && hipEventCreateWithFlags(&evs[i], hipEventDisableTiming) != hipSuccess) ||
          hipEventRecord(evs[i], ctx->copy_stream) != hipSuccess) {
        set_last_error("host-resident batch: upload of job %zu failed: %s", i, hipGetErrorString(hipGetLastError()));
        rc = SNARKV_ERR_DEVICE;
      }
      off += n[i];
    }
    if (rc != SNARKV_OK) break;
    if ((flags | ctx->flags) & SNARKV_FLAG_VALIDATE) {  // validation reads everything: no overlap on this path
      (void)hipStreamSynchronize(ctx->copy_stream);
      rc = check_validate(ctx, d_s, d_p, pts, flags);
      if (rc != SNARKV_OK) break;
    }
    rc = launch_msm_pippenger_many(ctx, hi - lo, ps.data(), pp.data(), n + lo, 0, d_out, false, evs.data() + lo);
    if (rc == SNARKV_OK) rc = fetch_out(ctx, d_out, out64s + 64 * lo, (hi - lo) * 64);
    lo = hi;
  }
  if (rc != SNARKV_OK) {
    (void)hipStreamSynchronize(ctx->copy_stream);
    (void)hipStreamSynchronize(ctx->stream);
  }
  drop_events();
  return rc;
}

// hipHostRegister / hipHostUnregister for callers without a HIP binding: pins `bytes` at `p` (e.g. a Vec<G1Affine>'s
// buffer) so that the uploads above are DMA reads straight out of it
int snarkv_host_register(void* p, size_t bytes) {
  if (!p || !bytes) return SNARKV_ERR_ARG;
  SNARKV_HIP(hipHostRegister(p, bytes, hipHostRegisterDefault));
  return SNARKV_OK;
}
int snarkv_host_unregister(void* p) {
  if (!p) return SNARKV_ERR_ARG;
  SNARKV_HIP(hipHostUnregister(p));
  return SNARKV_OK;
}

int snarkv_g1_msm_pippenger(snarkv_ctx* ctx, const uint8_t* scalars32, const uint8_t* points64, size_t n,
                            uint32_t flags, uint8_t out64[64]) {
  return msm_pippenger_staged(ctx, scalars32, points64, n, flags, out64);
}

int snarkv_g1_msm_pippenger_partial_dev(snarkv_ctx* ctx, const void* d_scalars32, const void* d_points64,
                                        size_t n, int window_bits, void* d_partial) {
  if (!ctx || !d_scalars32 || !d_points64 || !d_partial) return SNARKV_ERR_ARG;
  if (n == 0) return SNARKV_ERR_EMPTY;
  SNARKV_HIP(hipSetDevice(ctx->device));
  return launch_msm_pippenger_auto(ctx, d_scalars32, d_points64, n, window_bits, d_partial, true);
}

int snarkv_g1_fold_partials_dev(snarkv_ctx* ctx, const void* d_partials, size_t count, void* d_out64) {
  if (!ctx || !d_partials || !d_out64) return SNARKV_ERR_ARG;
  if (count == 0) return SNARKV_ERR_EMPTY;
  SNARKV_HIP(hipSetDevice(ctx->device));
  return launch_fold_partials(ctx, d_partials, count, d_out64);
}

int snarkv_g1_fold_partials_many_dev(snarkv_ctx* ctx, const void* d_partials, size_t count, size_t jobs, void* d_out64s) {
  if (!ctx || !d_partials || !d_out64s) return SNARKV_ERR_ARG;
  if (count == 0 || jobs == 0) return SNARKV_ERR_EMPTY;
  SNARKV_HIP(hipSetDevice(ctx->device));
  return launch_fold_partials_many(ctx, d_partials, count, jobs, d_out64s);
}

int snarkv_g1_msm_bucket_geometry(size_t n_total, int window_bits, uint32_t* c, uint32_t* windows,
                                  uint32_t* buckets_per_window) {
  if (!c || !windows || !buckets_per_window) return SNARKV_ERR_ARG;
  if (n_total == 0) return SNARKV_ERR_EMPTY;
  return pip_geometry(n_total, window_bits, c, windows, buckets_per_window);
}

int snarkv_g1_msm_fill_buckets_dev(snarkv_ctx* ctx, const void* d_scalars32, const void* d_points64, size_t n,
                                   int window_bits, void* d_buckets) {
  if (!ctx || !d_scalars32 || !d_points64 || !d_buckets || window_bits < 2 || window_bits > 22) return SNARKV_ERR_ARG;
  if (n == 0) return SNARKV_ERR_EMPTY;
  SNARKV_HIP(hipSetDevice(ctx->device));
  return launch_msm_pippenger(ctx, d_scalars32, d_points64, n, window_bits, nullptr, false, d_buckets);
}

int snarkv_g1_buckets_add_dev(snarkv_ctx* ctx, void* d_dst, const void* d_src, size_t count) {
  if (!ctx || !d_dst || !d_src) return SNARKV_ERR_ARG;
  if (count == 0) return SNARKV_ERR_EMPTY;
  if (count >= ((size_t)1 << 31)) return SNARKV_ERR_LENGTH;
  SNARKV_HIP(hipSetDevice(ctx->device));
  return launch_buckets_add(ctx, d_dst, d_src, count);
}

int snarkv_g1_buckets_reduce_dev(snarkv_ctx* ctx, const void* d_buckets, uint32_t c, uint32_t w0, uint32_t wcount,
                                 void* d_partial) {
  if (!ctx || !d_buckets || !d_partial || c < 2 || c > 22) return SNARKV_ERR_ARG;
  if (wcount == 0) return SNARKV_ERR_EMPTY;
  uint32_t cc, windows, bpw;
  SNARKV_TRY(pip_geometry(1, (int)c, &cc, &windows, &bpw));
  if ((uint64_t)w0 + wcount > windows) return SNARKV_ERR_LENGTH;
  SNARKV_HIP(hipSetDevice(ctx->device));
  return launch_buckets_reduce(ctx, d_buckets, c, w0, wcount, d_partial);
}

int snarkv_dk_create(snarkv_ctx* ctx, const uint8_t g1_64[64], const uint8_t g2_128[128],
                     const uint8_t s_g2_128[128], uint32_t flags, snarkv_dk** out) {
  if (!ctx || !g1_64 || !g2_128 || !s_g2_128 || !out) return SNARKV_ERR_ARG;
  SNARKV_HIP(hipSetDevice(ctx->device));
  SNARKV_CALL_FLAGS(ctx, flags);
  flags |= ctx->flags;
  uint8_t both[256];
  memcpy(both, g2_128, 128);
  memcpy(both + 128, s_g2_128, 128);
  void* d_in;
  SNARKV_TRY(stage_in(ctx, SLOT_IN_POINTS, both, 256, &d_in));
  // staging source is a stack buffer: finish the copy before returning
  SNARKV_HIP(hipStreamSynchronize(ctx->stream));
  if (flags & SNARKV_FLAG_VALIDATE) {
    int bad = 0;
    SNARKV_TRY(launch_validate_g2(ctx, d_in, &bad));
    if (bad) {
      set_last_error("deciding key: G2 point non-canonical or off the twist");
      return SNARKV_ERR_ENCODING;
    }
    void* d_g1;
    SNARKV_TRY(stage_in(ctx, SLOT_IN_SCALARS, g1_64, 64, &d_g1));
    SNARKV_TRY(launch_validate(ctx, nullptr, d_g1, 1, &bad));
    if (bad) {
      set_last_error("deciding key: G1 generator non-canonical or off-curve");
      return SNARKV_ERR_ENCODING;
    }
  }
  snarkv_dk* dk = new snarkv_dk();
  dk->device = ctx->device;
  memcpy(dk->g1, g1_64, 64);
  hipError_t e = hipMalloc(&dk->d_prep, 2 * g2_prepared_bytes());
  if (e != hipSuccess) {
    set_last_error("hipMalloc(dk): %s", hipGetErrorString(e));
    delete dk;
    return SNARKV_ERR_DEVICE;
  }
  int rc = launch_g2_prepare(ctx, d_in, dk->d_prep);
  if (rc == SNARKV_OK) {
    hipError_t e2 = hipStreamSynchronize(ctx->stream);
    if (e2 != hipSuccess) {
      set_last_error("g2_prepare: %s", hipGetErrorString(e2));
      rc = SNARKV_ERR_DEVICE;
    }
  }
  if (rc < 0) {
    (void)hipFree(dk->d_prep);
    delete dk;
    return rc;
  }
  *out = dk;
  return SNARKV_OK;
}

void snarkv_dk_destroy(snarkv_dk* dk) {
  if (!dk) return;
  (void)hipSetDevice(dk->device);
  if (dk->d_prep) (void)hipFree(dk->d_prep);
  delete dk;
}

int snarkv_kzg_decide_batch_dev(snarkv_ctx* ctx, const snarkv_dk* dk, const void* d_accs128, size_t m,
                                void* d_ok) {
  if (!ctx || !dk || !d_accs128 || !d_ok) return SNARKV_ERR_ARG;
  if (m == 0) return SNARKV_ERR_EMPTY;
  SNARKV_HIP(hipSetDevice(ctx->device));
  return launch_decide(ctx, dk->d_prep, d_accs128, m, d_ok, nullptr);
}

int snarkv_kzg_decide_batch(snarkv_ctx* ctx, const snarkv_dk* dk, const uint8_t* accs128, size_t m,
                            uint32_t flags, uint8_t* ok) {
  if (!ctx || !dk || !accs128 || !ok) return SNARKV_ERR_ARG;
  if (m == 0) return 1;  // decide_all over an empty list is Ok(()) (decider.rs:84-93)
  SNARKV_HIP(hipSetDevice(ctx->device));
  SNARKV_CALL_FLAGS(ctx, flags);
  flags |= ctx->flags;
  void *d_a, *d_ok;
  SNARKV_TRY(stage_in(ctx, SLOT_IN_POINTS, accs128, m * 128, &d_a));
  SNARKV_TRY(ctx_reserve(ctx, SLOT_OUT, m, &d_ok));
  if (flags & SNARKV_FLAG_VALIDATE) {
    int bad = 0;
    SNARKV_TRY(launch_validate(ctx, nullptr, d_a, 2 * m, &bad));
    if (bad) {
      set_last_error("%d accumulator points non-canonical or off-curve", bad);
      return SNARKV_ERR_ENCODING;
    }
  }
  SNARKV_TRY(launch_decide(ctx, dk->d_prep, d_a, m, d_ok, nullptr));
  SNARKV_TRY(fetch_out(ctx, d_ok, ok, m));
  int all = 1;
  for (size_t i = 0; i < m; ++i) all &= ok[i] ? 1 : 0;
  return all;
}

int snarkv_kzg_decide(snarkv_ctx* ctx, const snarkv_dk* dk, const uint8_t acc128[128], uint32_t flags) {
  uint8_t ok = 0;
  int rc = snarkv_kzg_decide_batch(ctx, dk, acc128, 1, flags, &ok);
  if (rc < 0) return rc;
  return ok ? 1 : 0;
}

int snarkv_kzg_pairing_value(snarkv_ctx* ctx, const snarkv_dk* dk, const uint8_t acc128[128], uint8_t gt384[384]) {
  if (!ctx || !dk || !acc128 || !gt384) return SNARKV_ERR_ARG;
  SNARKV_HIP(hipSetDevice(ctx->device));
  void *d_a, *d_gt;
  SNARKV_TRY(stage_in(ctx, SLOT_IN_POINTS, acc128, 128, &d_a));
  SNARKV_TRY(ctx_reserve(ctx, SLOT_OUT, 384, &d_gt));
  SNARKV_TRY(launch_decide(ctx, dk->d_prep, d_a, 1, nullptr, d_gt));
  return fetch_out(ctx, d_gt, gt384, 384);
}

int snarkv_sample_scalars_dev(snarkv_ctx* ctx, uint64_t seed, uint64_t first, size_t n, void* d_scalars32) {
  if (!ctx || !d_scalars32) return SNARKV_ERR_ARG;
  if (n == 0) return SNARKV_OK;
  SNARKV_HIP(hipSetDevice(ctx->device));
  return launch_sample_scalars(ctx, seed, first, n, d_scalars32);
}

int snarkv_sample_points_dev(snarkv_ctx* ctx, uint64_t seed, uint64_t first, size_t n, void* d_points64) {
  if (!ctx || !d_points64) return SNARKV_ERR_ARG;
  if (n == 0) return SNARKV_OK;
  SNARKV_HIP(hipSetDevice(ctx->device));
  return launch_sample_points(ctx, seed, first, n, d_points64);
}

int snarkv_ubench_valu(snarkv_ctx* ctx, int which, int iters, double* ops_per_s) {
  if (!ctx || !ops_per_s || iters <= 0 || which < 0 || which > 1) return SNARKV_ERR_ARG;
  SNARKV_HIP(hipSetDevice(ctx->device));
  return launch_ubench(ctx, which, iters, ops_per_s);
}

int snarkv_g1_validate(snarkv_ctx* ctx, const uint8_t* points64, size_t n) {
  if (!ctx || !points64) return SNARKV_ERR_ARG;
  if (n == 0) return SNARKV_OK;
  SNARKV_HIP(hipSetDevice(ctx->device));
  void* d_p;
  SNARKV_TRY(stage_in(ctx, SLOT_IN_POINTS, points64, n * 64, &d_p));
  int bad = 0;
  SNARKV_TRY(launch_validate(ctx, nullptr, d_p, n, &bad));
  if (bad) {
    set_last_error("%d of %zu points are non-canonical or off-curve", bad, n);
    return SNARKV_ERR_ENCODING;
  }
  return SNARKV_OK;
}

// ---- context-free entry points -------------------------------------------
int bn254_set_flags(uint32_t flags) {
  if (flags & ~(SNARKV_FLAG_VALIDATE | SNARKV_FLAG_MONTGOMERY)) return SNARKV_ERR_ARG;
  g_pool.flags.store(flags);  // applied to a pool context when a call checks it out; calls in flight keep theirs
  return SNARKV_OK;
}

uint32_t bn254_get_flags(void) { return tl_flags >= 0 ? (uint32_t)tl_flags : g_pool.flags.load(); }

int64_t bn254_set_thread_flags(int64_t flags) {
  const int64_t before = tl_flags;
  // unknown bits, or a negative value other than -1 (e.g. an error code of this very function handed back as "the
  // previous value"): refused, the override stays what it was
  if (flags < -1 || (flags >= 0 && (flags & ~(int64_t)(SNARKV_FLAG_VALIDATE | SNARKV_FLAG_MONTGOMERY)))) return SNARKV_ERR_ARG;
  tl_flags = flags;
  return before;
}

int bn254_default_contexts(int* created, int* cap) {
  std::lock_guard<std::mutex> lk(g_pool.mu);
  if (g_pool.cap == 0) g_pool.cap = pool_cap();
  if (created) *created = (int)g_pool.ctx.size();
  if (cap) *cap = g_pool.cap;
  return SNARKV_OK;
}

int bn254_g1_validate(const uint8_t* points64, size_t n) {
  SNARKV_DEFAULT_LEASE(c);
  return snarkv_g1_validate(c, points64, n);
}

int bn254_kzg_dk_create(const uint8_t g1_64[64], const uint8_t g2_128[128], const uint8_t s_g2_128[128],
                        snarkv_dk** out) {
  SNARKV_DEFAULT_LEASE(c);
  return snarkv_dk_create(c, g1_64, g2_128, s_g2_128, 0, out);
}

int bn254_kzg_dk_decide_batch(const snarkv_dk* dk, const uint8_t* accs128, size_t m, uint8_t* ok) {
  SNARKV_DEFAULT_LEASE(c);
  return snarkv_kzg_decide_batch(c, dk, accs128, m, 0, ok);
}

int bn254_g1_msm_naive(const uint8_t* scalars32, const uint8_t* points64, size_t n, uint8_t out64[64]) {
  SNARKV_DEFAULT_LEASE(c);
  return snarkv_g1_msm_naive(c, scalars32, points64, n, 0, out64);
}

int bn254_g1_msm_batched(const uint8_t* scalars32, const uint8_t* points64, const uint32_t* offsets, size_t n_msm,
                         uint8_t* out) {
  SNARKV_DEFAULT_LEASE(c);
  return snarkv_g1_msm_batched(c, scalars32, points64, offsets, n_msm, 0, out);
}

int bn254_g1_decompress(const uint8_t* in32, size_t n, uint8_t* out64, uint8_t* ok) {
  SNARKV_DEFAULT_LEASE(c);
  return snarkv_g1_decompress(c, in32, n, out64, ok);
}

int bn254_host_buffer(int slot, size_t bytes, void** out) {
  if (slot < 0 || slot >= SNARKV_HOST_BUFFERS || !out) return SNARKV_ERR_ARG;
  if (!tl_hb.p) {
    std::lock_guard<std::mutex> lk(g_hb_mu);
    if (!g_hb_free.empty()) {
      tl_hb.p = g_hb_free.back();
      g_hb_free.pop_back();
    } else {
      tl_hb.p = new ThreadHostBufs();
    }
  }
  ThreadHostBufs* hb = tl_hb.p;
  if (bytes == 0) bytes = 16;
  if (hb->cap[slot] < bytes) {
    {
      SNARKV_DEFAULT_LEASE(c);  // (a HIP device must exist; the allocation itself is not tied to a context)
      SNARKV_HIP(hipSetDevice(c->device));
    }
    const size_t old_cap = hb->cap[slot];
    if (hb->buf[slot]) SNARKV_HIP(hipHostFree(hb->buf[slot]));
    hb->buf[slot] = nullptr;
    hb->cap[slot] = 0;
    // (no copy out of the old buffer can be queued: the context-free calls return after their result is on the host)
    // geometric growth: hipHostFree / hipHostMalloc synchronise the whole device (other pool contexts are in flight), so a
    // thread whose requests creep up must not reallocate on every call
    const size_t cap = std::max(bytes + bytes / 4 + 4096, 2 * old_cap);
    SNARKV_HIP(hipHostMalloc(&hb->buf[slot], cap, hipHostMallocDefault));
    hb->cap[slot] = cap;
  }
  *out = hb->buf[slot];
  return SNARKV_OK;
}

// Everything the context-free entry points keep for the life of the process, released: the pool's contexts (streams +
// scratch), the deciding-key line tables, the pinned buffer sets of the calling thread and of threads that have ended.
// Refused (SNARKV_ERR_ARG) while any context-free call is in flight.  The next bn254_* call starts over lazily.
int bn254_shutdown(void) {
  {
    std::lock_guard<std::mutex> lk(g_pool.mu);
    if (tl_depth > 0) {
      set_last_error("bn254_shutdown: called from inside a context-free call");
      return SNARKV_ERR_ARG;
    }
    for (char b : g_pool.busy)
      if (b) {
        set_last_error("bn254_shutdown: a context-free call is in flight on another thread");
        return SNARKV_ERR_ARG;
      }
    for (snarkv_ctx* c : g_pool.ctx) snarkv_ctx_destroy(c);
    g_pool.ctx.clear();
    g_pool.busy.clear();
  }
  tl_slot = -1;
  {
    std::lock_guard<std::mutex> lk(g_dk_cache_mu);
    for (auto& e : g_dk_cache) e.dk.reset();
  }
  std::vector<ThreadHostBufs*> sets;
  {
    std::lock_guard<std::mutex> lk(g_hb_mu);
    sets.swap(g_hb_free);
  }
  if (tl_hb.p) sets.push_back(tl_hb.p), tl_hb.p = nullptr;
  for (ThreadHostBufs* hb : sets) {
    for (int i = 0; i < SNARKV_HOST_BUFFERS; ++i)
      if (hb->buf[i]) (void)hipHostFree(hb->buf[i]);
    delete hb;
  }
  (void)hipGetLastError();
  return SNARKV_OK;
}

int bn254_g1_msm_pippenger(const uint8_t* scalars32, const uint8_t* points64, size_t n, uint8_t out64[64]) {
  SNARKV_DEFAULT_LEASE(c);
  return snarkv_g1_msm_pippenger(c, scalars32, points64, n, 0, out64);
}

int bn254_kzg_decide_batch(const uint8_t g1_64[64], const uint8_t g2_128[128], const uint8_t s_g2_128[128],
                           const uint8_t* accs128, size_t m, uint8_t* ok) {
  SNARKV_DEFAULT_LEASE(c);
  if (!g1_64 || !g2_128 || !s_g2_128) return SNARKV_ERR_ARG;
  // The reference rebuilds `G2Prepared` on every decide (decider.rs:74); a verifier decides against ONE key (or a few:
  // one per recursion layer / encoding), so the line tables of the last DK_CACHE keys are kept; the 320 key bytes + the
  // encoding they were given in are the tag.  Shared by the pool's contexts (the tables are read-only device memory).
  // The lock covers the lookup and the publication only: a miss builds its tables (G2 preparation on the GPU + a
  // synchronisation) OUTSIDE it, so concurrent callers with other keys -- or the same key: the loser of the race drops
  // its copy -- never queue behind a build.  A replaced key's tables are freed when the last call using
  // them returns (shared_ptr).
  uint8_t now[321];
  memcpy(now, g1_64, 64), memcpy(now + 64, g2_128, 128), memcpy(now + 192, s_g2_128, 128);
  now[320] = c->mont ? 1 : 0;
  auto& cache_mu = g_dk_cache_mu;
  auto& cache = g_dk_cache;
  auto& tick = g_dk_tick;
  auto lookup = [&]() -> std::shared_ptr<snarkv_dk> {  // (under cache_mu)
    for (auto& e : cache)
      if (e.dk && memcmp(e.tag, now, sizeof now) == 0) {
        e.used = ++tick;
        return e.dk;
      }
    return nullptr;
  };
  std::shared_ptr<snarkv_dk> dk;
  {
    std::lock_guard<std::mutex> lk(cache_mu);
    dk = lookup();
  }
  if (!dk) {
    snarkv_dk* fresh = nullptr;
    SNARKV_TRY(snarkv_dk_create(c, g1_64, g2_128, s_g2_128, 0, &fresh));
    std::shared_ptr<snarkv_dk> mine(fresh, [](snarkv_dk* p) { snarkv_dk_destroy(p); });
    std::lock_guard<std::mutex> lk(cache_mu);
    dk = lookup();  // somebody else published the same key meanwhile: use theirs, `mine` is freed on return
    if (!dk) {
      DkCacheEntry* victim = &cache[0];
      for (auto& e : cache) {  // a free slot, else the least recently used
        if (!e.dk) {
          victim = &e;
          break;
        }
        if (e.used < victim->used) victim = &e;
      }
      victim->dk = mine;
      memcpy(victim->tag, now, sizeof now);
      victim->used = ++tick;
      dk = mine;
    }
  }
  return snarkv_kzg_decide_batch(c, dk.get(), accs128, m, 0, ok);
}

int bn254_kzg_decide(const uint8_t g1_64[64], const uint8_t g2_128[128], const uint8_t s_g2_128[128],
                     const uint8_t acc128[128]) {
  uint8_t ok = 0;
  int rc = bn254_kzg_decide_batch(g1_64, g2_128, s_g2_128, acc128, 1, &ok);
  if (rc < 0) return rc;
  return ok ? 1 : 0;
}

int bn254_poseidon_create(uint32_t t, uint32_t rate, uint32_t r_f, uint32_t r_p, const uint8_t* start,
                          const uint8_t* partial, const uint8_t* end, const uint8_t* mds, const uint8_t* pre_sparse_mds,
                          const uint8_t* sparse_rows, const uint8_t* sparse_col_hats, snarkv_poseidon** out) {
  SNARKV_DEFAULT_LEASE(c);
  return snarkv_poseidon_create(c, t, rate, r_f, r_p, start, partial, end, mds, pre_sparse_mds, sparse_rows,
                                sparse_col_hats, out);
}

int bn254_ipa_dk_create(const uint8_t* g_points64, size_t n, snarkv_ipa_dk** out) {
  SNARKV_DEFAULT_LEASE(c);
  return snarkv_ipa_dk_create(c, g_points64, n, out);
}

int bn254_ipa_decide_batch(const snarkv_ipa_dk* dk, const uint8_t* xi32, const uint8_t* u64, size_t m, uint8_t* ok) {
  SNARKV_DEFAULT_LEASE(c);
  return snarkv_ipa_decide_batch(c, dk, xi32, u64, m, ok);
}

int bn254_ipa_commit_batch(const snarkv_ipa_dk* dk, const uint8_t* polys32, size_t n, size_t m, uint8_t* out64s) {
  SNARKV_DEFAULT_LEASE(c);
  return snarkv_ipa_commit_batch(c, dk, polys32, n, m, out64s);
}

int bn254_ipa_decide_folded(const snarkv_ipa_dk* dk, const uint8_t* xi32, const uint8_t* u64, size_t m,
                            const uint8_t rho32[32], int* all_ok) {
  SNARKV_DEFAULT_LEASE(c);
  return snarkv_ipa_decide_folded(c, dk, xi32, u64, m, rho32, all_ok);
}

int bn254_ipa_create_proof(const snarkv_ipa_dk* dk, const uint8_t h64[64], const uint8_t* s64, const uint8_t* coeffs32, size_t n,
                           const uint8_t z32[32], const uint8_t* omega32, const uint8_t* pbar32, const uint8_t* omega_bar32,
                           const uint8_t* absorbed, size_t absorbed_len, uint8_t* proof_out, size_t proof_cap,
                           size_t* proof_len, uint8_t* xi_out32, uint8_t u_out64[64]) {
  SNARKV_DEFAULT_LEASE(c);
  return snarkv_ipa_create_proof(c, dk, h64, s64, coeffs32, n, z32, omega32, pbar32, omega_bar32, absorbed, absorbed_len, proof_out,
                                 proof_cap, proof_len, xi_out32, u_out64);
}

int bn254_ipa_multiopen_create_proof(const snarkv_ipa_dk* dk, const uint8_t h64[64], const uint8_t s64[64], const uint8_t* polys32, size_t n, size_t n_polys,
    const uint8_t* blinds32, const uint8_t x32[32], const uint32_t* q_poly, const uint8_t* q_shift32, const uint8_t* q_eval32,
    size_t n_queries, const uint8_t f_blind32[32], const uint8_t* pbar32, const uint8_t omega_bar32[32], const uint8_t* absorbed,
    size_t absorbed_len, uint8_t* proof_out, size_t proof_cap, size_t* proof_len, uint8_t* xi_out32, uint8_t u_out64[64]) {
  SNARKV_DEFAULT_LEASE(c);
  return snarkv_ipa_multiopen_create_proof(c, dk, h64, s64, polys32, n, n_polys, blinds32, x32, q_poly, q_shift32, q_eval32, n_queries,
                                           f_blind32, pbar32, omega_bar32, absorbed, absorbed_len, proof_out, proof_cap, proof_len,
                                           xi_out32, u_out64);
}

int bn254_poseidon_transcript_batch(const snarkv_poseidon* ps, const uint8_t* elems, size_t n, size_t L,
                                    const uint32_t* seg_len, size_t S, uint8_t* out) {
  SNARKV_DEFAULT_LEASE(c);
  return snarkv_poseidon_transcript_batch(c, ps, elems, n, L, seg_len, S, out);
}

int bn254_poseidon_read_batch(const snarkv_poseidon* ps, const uint8_t* proofs, size_t n, size_t stride, const uint8_t* lead,
                              size_t n_lead, const uint32_t* layout, size_t L, const uint32_t* point_offsets, size_t P,
                              const uint32_t* seg_len, size_t S, uint8_t* challenges, uint8_t* points64, uint8_t* ok) {
  SNARKV_DEFAULT_LEASE(c);
  return snarkv_poseidon_read_batch(c, ps, proofs, n, stride, lead, n_lead, layout, L, point_offsets, P, seg_len, S, challenges,
                                    points64, ok);
}

}  // extern "C"
