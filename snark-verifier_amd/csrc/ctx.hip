// Context object behind the C ABI: error string, grow-only scratch slots, create / destroy / sync, the staging
// helpers of the entry points.  Built into both libraries (BN254: snarkv_*, the pasta build: snarkv_pallas_*); the
// entry point names come from SNARKV_API (ctx.hpp).
#include <stdarg.h>
#include <string.h>
#include "ctx.hpp"

namespace snarkv {

static thread_local char g_err[512] = "";

void set_last_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
}

int ctx_reserve(snarkv_ctx* ctx, int slot, size_t bytes, void** out) {
  if (bytes == 0) bytes = 16;
  if (ctx->cap[slot] < bytes) {
    if (ctx->buf[slot]) {
      // earlier launches may still use the old buffer: on the context's stream -- or, for a lane / job context, on
      // whichever stream of the owning scheduler its phases were enqueued on (msm_api.hip: the batch's sort and
      // accumulation streams never are the job's own), so a lane waits for the whole device
      if (ctx->is_lane) SNARKV_HIP(hipDeviceSynchronize());
      else SNARKV_HIP(hipStreamSynchronize(ctx->stream));
      SNARKV_HIP(hipFree(ctx->buf[slot]));
      ctx->buf[slot] = nullptr;
      ctx->cap[slot] = 0;
    }
    size_t cap = bytes + bytes / 8 + 256;
    SNARKV_HIP(hipMalloc(&ctx->buf[slot], cap));
    ctx->cap[slot] = cap;
  }
  *out = ctx->buf[slot];
  return SNARKV_OK;
}

int stage_in(snarkv_ctx* ctx, int slot, const void* host, size_t bytes, void** d) {
  SNARKV_TRY(ctx_reserve(ctx, slot, bytes, d));
  SNARKV_HIP(hipMemcpyAsync(*d, host, bytes, hipMemcpyHostToDevice, ctx->stream));
  return SNARKV_OK;
}

int fetch_out(snarkv_ctx* ctx, const void* d, void* host, size_t bytes) {
  SNARKV_HIP(hipMemcpyAsync(host, d, bytes, hipMemcpyDeviceToHost, ctx->stream));
  SNARKV_HIP(hipStreamSynchronize(ctx->stream));
  return SNARKV_OK;
}

int check_validate(snarkv_ctx* ctx, const void* d_s, const void* d_p, size_t n, uint32_t flags) {
  if (!((flags | ctx->flags) & SNARKV_FLAG_VALIDATE)) return SNARKV_OK;
  int bad = 0;
  SNARKV_TRY(launch_validate(ctx, d_s, d_p, n, &bad));
  if (bad) {
    set_last_error("%d of %zu inputs are non-canonical or off-curve", bad, n);
    return SNARKV_ERR_ENCODING;
  }
  return SNARKV_OK;
}

}  // namespace snarkv

extern "C" {

const char* SNARKV_API(last_error)(void) { return snarkv::g_err; }
const char* SNARKV_API(version)(void) { return "snarkv_amd 0.1 (gfx950, " SNARKV_CURVE_NAME ")"; }

int SNARKV_API(ctx_create)(int device, void* hip_stream, snarkv_ctx** out) {
  if (!out) return SNARKV_ERR_ARG;
  int count = 0;
  SNARKV_HIP(hipGetDeviceCount(&count));
  if (count <= 0 || device < 0 || device >= count) {
    snarkv::set_last_error("no HIP device %d (count=%d): the MI355X path has no CPU fallback", device, count);
    return SNARKV_ERR_DEVICE;
  }
  SNARKV_HIP(hipSetDevice(device));
  snarkv_ctx* c = new snarkv_ctx();
  memset(c, 0, sizeof(*c));
  c->device = device;
  if (hip_stream) {
    c->stream = (hipStream_t)hip_stream;
    c->own_stream = false;
  } else {
    hipError_t e = hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking);
    if (e != hipSuccess) {
      snarkv::set_last_error("hipStreamCreate: %s", hipGetErrorString(e));
      delete c;
      return SNARKV_ERR_DEVICE;
    }
    c->own_stream = true;
  }
  *out = c;
  return SNARKV_OK;
}

void SNARKV_API(ctx_destroy)(snarkv_ctx* ctx) {
  if (!ctx) return;
  (void)hipSetDevice(ctx->device);
  (void)hipStreamSynchronize(ctx->stream);
  for (int i = 0; i < snarkv::SLOT_COUNT; ++i)
    if (ctx->buf[i]) (void)hipFree(ctx->buf[i]);
  for (int i = 0; i < SNARKV_HOST_BUFFERS; ++i)
    if (ctx->hbuf[i]) (void)hipHostFree(ctx->hbuf[i]);
  if (ctx->ev_ready)
    for (int i = 0; i <= SNARKV_PIP_STAGES; ++i) (void)hipEventDestroy(ctx->ev[i]);
  if (ctx->sub_ready) {
    for (int i = 0; i < 3; ++i) SNARKV_API(ctx_destroy)(ctx->sub[i]);
    for (int i = 0; i < 5; ++i) (void)hipEventDestroy(ctx->sub_ev[i]);
  }
  if (ctx->sorted_ev_ready) (void)hipEventDestroy(ctx->sorted_ev);
  for (int i = 0; i < ctx->njobs; ++i) SNARKV_API(ctx_destroy)(ctx->jobs[i]);
  if (ctx->hi_ready)
    for (int i = 0; i < 2; ++i) {
      (void)hipStreamDestroy(ctx->hi_stream[i]);
      (void)hipEventDestroy(ctx->many_ev[i]);
    }
  if (ctx->copy_ready) (void)hipStreamDestroy(ctx->copy_stream);
  if (ctx->order_ev_ready) (void)hipEventDestroy(ctx->order_ev);
  if (ctx->own_stream) (void)hipStreamDestroy(ctx->stream);
  delete ctx;
}

int SNARKV_API(ctx_host_buffer)(snarkv_ctx* ctx, int slot, size_t bytes, void** out) {
  if (!ctx || !out || slot < 0 || slot >= SNARKV_HOST_BUFFERS) return SNARKV_ERR_ARG;
  if (bytes == 0) bytes = 16;
  if (ctx->hbuf_cap[slot] < bytes) {
    SNARKV_HIP(hipSetDevice(ctx->device));
    if (ctx->hbuf[slot]) {
      SNARKV_HIP(hipStreamSynchronize(ctx->stream));  // a copy out of the old buffer may still be queued
      SNARKV_HIP(hipHostFree(ctx->hbuf[slot]));
      ctx->hbuf[slot] = nullptr;
      ctx->hbuf_cap[slot] = 0;
    }
    size_t cap = bytes + bytes / 4 + 4096;
    SNARKV_HIP(hipHostMalloc(&ctx->hbuf[slot], cap, hipHostMallocDefault));
    ctx->hbuf_cap[slot] = cap;
  }
  *out = ctx->hbuf[slot];
  return SNARKV_OK;
}

int SNARKV_API(ctx_sync)(snarkv_ctx* ctx) {
  if (!ctx) return SNARKV_ERR_ARG;
  SNARKV_HIP(hipStreamSynchronize(ctx->stream));
  return SNARKV_OK;
}

// Cross-stream ordering for the asynchronous `_dev` entry points: one event, recorded on the producer stream and waited
// for by the consumer stream.  Re-recording the event later does not disturb a wait already enqueued (the wait
// captures the record that preceded it), so one event per context serves every call.
static int order_streams(snarkv_ctx* ctx, hipStream_t first, hipStream_t then) {
  if (first == then) return SNARKV_OK;
  SNARKV_HIP(hipSetDevice(ctx->device));
  if (!ctx->order_ev_ready) {
    SNARKV_HIP(hipEventCreateWithFlags(&ctx->order_ev, hipEventDisableTiming));
    ctx->order_ev_ready = true;
  }
  SNARKV_HIP(hipEventRecord(ctx->order_ev, first));
  SNARKV_HIP(hipStreamWaitEvent(then, ctx->order_ev, 0));
  return SNARKV_OK;
}

int SNARKV_API(ctx_wait_stream)(snarkv_ctx* ctx, void* hip_stream) {
  if (!ctx) return SNARKV_ERR_ARG;
  return order_streams(ctx, (hipStream_t)hip_stream, ctx->stream);
}

int SNARKV_API(stream_wait_ctx)(snarkv_ctx* ctx, void* hip_stream) {
  if (!ctx) return SNARKV_ERR_ARG;
  return order_streams(ctx, ctx->stream, (hipStream_t)hip_stream);
}

void* SNARKV_API(ctx_stream)(snarkv_ctx* ctx) { return ctx ? (void*)ctx->stream : nullptr; }

}  // extern "C"

namespace snarkv {

// Four lanes for independent launches on one context: the caller's own stream + three private
// sub-contexts (one HIP stream + scratch each).  Not four private ones: HIP multiplexes streams onto
// 4 hardware queues by default, and a fifth busy stream would share a queue with one of the lanes.
// (Streams sharing a queue serialise.  The queue count is a process-wide setting of the runtime and the
// host: the library never touches it.)
int ctx_lanes(snarkv_ctx* ctx) {
  if (!ctx->sub_ready) {
    for (int i = 0; i < 3; ++i) {
      SNARKV_TRY(SNARKV_API(ctx_create)(ctx->device, nullptr, &ctx->sub[i]));
      ctx->sub[i]->throughput_mode = true;  // a lane runs next to other lanes
      ctx->sub[i]->is_lane = true;
    }
    ctx->sub[3] = nullptr;
    for (int i = 0; i < 5; ++i) SNARKV_HIP(hipEventCreateWithFlags(&ctx->sub_ev[i], hipEventDisableTiming));
    ctx->sub_ready = true;
  }
  return SNARKV_OK;
}
// everything queued on the caller's stream so far happens-before the sub-lanes' next work
int ctx_lanes_fork(snarkv_ctx* ctx) {
  SNARKV_HIP(hipEventRecord(ctx->sub_ev[4], ctx->stream));
  for (int i = 0; i < 3; ++i) {
    SNARKV_HIP(hipStreamWaitEvent(ctx->sub[i]->stream, ctx->sub_ev[4], 0));
    ctx->sub[i]->mont = ctx->mont;  // the lanes work in the encoding of the call that forks them (never a stale one)
  }
  return SNARKV_OK;
}
// ... and the sub-lanes' work happens-before whatever the caller's stream does next
int ctx_lanes_join(snarkv_ctx* ctx) {
  for (int i = 0; i < 3; ++i) {
    SNARKV_HIP(hipEventRecord(ctx->sub_ev[i], ctx->sub[i]->stream));
    SNARKV_HIP(hipStreamWaitEvent(ctx->stream, ctx->sub_ev[i], 0));
  }
  return SNARKV_OK;
}

}  // namespace snarkv
