// Internal: context object behind the C ABI (include/snarkv_amd.h).
#pragma once
#include <hip/hip_runtime.h>
#include <mutex>
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>
#include "../../include/snarkv_amd.h"
#include "curve_consts.h"

// extern "C" names of the units shared between the BN254 library and the pasta build, and where the two builds'
// MSM entry points (msm_api.hip) differ:
//   SNARKV_CHUNK_PIPELINE  large MSMs may run as the chunk pipeline (pip_chunk_pipeline); the pasta build keeps the
//                          single launch at every size
//   SNARKV_API_FLAGS       the bits of a call's `flags` the entry points honour; the pasta build takes
//                          SNARKV_FLAG_VALIDATE only (include/snarkv_pallas.h)
#if defined(SNARKV_CURVE_PALLAS)
#define SNARKV_API(name) snarkv_pallas_##name
#define SNARKV_CHUNK_PIPELINE 0
#define SNARKV_API_FLAGS SNARKV_FLAG_VALIDATE
#else
#define SNARKV_API(name) snarkv_##name
#define SNARKV_CHUNK_PIPELINE 1
#define SNARKV_API_FLAGS (SNARKV_FLAG_VALIDATE | SNARKV_FLAG_MONTGOMERY)
#endif

namespace snarkv {

void set_last_error(const char* fmt, ...);

#define SNARKV_HIP(expr)                                                                   \
  do {                                                                                     \
    hipError_t _e = (expr);                                                                \
    if (_e != hipSuccess) {                                                                \
      ::snarkv::set_last_error("%s:%d: %s -> %s", __FILE__, __LINE__, #expr, hipGetErrorString(_e)); \
      return SNARKV_ERR_DEVICE;                                                            \
    }                                                                                      \
  } while (0)

#define SNARKV_TRY(expr)      \
  do {                        \
    int _rc = (expr);         \
    if (_rc < 0) return _rc;  \
  } while (0)

// Scratch slots (grow-only device buffers owned by the context).
enum Slot {
  SLOT_IN_SCALARS = 0,
  SLOT_IN_POINTS,
  SLOT_IN_OFFSETS,
  SLOT_OUT,
  SLOT_POINTS_MONT,
  SLOT_COUNTS,
  SLOT_OFFSETS,
  SLOT_CURSOR,
  SLOT_BLOCKSUMS,
  SLOT_ENTRIES,
  SLOT_PIECES,       // S5 piece descriptors (uint4)
  SLOT_SPLIT_PARTS,  // partials of the pieces of split buckets
  SLOT_PIECE_HIST,   // S5 length x workgroup histogram
  SLOT_BUCKETS,
  SLOT_CHUNK_PARTIALS,
  SLOT_WINDOW_SUMS,
  SLOT_TERM_PARTIALS,
  SLOT_FLAGS,
  SLOT_MISC,
  SLOT_SORT_TMP,
  SLOT_SHIFTED,
  SLOT_GLV,
  SLOT_FIX_LISTS,    // k_fixup's lists: small split | big split | degenerate buckets
  SLOT_MISC2,
  SLOT_TERM_CHAIN,
  SLOT_TERM_MAGS,
  SLOT_SPLIT_PARTIALS,
  SLOT_IPA_XI,
  SLOT_IPA_H,
  SLOT_IPA_OUT,
  SLOT_MGPU_GRID,
  SLOT_MGPU_RECV,
  SLOT_IPA_FOLD,     // the folded decide (ipa_fold.hip): challenges and powers in the Montgomery domain, partial vectors
  SLOT_POLY,         // the polynomial calls (poly.hip): the roots and totals of the scan's levels, a staged pass of terms
  SLOT_NTT,          // the transforms (ntt.hip): the tables of powers, then the working buffer of the passes
  SLOT_POLY_PROD,    // the column products (poly_prod.hip): a staged pass of affine terms, the totals of the scans' levels
  SLOT_QUOTIENT,     // the quotient (quotient.hip): the staged program and constants, the vanishing polynomial's table
  SLOT_LOOKUP,       // the lookup argument (lookup.hip): the sort's partition points, the flags and the totals of the count scans
  SLOT_POLY_BATCH,   // the batched evaluation (poly_batch.hip): a chunk's indices, and per query the roots and totals of the levels
  SLOT_BLIND_ROWS,   // the blind term of a blinded commitment (msm_shared.hip): the rows 2^(8 w) S of the last S, S, staging
  SLOT_G1_NTT,       // the transform over group elements (g1_ntt.hip): the twiddles, two working buffers, the window tables
  SLOT_COUNT
};

}  // namespace snarkv

struct snarkv_ctx {
  int device;
  hipStream_t stream;
  bool own_stream;
  void* buf[snarkv::SLOT_COUNT];
  size_t cap[snarkv::SLOT_COUNT];
  // pinned host buffers handed to the caller (snarkv_ctx_host_buffer): inputs packed there reach the device by DMA
  // instead of the runtime's bounce copy of pageable memory
  void* hbuf[SNARKV_HOST_BUFFERS];
  size_t hbuf_cap[SNARKV_HOST_BUFFERS];
  uint32_t flags;  // default flags of the context (snarkv_ctx_set_flags), OR-ed into every call's own
  bool mont;       // SNARKV_FLAG_MONTGOMERY in effect for the call being enqueued (set by the entry points)
  bool stage_timing;
  float stage_ms[SNARKV_PIP_STAGES];
  hipEvent_t ev[SNARKV_PIP_STAGES + 1];
  bool ev_ready;
  // large MSMs run as pipelined 2^20-point chunks on private sub-contexts (msm_api.hip)
  snarkv_ctx* sub[4];
  hipEvent_t sub_ev[5];
  bool sub_ready;
  hipEvent_t sorted_ev;  // job contexts of a batch: this job's prepare + sort is done (its accumulation waits for it)
  bool sorted_ev_ready;
  int last_split_workers;  // > 0: the last Pippenger ran as a chunk pipeline on that many worker lanes (stage timing)
  bool throughput_mode;  // several MSMs are kept in flight next to this context's (snarkv_ctx_set_throughput_hint; always on lanes)
  int throughput_peers;  // how many launches share the GPU under the hint (0 = unknown: 16, what bench.py keeps in flight)
  bool is_lane;          // a private sub-context of another context (never starts lanes of its own)
  // job contexts of the batch entry point (snarkv_g1_msm_pippenger_many_dev): scratch of one MSM each
  snarkv_ctx* jobs[SNARKV_MANY_MAX_JOBS];
  int njobs;
  int last_many_jobs;    // > 0: the last call was a batch of that many jobs per round (stage timing reads the jobs' events)
  size_t many_sig;       // shape of the last batch (a new shape may grow scratch: synchronise first)
  hipStream_t copy_stream;   // host-resident batches (snarkv_g1_msm_pippenger_many): the uploads, one event per job
  bool copy_ready;
  hipEvent_t many_ev[2];
  hipEvent_t order_ev;  // snarkv_ctx_wait_stream / snarkv_stream_wait_ctx: the record-and-wait event
  bool order_ev_ready;
  hipStream_t hi_stream[2];  // high-priority streams of the batch pipeline (the sorts) + their join events (many_ev)
  bool hi_ready;
  // the transforms (ntt.hip): which (k, direction) the tables in SLOT_NTT were built for (0: none), and where the slot was then
  void* ntt_tables;
  uint32_t ntt_key;
  // the blind term (msm_shared.hip): the S that the rows in SLOT_BLIND_ROWS were built for
  uint8_t blind_s[64];
  bool blind_rows_ready;
};

struct snarkv_dk {
  int device;
  void* d_prep;  // 2 x G2Prepared29 (g2, -s_g2): the line tables the decide kernels read
  uint8_t g1[64];
};

// the IPA deciding key (ipa.hip); the prover session (ipa_prover.hip) reads its points
struct snarkv_ipa_dk {
  int device;
  uint32_t k;
  void* d_points;  // the points held: 64 B canonical affine each, as the Pippenger entry point takes them
  size_t first;    // index of the first point held in the 2^k-point key (0 unless a multi-GPU shard)
  size_t count;    // points held (2^k unless a shard)
  // the window table of the shared-key MSM (msm_shared.hip): T[w][j] = 2^(8 w) G[j], packed Montgomery affine.  Built at most
  // once per key, under `table_mu` (handles are shared between host threads), by the first batched call or by
  // snarkv_ipa_dk_prepare; freed with the key.  The fields are mutable: every call takes the key as const.
  mutable std::mutex table_mu;
  mutable int table_state;     // 0 not tried, 1 built, 2 declined (a shard, or over kSharedTableCap)
  mutable void* d_table;
  mutable size_t table_bytes;  // 0 until built
};

namespace snarkv {

// The encoding of a call = the context's default flags | the call's own: kept in ctx->mont while the call enqueues its
// kernels (every launcher reads it), restored on the way out.
struct CallFlags {
  snarkv_ctx* c;
  bool saved;
  CallFlags(snarkv_ctx* ctx, uint32_t call_flags) : c(ctx), saved(ctx ? ctx->mont : false) {
    if (c) c->mont = ((c->flags | call_flags) & SNARKV_FLAG_MONTGOMERY) != 0;
  }
  ~CallFlags() {
    if (c) c->mont = saved;
  }
};
#define SNARKV_CALL_FLAGS(ctx, f) ::snarkv::CallFlags _call_flags((ctx), (f))
// Entry points SNARKV_FLAG_MONTGOMERY does NOT cover (the IPA, the Poseidon transcripts: include/snarkv_amd.h): their
// kernels run in the wire form whatever the context's default says
struct WireFormScope {
  snarkv_ctx* c;
  bool saved;
  explicit WireFormScope(snarkv_ctx* ctx) : c(ctx), saved(ctx ? ctx->mont : false) {
    if (c) c->mont = false;
  }
  ~WireFormScope() {
    if (c) c->mont = saved;
  }
};
#define SNARKV_WIRE_FORM(ctx) ::snarkv::WireFormScope _wire_form((ctx))

// Ensure slot capacity; returns device pointer through *out.
int ctx_reserve(snarkv_ctx* ctx, int slot, size_t bytes, void** out);
// staging of the host-resident entry points (ctx.hip): host bytes into a slot, a result back to the host (synchronous),
// and the device check of SNARKV_FLAG_VALIDATE (the call's flags | the context's)
int stage_in(snarkv_ctx* ctx, int slot, const void* host, size_t bytes, void** d);
int fetch_out(snarkv_ctx* ctx, const void* d, void* host, size_t bytes);
int check_validate(snarkv_ctx* ctx, const void* d_s, const void* d_p, size_t n, uint32_t flags);
// four lanes (the context's stream + three private sub-contexts) for independent launches: ctx.hip
int ctx_lanes(snarkv_ctx* ctx);
int ctx_lanes_fork(snarkv_ctx* ctx);
int ctx_lanes_join(snarkv_ctx* ctx);
inline snarkv_ctx* ctx_lane(snarkv_ctx* ctx, size_t i) { return (i % 4 == 3) ? ctx : ctx->sub[i % 4]; }

// kernels' host-side launchers (each enqueues on ctx->stream)
int launch_msm_batched(snarkv_ctx* ctx, const void* d_scalars, const void* d_points, const void* d_offsets,
                       size_t n_msm, size_t n_terms, void* d_out);
int launch_g1_decompress(snarkv_ctx* ctx, const void* d_in32, size_t n, void* d_out64, void* d_ok);
int launch_msm_pippenger(snarkv_ctx* ctx, const void* d_scalars, const void* d_points, size_t n, int window_bits,
                         void* d_out, bool partial_out, void* d_buckets_out = nullptr);
// one Pippenger cut into phases, each on a stream of the caller's choice (msm_pippenger.hip); `ctx` owns the scratch
enum { PIP_PHASE_SORT = 1, PIP_PHASE_ACC = 2, PIP_PHASE_TAIL = 4, PIP_PHASE_ALL = 7 };
int launch_msm_pippenger_phases(snarkv_ctx* ctx, hipStream_t st, int phases, const void* d_scalars, const void* d_points,
                                size_t n, int window_bits, void* d_out, bool partial_out, void* d_buckets_out,
                                void* d_grid);
int launch_buckets_reduce_many(snarkv_ctx* ctx, hipStream_t st, const void* d_grids, uint32_t c, uint32_t windows,
                               uint32_t jobs, void* d_out, bool partial_out);
// `count` independent MSMs, phase-ordered over private job contexts (msm_api.hip)
// `ready` (optional): one event per job -- its inputs are in place (uploads of a host-resident batch); a job's first kernel
// waits for its event only, so the uploads of later jobs run under the kernels of earlier ones
int launch_msm_pippenger_many(snarkv_ctx* ctx, size_t count, const void* const* d_scalars, const void* const* d_points,
                              const size_t* n, int window_bits, void* d_out, bool partial_out, hipEvent_t* ready = nullptr);
// the product path of a large MSM: single launch, or the chunk pipeline over shared bucket grids (msm_api.hip)
int launch_msm_pippenger_auto(snarkv_ctx* ctx, const void* d_scalars, const void* d_points, size_t n, int window_bits,
                              void* d_out, bool partial_out);
// does an n-point MSM run as the chunk pipeline over shared bucket grids? (the one rule: msm_api.hip)
bool pip_chunk_pipeline(size_t n, int window_bits, bool is_lane, size_t* chunk);
// the host-staged Pippenger behind snarkv_g1_msm_pippenger / snarkv_pallas_g1_msm_pippenger (msm_api.hip)
int msm_pippenger_staged(snarkv_ctx* ctx, const uint8_t* scalars32, const uint8_t* points64, size_t n, uint32_t flags,
                         uint8_t out64[64]);
int pip_geometry(size_t n_total, int window_bits, uint32_t* c, uint32_t* windows, uint32_t* buckets_per_window);
int launch_buckets_add(snarkv_ctx* ctx, void* d_dst, const void* d_src, size_t count);
int launch_buckets_reduce(snarkv_ctx* ctx, const void* d_buckets, uint32_t c, uint32_t w0, uint32_t wcount, void* d_partial);
int launch_fold_partials(snarkv_ctx* ctx, const void* d_partials, size_t count, void* d_out64, bool partial_out = false);
int launch_fold_partials_many(snarkv_ctx* ctx, const void* d_partials, size_t count, size_t jobs, void* d_out64s);
// the shared-key MSM (msm_shared.hip): many scalar vectors against the window table of one resident key
constexpr size_t kSharedTableCap = (size_t)256 << 20;  // largest table built (2 KiB per base: keys up to 2^17)
// can this key have a table at all? (whole key, table within the cap)
bool ipa_dk_table_fits(const snarkv_ipa_dk* dk);
// build the table if it is not there and fits; *have = the table can be used.  Synchronises ctx->stream when it builds.
int ipa_dk_table_prepare(snarkv_ctx* ctx, const snarkv_ipa_dk* dk, bool* have);
// out[a] = sum_{j < n} s[a][j] G[j], a < m: d_scalars = m x n canonical scalars, d_out64s = m affine points in the call's
// encoding.  The table must be built.  slices = 0: chosen so that m x slices workgroups fill the machine.
int launch_msm_shared(snarkv_ctx* ctx, const snarkv_ipa_dk* dk, const void* d_scalars, size_t n, size_t m, uint32_t slices,
                      void* d_out64s);
// ... + blinds[a] * S: d_blinds = m canonical scalars in device memory, s64 = S on the host (read before the call returns).  The
// blind terms are one more partial per vector, computed beside the MSM on the context's first lane.
int launch_msm_shared_blinded(snarkv_ctx* ctx, const snarkv_ipa_dk* dk, const void* d_scalars, size_t n, size_t m,
                              uint32_t slices, const void* d_blinds, const uint8_t* s64, void* d_out64s);
// enqueue steps that another unit chains (quotient.hip), arguments taken as checked: the transform of snarkv_ntt_dev
// (ntt.hip; shift = 8 canonical words or null) and the batch inversion of snarkv_poly_batch_invert_dev (poly_prod.hip)
int ntt_enqueue(snarkv_ctx* ctx, const void* d_in, void* d_out, uint32_t k, size_t count, bool inverse, const uint32_t* shift);
int prod_batch_invert_enqueue(snarkv_ctx* ctx, const void* d_in, size_t n, void* d_out);
// ... and, for the lookup product (lookup.hip), the steps of snarkv_poly_mul_dev, snarkv_poly_prod_affine_dev and
// snarkv_poly_grand_product_dev
int prod_mul_enqueue(snarkv_ctx* ctx, const void* d_a, const void* d_b, size_t n, void* d_out);
int prod_affine_enqueue(snarkv_ctx* ctx, const void* d_polys, size_t n, const uint32_t* idx_a, const uint32_t* idx_b,
                        const uint8_t* betas32, const uint8_t* gammas32, size_t count, void* d_out);
int prod_grand_product_enqueue(snarkv_ctx* ctx, const void* d_f, size_t n, const void* d_start, void* d_out, void* d_total);
int launch_validate(snarkv_ctx* ctx, const void* d_scalars, const void* d_points, size_t n, int* bad_host);
int launch_g2_prepare(snarkv_ctx* ctx, const void* d_g2x2_256, void* d_prep);
int launch_decide(snarkv_ctx* ctx, const void* d_prep, const void* d_accs, size_t m, void* d_ok, void* d_gt);
int launch_validate_g2(snarkv_ctx* ctx, const void* d_g2x2_256, int* bad_host);
size_t g2_prepared_bytes();
int launch_sample_scalars(snarkv_ctx* ctx, uint64_t seed, uint64_t first, size_t n, void* d_out);
int launch_sample_points(snarkv_ctx* ctx, uint64_t seed, uint64_t first, size_t n, void* d_out);
int launch_ubench(snarkv_ctx* ctx, int which, int iters, double* ops_per_s);

}  // namespace snarkv
