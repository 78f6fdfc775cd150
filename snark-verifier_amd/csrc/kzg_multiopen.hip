// The two KZG multi-open provers (include/snarkv_kzg_multiopen.h) on the pieces of poly.hip and the Pippenger batch.
//   host    the plan (kzg_multiopen_plan.h): sets, per set the lincomb scalars, the points z shift_t, the coefficients of r
//   device  per set  q = sum c^j polys[..]                 poly_enqueue_lincomb
//                    (q - r) / prod (X - point)             k_kzg_axpy_sub + poly_enqueue_div_linear per point, ping-pong;
//                                                           a remainder marks the set in the status word (k_kzg_check_rem)
//   Gwc19   the S quotients are S jobs of ONE launch_msm_pippenger_many over the one base        -> the only sync: ws, status
//   Bdfg21  h += gamma^i quotient_i (k_kzg_axpy_sub), W = commit(h)                              -> sync 1: W, status
//           host: draw_z_prime(W), the rest of the plan
//           L = sum scalars polys[..] - Z_1(z') h - constant   poly_enqueue_lincomb + k_kzg_axpy_sub
//           W' = commit(L / (X - z')), its remainder checked the same way                        -> sync 2: W', status
// One linear factor per division, as the IPA multi-open prover: a set of m points costs m scans.
#include <string.h>
#include <algorithm>
#include <vector>
#include "ipa_opening.hpp"
#include "kzg_multiopen_plan.h"
#include "poly.hpp"
#include "poly_args.hpp"
#include "../../include/snarkv_kzg_multiopen.h"

namespace snarkv {

// out[j] += scalar * src[j] for j < n (src = null: nothing is added), then out[j] -= sub[j] for j < m
__global__ void __launch_bounds__(256) k_kzg_axpy_sub(uint32_t* __restrict__ out, const uint32_t* __restrict__ src,
                                                      const uint32_t* __restrict__ scalar, uint32_t n,
                                                      const uint32_t* __restrict__ sub, uint32_t m) {
  const uint32_t j = blockIdx.x * 256u + threadIdx.x;
  if (j >= n || (!src && j >= m)) return;
  Fr29 a = ld_fr(out + 8 * (size_t)j);  // (-r/2, 3r/2), and so is every term below: within fr29_to_canonical's 8 r
  if (src) a = fr29_norm(fr29_add(a, fr29_mul(ld_fr(scalar), ld_fr(src + 8 * (size_t)j))));
  if (j < m) {
    const Fr29 b = ld_fr(sub + 8 * (size_t)j);
#pragma unroll
    for (int i = 0; i < 9; ++i) a.v[i] -= b.v[i];
  }
  st_fr(out + 8 * (size_t)j, a);
}

// a remainder (canonical) that is not zero marks its set; the pipeline runs on
__global__ void __launch_bounds__(64) k_kzg_check_rem(const uint32_t* __restrict__ rem, uint32_t set, uint32_t* __restrict__ first_bad) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  uint32_t any = 0;
  for (int w = 0; w < 8; ++w) any |= rem[w];
  if (any) atomicMin(first_bad, set);
}

namespace {

using namespace kzgplan;

struct KzgArgs {
  const char* who;
  int mos;
  const void *srs, *polys;
  bool on_device;
  size_t n, n_polys, n_queries;
  const uint8_t *z32, *q_shift32, *q_eval32, *c32, *gamma32;
  const uint32_t* q_poly;
};

constexpr uint32_t kNone = 0xffffffffu;

// the small device block of a call: status words, the scalars the kernels read, the outputs
enum : size_t {
  KB_STATUS = 0,   // [0] the first set whose division left a remainder, [1] the same for L / (X - z'), [2] the validate count
  KB_SCALAR = 32,  // the scalar of k_kzg_axpy_sub: gamma^i, then -Z_1(z')
  KB_SUB = 64,     // L's constant
  KB_ZP = 96,      // z'
  KB_REM = 128,    // the remainder of L / (X - z')
  KB_OUT = 192,    // W | W' (Bdfg21); Gwc19's ws follow the variable part
  KB_VAR = 320,    // per set: points | remainders | r | gamma^i
};

int refuse_plan(const char* who, int what, size_t set) {
  if (what == kCoincide) set_last_error("%s: two points of query set %zu coincide", who, set);
  else if (what == kTooManyPoints) set_last_error("%s: query set %zu has more points than the polynomials have coefficients", who, set);
  else if (what == kZeroZ) set_last_error("%s: z' is a point of query set %zu", who, set);
  else set_last_error("%s: unknown scheme", who);
  return SNARKV_ERR_ARG;
}

struct KzgRun {
  snarkv_ctx* ctx;
  const KzgArgs& a;
  KzgPlan plan;
  Buffers bufs;
  uint8_t *blk = nullptr, *d_t = nullptr, *d_quot = nullptr;
  const uint8_t *d_polys = nullptr, *d_srs = nullptr;
  size_t total_points = 0, var_pts = 0, var_rem = 0, var_r = 0, var_g = 0, var_ws = 0, blk_bytes = 0;
  std::vector<size_t> first_point;

  KzgRun(snarkv_ctx* c, const KzgArgs& args) : ctx(c), a(args), bufs(c->stream) {}

  // buffers and staging: `quots` quotient polynomials of n coefficients each are kept
  int open(size_t quots) {
    const size_t n = a.n, S = plan.sets.size();
    hipStream_t s = ctx->stream;
    for (const KzgPlanSet& st : plan.sets) {
      first_point.push_back(total_points);
      total_points += st.m();
    }
    var_pts = KB_VAR, var_rem = var_pts + 32 * total_points, var_r = var_rem + 32 * total_points;
    var_g = var_r + 32 * total_points, var_ws = var_g + 32 * S, blk_bytes = var_ws + 64 * S;
    std::vector<uint8_t> stage(blk_bytes, 0);
    const uint32_t st0[3] = {kNone, kNone, 0};
    memcpy(&stage[KB_STATUS], st0, sizeof(st0));
    const std::vector<Fr29> pg = h_powers(a.gamma32 ? h_load(a.gamma32) : fr29_one(), S);
    for (size_t i = 0; i < S; ++i) {
      const KzgPlanSet& st = plan.sets[i];
      memcpy(&stage[var_pts + 32 * first_point[i]], st.points.data(), st.points.size());
      memcpy(&stage[var_r + 32 * first_point[i]], st.r.data(), st.r.size());
      h_store(&stage[var_g + 32 * i], pg[i]);
    }
    void *d_blk, *d_p = nullptr, *d_s = nullptr, *d_t_, *d_q_;
    SNARKV_TRY(bufs.get(&d_blk, blk_bytes));
    if (!a.on_device) {
      SNARKV_TRY(bufs.get(&d_p, 32 * n * a.n_polys));
      SNARKV_TRY(bufs.get(&d_s, 64 * n));
    }
    SNARKV_TRY(bufs.get(&d_t_, 32 * n * 2));
    SNARKV_TRY(bufs.get(&d_q_, 32 * n * quots));
    blk = (uint8_t*)d_blk, d_t = (uint8_t*)d_t_, d_quot = (uint8_t*)d_q_;
    d_polys = a.on_device ? (const uint8_t*)a.polys : (const uint8_t*)d_p;
    d_srs = a.on_device ? (const uint8_t*)a.srs : (const uint8_t*)d_s;
    // `stage` is pageable: the copy has left it when hipMemcpyAsync returns
    SNARKV_HIP(hipMemcpyAsync(blk, stage.data(), blk_bytes, hipMemcpyHostToDevice, s));
    if (!a.on_device) {
      SNARKV_HIP(hipMemcpyAsync(d_p, a.polys, 32 * n * a.n_polys, hipMemcpyHostToDevice, s));
      SNARKV_HIP(hipMemcpyAsync(d_s, a.srs, 64 * n, hipMemcpyHostToDevice, s));
    }
    if (ctx->flags & SNARKV_FLAG_VALIDATE) {
      const size_t step = (size_t)1 << 30, total = n * a.n_polys;
      int bad = 0;
      for (size_t i = 0; i < total && !bad; i += step)
        SNARKV_TRY(count_bad(ctx, d_polys + 32 * i, std::min(step, total - i), (int*)(blk + KB_STATUS + 8), &bad));
      if (bad) {
        set_last_error("%s: %d coefficients of the polynomials are not canonical", a.who, bad);
        return SNARKV_ERR_ENCODING;
      }
    }
    return SNARKV_OK;
  }

  uint32_t* status() { return (uint32_t*)(blk + KB_STATUS); }

  // out[j] += scalar src[j] (j < n), out[j] -= sub[j] (j < m)
  int axpy_sub(uint8_t* out, const uint8_t* src, const uint8_t* scalar, const uint8_t* sub, size_t m) {
    const size_t span = src ? a.n : m;
    if (span == 0) return SNARKV_OK;
    hipLaunchKernelGGL(k_kzg_axpy_sub, dim3((uint32_t)((span + 255) / 256)), dim3(256), 0, ctx->stream, (uint32_t*)out,
                       (const uint32_t*)src, (const uint32_t*)scalar, (uint32_t)a.n, (const uint32_t*)sub, (uint32_t)m);
    SNARKV_HIP(hipGetLastError());
    return SNARKV_OK;
  }

  // src (n coefficients, overwritten when it is a work polynomial) / prod_t (X - points[t]) -> dst (n coefficients, the top
  // ones zero); src is one half of d_t, the other half is the ping-pong partner.  Every remainder is checked into `word`.
  int divide(uint8_t* src, const uint8_t* points, uint8_t* rems, size_t m, uint32_t set, uint32_t* word, uint8_t* dst) {
    const size_t n = a.n;
    hipStream_t s = ctx->stream;
    size_t len = n;
    for (size_t t = 0; t < m; ++t) {
      uint8_t* to = t + 1 == m ? dst : (src == d_t ? d_t + 32 * n : d_t);
      uint8_t* rem = rems + 32 * t;
      SNARKV_TRY(poly_enqueue_div_linear(ctx, src, len, points + 32 * t, len > 1 ? to : nullptr, rem));
      len -= 1;
      SNARKV_HIP(hipMemsetAsync(to + 32 * len, 0, 32 * (n - len), s));  // the quotient has `len` coefficients
      hipLaunchKernelGGL(k_kzg_check_rem, dim3(1), dim3(64), 0, s, (const uint32_t*)rem, set, word);
      SNARKV_HIP(hipGetLastError());
      src = to;
    }
    return SNARKV_OK;
  }

  // set i: (sum c^j polys[..] - r) / prod (X - point) -> dst
  int set_quotient(size_t i, uint8_t* dst) {
    const KzgPlanSet& st = plan.sets[i];
    SNARKV_TRY(poly_enqueue_lincomb(ctx, d_polys, a.n, st.idx.data(), st.scalars.data(), st.idx.size(), d_t));
    SNARKV_TRY(axpy_sub(d_t, nullptr, nullptr, blk + var_r + 32 * first_point[i], st.m()));
    return divide(d_t, blk + var_pts + 32 * first_point[i], blk + var_rem + 32 * first_point[i], st.m(), (uint32_t)i, status(), dst);
  }

  int refuse_bad_set(uint32_t set) {
    set_last_error("%s: evaluation does not match the polynomial (query set %u)", a.who, set);
    return SNARKV_ERR_ARG;
  }
};

int check_common(snarkv_ctx* ctx, const KzgArgs& a) {
  if (!ctx || !a.srs || !a.polys || !a.z32 || !a.q_poly || !a.q_shift32 || !a.q_eval32 || !a.c32) {
    set_last_error("%s: a null argument", a.who);
    return SNARKV_ERR_ARG;
  }
  if (a.on_device && (!aligned16(a.srs) || !aligned16(a.polys))) return SNARKV_ERR_ARG;
  if (a.n_polys == 0 || a.n_queries == 0) return SNARKV_ERR_EMPTY;
  SNARKV_TRY(check_len(a.n, kPolyMaxLen));
  for (size_t i = 0; i < a.n_queries; ++i)
    if (a.q_poly[i] >= a.n_polys) {
      set_last_error("%s: query %zu names polynomial %u of %zu", a.who, i, a.q_poly[i], a.n_polys);
      return SNARKV_ERR_ARG;
    }
  return SNARKV_OK;
}

int check_canonical(snarkv_ctx* ctx, const KzgArgs& a) {
  if (!(ctx->flags & SNARKV_FLAG_VALIDATE)) return SNARKV_OK;
  bool ok = below_r(a.z32) && below_r(a.c32) && (!a.gamma32 || below_r(a.gamma32));
  ok = ok && all_below_r(a.q_shift32, a.n_queries) && all_below_r(a.q_eval32, a.n_queries);
  if (!ok) {
    set_last_error("%s: z, a challenge, a shift or an evaluation is not canonical", a.who);
    return SNARKV_ERR_ENCODING;
  }
  return SNARKV_OK;
}

int gwc19_create_proof(snarkv_ctx* ctx, const KzgArgs& a, uint8_t* ws_out64, size_t ws_cap, size_t* n_sets_out) {
  SNARKV_TRY(check_common(ctx, a));
  if (!ws_out64 || !n_sets_out) {
    set_last_error("%s: a null argument", a.who);
    return SNARKV_ERR_ARG;
  }
  KzgRun run(ctx, a);
  size_t bad_set = 0;
  {
    std::vector<MultiopenSet> sets;
    (void)kzg_plan_sets(a.mos, a.q_poly, a.q_shift32, a.n_queries, &sets);
    *n_sets_out = sets.size();
    if (ws_cap < sets.size()) {
      set_last_error("%s: there are %zu query sets, ws_cap is %zu", a.who, sets.size(), ws_cap);
      return SNARKV_ERR_LENGTH;
    }
  }
  SNARKV_TRY(check_canonical(ctx, a));
  const int what = kzg_plan_build(a.mos, a.q_poly, a.q_shift32, a.q_eval32, a.n_queries, a.n, a.z32, a.c32, &run.plan, &bad_set);
  if (what != kOk) return refuse_plan(a.who, what, bad_set);
  const size_t S = run.plan.sets.size(), n = a.n;
  SNARKV_HIP(hipSetDevice(ctx->device));
  SNARKV_WIRE_FORM(ctx);
  hipStream_t s = ctx->stream;
  SNARKV_TRY(run.open(S));
  std::vector<const void*> d_s(S), d_p(S, run.d_srs);
  std::vector<size_t> ns(S, n);
  for (size_t i = 0; i < S; ++i) {
    d_s[i] = run.d_quot + 32 * n * i;
    SNARKV_TRY(run.set_quotient(i, run.d_quot + 32 * n * i));
  }
  SNARKV_TRY(launch_msm_pippenger_many(ctx, S, d_s.data(), d_p.data(), ns.data(), 0, run.blk + run.var_ws, false));
  std::vector<uint8_t> ws(64 * S);
  uint32_t first_bad = kNone;
  SNARKV_HIP(hipMemcpyAsync(ws.data(), run.blk + run.var_ws, 64 * S, hipMemcpyDeviceToHost, s));
  SNARKV_HIP(hipMemcpyAsync(&first_bad, run.status(), 4, hipMemcpyDeviceToHost, s));
  SNARKV_HIP(hipStreamSynchronize(s));  // the only one
  run.bufs.drained = true;
  if (first_bad != kNone) return run.refuse_bad_set(first_bad);
  memcpy(ws_out64, ws.data(), 64 * S);
  return SNARKV_OK;
}

int bdfg21_create_proof(snarkv_ctx* ctx, const KzgArgs& a, snarkv_kzg_challenge_fn draw_z_prime, void* user, uint8_t* w_out64,
                        uint8_t* z_prime_out32, uint8_t* w_prime_out64) {
  SNARKV_TRY(check_common(ctx, a));
  if (!a.gamma32 || !draw_z_prime || !w_out64 || !z_prime_out32 || !w_prime_out64) {
    set_last_error("%s: a null argument", a.who);
    return SNARKV_ERR_ARG;
  }
  SNARKV_TRY(check_canonical(ctx, a));
  KzgRun run(ctx, a);
  size_t bad_set = 0;
  int what = kzg_plan_build(a.mos, a.q_poly, a.q_shift32, a.q_eval32, a.n_queries, a.n, a.z32, a.c32, &run.plan, &bad_set);
  if (what != kOk) return refuse_plan(a.who, what, bad_set);
  const size_t S = run.plan.sets.size(), n = a.n;
  SNARKV_HIP(hipSetDevice(ctx->device));
  SNARKV_WIRE_FORM(ctx);
  hipStream_t s = ctx->stream;
  SNARKV_TRY(run.open(2));  // h, and one quotient at a time
  uint8_t *d_h = run.d_quot, *d_f = run.d_quot + 32 * n;
  // ---- h = sum gamma^i (q_i - r_i) / Z_i, W = commit(h) ---------------------------------------------------------------------
  SNARKV_TRY(run.set_quotient(0, d_h));  // gamma^0
  for (size_t i = 1; i < S; ++i) {
    SNARKV_TRY(run.set_quotient(i, d_f));
    SNARKV_TRY(run.axpy_sub(d_h, d_f, run.blk + run.var_g + 32 * i, nullptr, 0));
  }
  SNARKV_TRY(launch_msm_pippenger_auto(ctx, d_h, run.d_srs, n, 0, run.blk + KB_OUT, false));
  uint8_t w64[64], zp[32];
  uint32_t first_bad = kNone;
  SNARKV_HIP(hipMemcpyAsync(w64, run.blk + KB_OUT, 64, hipMemcpyDeviceToHost, s));
  SNARKV_HIP(hipMemcpyAsync(&first_bad, run.status(), 4, hipMemcpyDeviceToHost, s));
  SNARKV_HIP(hipStreamSynchronize(s));  // 1 of 2
  if (first_bad != kNone) return run.refuse_bad_set(first_bad);
  // ---- the caller's transcript: W in, z' out -------------------------------------------------------------------------------
  if (draw_z_prime(user, w64, zp) != 0) {
    set_last_error("%s: draw_z_prime failed", a.who);
    return SNARKV_ERR_ARG;
  }
  if ((ctx->flags & SNARKV_FLAG_VALIDATE) && !below_r(zp)) {
    set_last_error("%s: z' is not canonical", a.who);
    return SNARKV_ERR_ENCODING;
  }
  KzgPlanL pl;
  what = kzg_plan_finish(run.plan, a.gamma32, zp, &pl, &bad_set);
  if (what != kOk) return refuse_plan(a.who, what, bad_set);
  // ---- L = sum scalars polys[..] - Z_1(z') h - constant, W' = commit(L / (X - z')) ------------------------------------------
  uint8_t small[96];
  h_store(small, h_sub(fr29_zero(), h_load(pl.z1)));
  memcpy(small + 32, pl.constant, 32);
  memcpy(small + 64, zp, 32);
  SNARKV_HIP(hipMemcpyAsync(run.blk + KB_SCALAR, small, 96, hipMemcpyHostToDevice, s));
  uint8_t* d_l = run.d_t;
  SNARKV_TRY(poly_enqueue_lincomb(ctx, run.d_polys, n, pl.idx.data(), pl.scalars.data(), pl.idx.size(), d_l));
  SNARKV_TRY(run.axpy_sub(d_l, d_h, run.blk + KB_SCALAR, run.blk + KB_SUB, 1));
  SNARKV_TRY(run.divide(d_l, run.blk + KB_ZP, run.blk + KB_REM, 1, 0, run.status() + 1, d_f));
  SNARKV_TRY(launch_msm_pippenger_auto(ctx, d_f, run.d_srs, n, 0, run.blk + KB_OUT + 64, false));
  uint8_t wp64[64];
  SNARKV_HIP(hipMemcpyAsync(wp64, run.blk + KB_OUT + 64, 64, hipMemcpyDeviceToHost, s));
  SNARKV_HIP(hipMemcpyAsync(&first_bad, run.status() + 1, 4, hipMemcpyDeviceToHost, s));
  SNARKV_HIP(hipStreamSynchronize(s));  // 2 of 2
  run.bufs.drained = true;
  if (first_bad != kNone) {
    set_last_error("%s: internal error: L / (X - z') leaves a remainder", a.who);
    return SNARKV_ERR_DEVICE;
  }
  memcpy(w_out64, w64, 64);
  memcpy(z_prime_out32, zp, 32);
  memcpy(w_prime_out64, wp64, 64);
  return SNARKV_OK;
}

}  // namespace
}  // namespace snarkv

using namespace snarkv;

extern "C" {

int snarkv_kzg_multiopen_sets(int mos, const uint32_t* q_poly, const uint8_t* q_shift32, size_t n_queries, size_t* n_sets) {
  if (!n_sets || (n_queries && (!q_poly || !q_shift32))) return SNARKV_ERR_ARG;
  std::vector<MultiopenSet> sets;
  if (kzgplan::kzg_plan_sets(mos, q_poly, q_shift32, n_queries, &sets) != kzgplan::kOk) return SNARKV_ERR_ARG;
  *n_sets = sets.size();
  return SNARKV_OK;
}

int snarkv_kzg_gwc19_create_proof(snarkv_ctx* ctx, const uint8_t* srs64, const uint8_t* polys32, size_t n, size_t n_polys,
                                  const uint8_t z32[32], const uint32_t* q_poly, const uint8_t* q_shift32,
                                  const uint8_t* q_eval32, size_t n_queries, const uint8_t v32[32], uint8_t* ws_out64,
                                  size_t ws_cap, size_t* n_sets_out) {
  const KzgArgs a = {"kzg_gwc19_create_proof", SNARKV_KZG_MOS_GWC19, srs64, polys32, false, n, n_polys, n_queries, z32, q_shift32,
                     q_eval32, v32, nullptr, q_poly};
  return gwc19_create_proof(ctx, a, ws_out64, ws_cap, n_sets_out);
}

int snarkv_kzg_gwc19_create_proof_dev(snarkv_ctx* ctx, const void* d_srs64, const void* d_polys32, size_t n, size_t n_polys,
                                      const uint8_t z32[32], const uint32_t* q_poly, const uint8_t* q_shift32,
                                      const uint8_t* q_eval32, size_t n_queries, const uint8_t v32[32], uint8_t* ws_out64,
                                      size_t ws_cap, size_t* n_sets_out) {
  const KzgArgs a = {"kzg_gwc19_create_proof", SNARKV_KZG_MOS_GWC19, d_srs64, d_polys32, true, n, n_polys, n_queries, z32, q_shift32,
                     q_eval32, v32, nullptr, q_poly};
  return gwc19_create_proof(ctx, a, ws_out64, ws_cap, n_sets_out);
}

int snarkv_kzg_bdfg21_create_proof(snarkv_ctx* ctx, const uint8_t* srs64, const uint8_t* polys32, size_t n, size_t n_polys,
                                   const uint8_t z32[32], const uint32_t* q_poly, const uint8_t* q_shift32,
                                   const uint8_t* q_eval32, size_t n_queries, const uint8_t mu32[32],
                                   const uint8_t gamma32[32], snarkv_kzg_challenge_fn draw_z_prime, void* user,
                                   uint8_t w_out64[64], uint8_t z_prime_out32[32], uint8_t w_prime_out64[64]) {
  const KzgArgs a = {"kzg_bdfg21_create_proof", SNARKV_KZG_MOS_BDFG21, srs64, polys32, false, n, n_polys, n_queries, z32, q_shift32,
                     q_eval32, mu32, gamma32, q_poly};
  return bdfg21_create_proof(ctx, a, draw_z_prime, user, w_out64, z_prime_out32, w_prime_out64);
}

int snarkv_kzg_bdfg21_create_proof_dev(snarkv_ctx* ctx, const void* d_srs64, const void* d_polys32, size_t n, size_t n_polys,
                                       const uint8_t z32[32], const uint32_t* q_poly, const uint8_t* q_shift32,
                                       const uint8_t* q_eval32, size_t n_queries, const uint8_t mu32[32],
                                       const uint8_t gamma32[32], snarkv_kzg_challenge_fn draw_z_prime, void* user,
                                       uint8_t w_out64[64], uint8_t z_prime_out32[32], uint8_t w_prime_out64[64]) {
  const KzgArgs a = {"kzg_bdfg21_create_proof", SNARKV_KZG_MOS_BDFG21, d_srs64, d_polys32, true, n, n_polys, n_queries, z32,
                     q_shift32, q_eval32, mu32, gamma32, q_poly};
  return bdfg21_create_proof(ctx, a, draw_z_prime, user, w_out64, z_prime_out32, w_prime_out64);
}

}  // extern "C"
