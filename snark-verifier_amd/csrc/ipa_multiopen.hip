// The Bgh19 multi-open prover in one call (include/snarkv_ipa_multiopen.h), step by step as oracle/ipa.py::bgh19_create_proof:
//   host    grouping (ipa_multiopen_sets.h), x_1, x_2, per set the blind, the points x shift and the interpolation r of the
//           combined evaluations -- a handful of scalars each
//   device  per set  q = sum x_1^j polys[..]              poly_enqueue_lincomb
//                    f_i = (q - r) / prod (X - point)       k_mo_sub_low + poly_enqueue_div_linear per point, ping-pong;
//                                                           a remainder marks the set in the status word (k_mo_check_rem)
//           f = sum x_2^j f_i, commit(f, f_blind)           poly_enqueue_lincomb + ipa_enqueue_commit     -> sync 1: f, status
//   host    writes f, squeezes x_3
//   device  q_i(x_3), f(x_3)                                poly_enqueue_eval                              -> sync 2: S + 1 scalars
//   host    writes the q_i(x_3), squeezes x_4, forms omega and p(x_3)'s correction
//   device  p = x_4^S f + sum x_4^(S-i) q_i, p[0] -= ...    poly_enqueue_lincomb + k_mo_sub_low
//           the blinded opening of p at x_3 (ipa_opening.hip) in `TranscriptOrder::Bgh19`: s, alpha, xi_0 before the k
//           rounds, c, omega', U after them, where `Ipa::create_proof` writes omega' before xi_0 and U before c
//                                                                                                         -> sync 3: the proof
#include <string.h>
#include <algorithm>
#include <vector>
#include "fr_host.h"
#include "ipa_multiopen_sets.h"
#include "ipa_opening.hpp"
#include "poly.hpp"
#include "../../include/snarkv_ipa_multiopen.h"

namespace snarkv {

// the variable part of the call's device block (ipa_opening.hpp), staged by the host: points | remainders | r | evaluations
constexpr size_t MO_VAR = OP_BYTES;

// poly[j] -= sub[j], j < m
__global__ void __launch_bounds__(64) k_mo_sub_low(uint32_t* __restrict__ poly, const uint32_t* __restrict__ sub, uint32_t m) {
#pragma unroll 1
  for (uint32_t j = threadIdx.x; j < m; j += 64) {
    const Fr29 a = ld_fr(poly + 8 * (size_t)j), b = ld_fr(sub + 8 * (size_t)j);
    Fr29 d;  // (-r/2, 3r/2) minus the same: within fr29_to_canonical's 8 r
#pragma unroll
    for (int i = 0; i < 9; ++i) d.v[i] = a.v[i] - b.v[i];
    st_fr(poly + 8 * (size_t)j, d);
  }
}

// a remainder (canonical) that is not zero marks its set; the pipeline runs on
__global__ void __launch_bounds__(64) k_mo_check_rem(const uint32_t* __restrict__ rem, uint32_t set, uint32_t* __restrict__ first_bad) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  uint32_t any = 0;
  for (int w = 0; w < 8; ++w) any |= rem[w];
  if (any) atomicMin(first_bad, set);
}

namespace {

// ---- the host's few scalars: fr_host.h; a challenge comes from the transcript -----------------------------------------------
Fr29 h_squeeze(Blake2bState& st, uint8_t* canon32_or_null) {
  uint32_t w[8];
  const Fr29 c = h_red(tr_squeeze(st, w));
  if (canon32_or_null) memcpy(canon32_or_null, w, 32);
  return c;
}

struct MoArgs {
  const uint8_t *h64, *s64, *blinds32, *x32, *q_shift32, *q_eval32, *f_blind32, *omega_bar32, *absorbed;
  const uint32_t* q_poly;
  const void *polys, *pbar;
  bool on_device;
  size_t n, n_polys, n_queries, absorbed_len;
};

// what the host works out per set before any device work
struct SetPlan {
  std::vector<uint32_t> idx;     // the polynomials, reversed: the term of x_1^j
  std::vector<uint8_t> scalars;  // x_1^j, canonical
  Fr29 blind;
  size_t first_point;            // where its points, remainders and r lie in the variable part
  size_t m;
};

const char kWho[] = "ipa_multiopen_create_proof";

int multiopen_run(snarkv_ctx* ctx, const snarkv_ipa_dk* dk, const MoArgs& a, const std::vector<MultiopenSet>& sets, size_t need,
                  uint8_t* proof_out, uint8_t* xi_out32, uint8_t* u_out64) {
  const size_t n = a.n, S = sets.size();
  const bool validate = (ctx->flags & SNARKV_FLAG_VALIDATE) != 0;
  hipStream_t s = ctx->stream;
  SNARKV_WIRE_FORM(ctx);

  // ---- host: x_1, x_2 and the plan of every set ---------------------------------------------------------------------------
  Blake2bState ts;
  tr_init(ts);
  b2b_update(ts, a.absorbed, a.absorbed_len);
  const Fr29 x1 = h_squeeze(ts, nullptr), x2 = h_squeeze(ts, nullptr);
  const Fr29 x = h_load(a.x32);
  size_t total_points = 0, most_polys = 0;
  for (const MultiopenSet& st : sets) {
    total_points += st.shifts.size();
    most_polys = std::max(most_polys, st.polys.size());
    if (st.shifts.size() > n) {
      set_last_error("ipa_multiopen_create_proof: a polynomial is queried at %zu points, it has %zu coefficients", st.shifts.size(), n);
      return SNARKV_ERR_ARG;
    }
  }
  // the variable part of the device buffer: points | remainders | r | evaluations at x_3
  const size_t var_pts = MO_VAR, var_rem = var_pts + 32 * total_points, var_r = var_rem + 32 * total_points,
               var_ev = var_r + 32 * total_points, mo_bytes = var_ev + 32 * (S + 1);
  std::vector<uint8_t> stage(mo_bytes, 0);
  const std::vector<Fr29> px1 = h_powers(x1, most_polys);
  std::vector<SetPlan> plan(S);
  size_t at = 0;
  for (size_t i = 0; i < S; ++i) {
    const MultiopenSet& st = sets[i];
    SetPlan& pl = plan[i];
    const size_t np = st.polys.size(), m = st.shifts.size();
    pl.m = m;
    pl.first_point = at;
    pl.blind = fr29_zero();
    pl.scalars.resize(32 * np);
    std::vector<Fr29> pts(m), vals(m, fr29_zero()), r;
    for (size_t t = 0; t < m; ++t) pts[t] = h_mul(x, h_load(a.q_shift32 + 32 * st.shifts[t]));
    for (size_t j = 0; j < np; ++j) {  // QuerySet::msm order: polys reversed against ascending powers of x_1
      const size_t which = np - 1 - j;
      pl.idx.push_back(st.polys[which]);
      h_store(&pl.scalars[32 * j], px1[j]);
      pl.blind = h_add(pl.blind, h_mul(px1[j], h_load(a.blinds32 + 32 * (size_t)st.polys[which])));
      for (size_t t = 0; t < m; ++t) vals[t] = h_add(vals[t], h_mul(px1[j], h_load(a.q_eval32 + 32 * st.evals[which][t])));
    }
    if (!h_interpolate(pts, vals, r)) {
      set_last_error("ipa_multiopen_create_proof: two points of query set %zu coincide", i);
      return SNARKV_ERR_ARG;
    }
    for (size_t t = 0; t < m; ++t) {
      h_store(&stage[var_pts + 32 * (at + t)], pts[t]);
      h_store(&stage[var_r + 32 * (at + t)], r[t]);
    }
    at += m;
  }
  const uint32_t none = 0xffffffffu, off0n[2] = {0, (uint32_t)n};
  memcpy(&stage[OP_STATUS + 4], &none, 4);
  stage[OP_SC2F] = 1;
  memcpy(&stage[OP_SC2F + 32], a.f_blind32, 32);
  opening_stage_blinding(stage.data(), a.omega_bar32, a.s64);
  memcpy(&stage[OP_OFF0N], off0n, sizeof(off0n));

  // ---- device buffers: the polynomials (host form), q_1..q_S | f, f_1..f_S, two work polynomials, p_bar ------------------
  Buffers bufs(s);
  void *d_mo_, *d_polys_ = nullptr, *d_q_, *d_f_, *d_t_, *d_pbar_;
  SNARKV_TRY(bufs.get(&d_mo_, mo_bytes));
  if (!a.on_device) SNARKV_TRY(bufs.get(&d_polys_, 32 * n * a.n_polys));
  SNARKV_TRY(bufs.get(&d_q_, 32 * n * (S + 1)));
  SNARKV_TRY(bufs.get(&d_f_, 32 * n * S));
  SNARKV_TRY(bufs.get(&d_t_, 32 * n * 2));
  SNARKV_TRY(bufs.get(&d_pbar_, 32 * n));
  uint8_t *mo = (uint8_t*)d_mo_, *d_q = (uint8_t*)d_q_, *d_f = (uint8_t*)d_f_, *d_t = (uint8_t*)d_t_, *d_pbar = (uint8_t*)d_pbar_;
  const uint8_t* d_polys = a.on_device ? (const uint8_t*)a.polys : (const uint8_t*)d_polys_;
  uint8_t* d_fpoly = d_q + 32 * n * S;
  uint32_t* status = (uint32_t*)(mo + OP_STATUS);
  SNARKV_HIP(hipMemcpyAsync(mo, stage.data(), OP_STAGED, hipMemcpyHostToDevice, s));
  SNARKV_HIP(hipMemcpyAsync(mo + MO_VAR, stage.data() + MO_VAR, mo_bytes - MO_VAR, hipMemcpyHostToDevice, s));
  if (!a.on_device) SNARKV_HIP(hipMemcpyAsync(d_polys_, a.polys, 32 * n * a.n_polys, hipMemcpyHostToDevice, s));
  if (validate) {
    const size_t step = (size_t)1 << 30, total = n * a.n_polys;
    int bad = 0;
    for (size_t i = 0; i < total && !bad; i += step)
      SNARKV_TRY(count_bad(ctx, d_polys + 32 * i, std::min(step, total - i), (int*)(mo + OP_DELTA), &bad));
    if (bad) {
      set_last_error("ipa_multiopen_create_proof: %d coefficients of the polynomials are not canonical", bad);
      return SNARKV_ERR_ENCODING;
    }
  }
  SNARKV_TRY(opening_upload_pbar(ctx, kWho, d_pbar, a.pbar, a.on_device, n, (int*)(mo + OP_DELTA)));

  // ---- per set: q, then f_i = (q - r) / prod (X - point) ------------------------------------------------------------------
  for (size_t i = 0; i < S; ++i) {
    const SetPlan& pl = plan[i];
    uint8_t* q = d_q + 32 * n * i;
    SNARKV_TRY(poly_enqueue_lincomb(ctx, d_polys, n, pl.idx.data(), pl.scalars.data(), pl.idx.size(), q));
    SNARKV_HIP(hipMemcpyAsync(d_t, q, 32 * n, hipMemcpyDeviceToDevice, s));
    hipLaunchKernelGGL(k_mo_sub_low, dim3(1), dim3(64), 0, s, (uint32_t*)d_t, (const uint32_t*)(mo + var_r + 32 * pl.first_point),
                       (uint32_t)pl.m);
    SNARKV_HIP(hipGetLastError());
    uint8_t* src = d_t;
    size_t len = n;
    for (size_t t = 0; t < pl.m; ++t) {
      uint8_t* dst = t + 1 == pl.m ? d_f + 32 * n * i : (src == d_t ? d_t + 32 * n : d_t);
      uint8_t* rem = mo + var_rem + 32 * (pl.first_point + t);
      SNARKV_TRY(poly_enqueue_div_linear(ctx, src, len, mo + var_pts + 32 * (pl.first_point + t), dst, rem));
      len -= 1;
      SNARKV_HIP(hipMemsetAsync(dst + 32 * len, 0, 32 * (n - len), s));  // the quotient has `len` coefficients, f_i has n
      hipLaunchKernelGGL(k_mo_check_rem, dim3(1), dim3(64), 0, s, (const uint32_t*)rem, (uint32_t)i, status + 1);
      SNARKV_HIP(hipGetLastError());
      src = dst;
    }
  }
  // ---- f = sum x_2^j f_(S-1-j), its commitment ---------------------------------------------------------------------------
  {
    const std::vector<Fr29> px2 = h_powers(x2, S);
    std::vector<uint32_t> idx(S);
    std::vector<uint8_t> sc(32 * S);
    for (size_t j = 0; j < S; ++j) {
      idx[j] = (uint32_t)(S - 1 - j);
      h_store(&sc[32 * j], px2[j]);
    }
    SNARKV_TRY(poly_enqueue_lincomb(ctx, d_f, n, idx.data(), sc.data(), S, d_fpoly));
  }
  SNARKV_TRY(ipa_enqueue_commit(ctx, dk->d_points, d_fpoly, n, mo + OP_OFF0N, mo + OP_PTS2, mo + OP_SC2F, mo + OP_OFF02,
                                mo + OP_BLIND, true));
  uint8_t f64[64];
  uint32_t first_bad = none;
  SNARKV_HIP(hipMemcpyAsync(f64, mo + OP_BLIND, 64, hipMemcpyDeviceToHost, s));
  SNARKV_HIP(hipMemcpyAsync(&first_bad, status + 1, 4, hipMemcpyDeviceToHost, s));
  SNARKV_HIP(hipStreamSynchronize(s));  // 1 of 3
  if (first_bad != none) {
    set_last_error("ipa_multiopen_create_proof: evaluation does not match the polynomial (query set %u)", first_bad);
    return SNARKV_ERR_ARG;
  }
  std::vector<uint8_t> proof(need);
  if (!tr_common_point(ts, f64, f64 + 32)) return opening_infinity_error(kWho, "f");
  tr_compress_point(f64, f64 + 32, &proof[0]);
  uint8_t x3b[32];
  (void)h_squeeze(ts, x3b);
  // ---- q_i(x_3) and f(x_3) -------------------------------------------------------------------------------------------------
  SNARKV_HIP(hipMemcpyAsync(mo + OP_POINT, x3b, 32, hipMemcpyHostToDevice, s));
  for (size_t i = 0; i <= S; ++i) SNARKV_TRY(poly_enqueue_eval(ctx, d_q + 32 * n * i, n, mo + OP_POINT, mo + var_ev + 32 * i));
  std::vector<uint8_t> evb(32 * (S + 1));
  SNARKV_HIP(hipMemcpyAsync(evb.data(), mo + var_ev, evb.size(), hipMemcpyDeviceToHost, s));
  SNARKV_HIP(hipStreamSynchronize(s));  // 2 of 3
  for (size_t i = 0; i < S; ++i) {
    tr_common_scalar(ts, &evb[32 * i]);
    memcpy(&proof[32 + 32 * i], &evb[32 * i], 32);
  }
  const Fr29 x4 = h_squeeze(ts, nullptr);
  // ---- p = x_4^S f + sum x_4^(S-1-i) q_i, lowered so that p(x_3) = 0; omega the same combination of the blinds -----------
  uint8_t* d_p = d_t;
  {
    const std::vector<Fr29> px4 = h_powers(x4, S + 1);
    std::vector<uint32_t> idx(S + 1);
    std::vector<uint8_t> sc(32 * (S + 1));
    idx[0] = (uint32_t)S;
    h_store(&sc[0], px4[S]);
    Fr29 omega = h_mul(h_load(a.f_blind32), px4[S]), delta = h_mul(h_load(&evb[32 * S]), px4[S]);
    for (size_t i = 0; i < S; ++i) {
      idx[1 + i] = (uint32_t)i;
      h_store(&sc[32 * (1 + i)], px4[S - 1 - i]);
      omega = h_add(omega, h_mul(plan[i].blind, px4[S - 1 - i]));
      delta = h_add(delta, h_mul(h_load(&evb[32 * i]), px4[S - 1 - i]));
    }
    SNARKV_TRY(poly_enqueue_lincomb(ctx, d_q, n, idx.data(), sc.data(), S + 1, d_p));
    uint8_t small[96];
    h_store(small, delta);
    h_store(small + 32, omega);
    memcpy(small + 64, a.omega_bar32, 32);
    SNARKV_HIP(hipMemcpyAsync(mo + OP_DELTA, small, 32, hipMemcpyHostToDevice, s));
    SNARKV_HIP(hipMemcpyAsync(mo + OP_OMEGA, small + 32, 64, hipMemcpyHostToDevice, s));
    SNARKV_HIP(hipMemcpyAsync(mo + OP_STATE, &ts, sizeof(ts), hipMemcpyHostToDevice, s));
    hipLaunchKernelGGL(k_mo_sub_low, dim3(1), dim3(64), 0, s, (uint32_t*)d_p, (const uint32_t*)(mo + OP_DELTA), 1u);
    SNARKV_HIP(hipGetLastError());
  }
  // ---- the zk opening of p at x_3, Bgh19's transcript order ----------------------------------------------------------------
  snarkv_ipa_prover* p = nullptr;
  SNARKV_TRY(session_open(ctx, dk, d_p, true, n, x3b, a.h64, nullptr, kWho, &p));
  SNARKV_TRY(opening_prove(p, mo, d_pbar, TranscriptOrder::Bgh19, kWho, "s", &proof[32 + 32 * S], xi_out32, u_out64));
  bufs.drained = true;
  memcpy(proof_out, proof.data(), need);
  return SNARKV_OK;
}

int multiopen_create_proof(snarkv_ctx* ctx, const snarkv_ipa_dk* dk, const MoArgs& a, uint8_t* proof_out, size_t proof_cap,
                           size_t* proof_len, uint8_t* xi_out32, uint8_t* u_out64) {
  if (!ctx || !dk || !a.h64 || !a.s64 || !a.polys || !a.blinds32 || !a.x32 || !a.q_poly || !a.q_shift32 || !a.q_eval32 ||
      !a.f_blind32 || !a.pbar || !a.omega_bar32 || !proof_out || !proof_len || !xi_out32 || !u_out64 ||
      (a.absorbed_len && !a.absorbed)) {
    set_last_error("ipa_multiopen_create_proof: a null argument (h and s are both required: the scheme is zero-knowledge)");
    return SNARKV_ERR_ARG;
  }
  *proof_len = 0;
  if (dk->device != ctx->device) return SNARKV_ERR_ARG;
  if (dk->first != 0 || dk->count != ((size_t)1 << dk->k) || dk->k < 1 || dk->k > 30) return SNARKV_ERR_LENGTH;
  if (a.n != dk->count) return SNARKV_ERR_LENGTH;
  if (a.n_polys == 0 || a.n_queries == 0) return SNARKV_ERR_EMPTY;
  if (a.on_device && ((uintptr_t)a.polys % 16 || (uintptr_t)a.pbar % 16)) return SNARKV_ERR_ARG;
  for (size_t i = 0; i < a.n_queries; ++i)
    if (a.q_poly[i] >= a.n_polys) {
      set_last_error("ipa_multiopen_create_proof: query %zu names polynomial %u of %zu", i, a.q_poly[i], a.n_polys);
      return SNARKV_ERR_ARG;
    }
  const std::vector<MultiopenSet> sets = multiopen_query_sets(a.q_poly, a.q_shift32, a.n_queries);
  const size_t need = 64 * (size_t)dk->k + 32 * sets.size() + 160;
  if (proof_cap < need) {
    *proof_len = need;
    set_last_error("ipa_multiopen_create_proof: the proof has %zu bytes, proof_cap is %zu", need, proof_cap);
    return SNARKV_ERR_LENGTH;
  }
  if (ctx->flags & SNARKV_FLAG_VALIDATE) {
    bool ok = host_canonical(a.x32) && host_canonical(a.f_blind32) && host_canonical(a.omega_bar32);
    for (size_t i = 0; ok && i < a.n_polys; ++i) ok = host_canonical(a.blinds32 + 32 * i);
    for (size_t i = 0; ok && i < a.n_queries; ++i) ok = host_canonical(a.q_shift32 + 32 * i) && host_canonical(a.q_eval32 + 32 * i);
    if (!ok) {
      set_last_error("ipa_multiopen_create_proof: x, a blind, a shift, an evaluation, f_blind or omega_bar is not canonical");
      return SNARKV_ERR_ENCODING;
    }
  }
  SNARKV_HIP(hipSetDevice(ctx->device));
  SNARKV_TRY(multiopen_run(ctx, dk, a, sets, need, proof_out, xi_out32, u_out64));
  *proof_len = need;
  return SNARKV_OK;
}

}  // namespace
}  // namespace snarkv

using namespace snarkv;

extern "C" {

int SNARKV_API(ipa_multiopen_create_proof)(snarkv_ctx* ctx, const snarkv_ipa_dk* dk, const uint8_t h64[64], const uint8_t s64[64],
                                           const uint8_t* polys32, size_t n, size_t n_polys, const uint8_t* blinds32,
                                           const uint8_t x32[32], const uint32_t* q_poly, const uint8_t* q_shift32,
                                           const uint8_t* q_eval32, size_t n_queries, const uint8_t f_blind32[32],
                                           const uint8_t* pbar32, const uint8_t omega_bar32[32], const uint8_t* absorbed,
                                           size_t absorbed_len, uint8_t* proof_out, size_t proof_cap, size_t* proof_len,
                                           uint8_t* xi_out32, uint8_t u_out64[64]) {
  const MoArgs a = {h64, s64, blinds32, x32, q_shift32, q_eval32, f_blind32, omega_bar32, absorbed, q_poly, polys32, pbar32, false,
                    n, n_polys, n_queries, absorbed_len};
  return multiopen_create_proof(ctx, dk, a, proof_out, proof_cap, proof_len, xi_out32, u_out64);
}

int SNARKV_API(ipa_multiopen_create_proof_dev)(snarkv_ctx* ctx, const snarkv_ipa_dk* dk, const uint8_t h64[64],
                                               const uint8_t s64[64], const void* d_polys32, size_t n, size_t n_polys,
                                               const uint8_t* blinds32, const uint8_t x32[32], const uint32_t* q_poly,
                                               const uint8_t* q_shift32, const uint8_t* q_eval32, size_t n_queries,
                                               const uint8_t f_blind32[32], const void* d_pbar32, const uint8_t omega_bar32[32],
                                               const uint8_t* absorbed, size_t absorbed_len, uint8_t* proof_out, size_t proof_cap,
                                               size_t* proof_len, uint8_t* xi_out32, uint8_t u_out64[64]) {
  const MoArgs a = {h64, s64, blinds32, x32, q_shift32, q_eval32, f_blind32, omega_bar32, absorbed, q_poly, d_polys32, d_pbar32, true,
                    n, n_polys, n_queries, absorbed_len};
  return multiopen_create_proof(ctx, dk, a, proof_out, proof_cap, proof_len, xi_out32, u_out64);
}

}  // extern "C"
