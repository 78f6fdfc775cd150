// The host-side plan of the two KZG multi-open provers (include/snarkv_kzg_multiopen.h, kzg_multiopen.hip): everything the
// host works out from the queries and the challenges -- a handful of scalars per set -- before and between the device's
// steps.  Host only and free of HIP types, so that the host compiles it alone (tests/hosttest/hosttest_kzg_open.cpp holds it
// against tests/kzg_multiopen_util.py number for number).
//
//   kzg_plan_sets     the query sets: Gwc19 by shift, first seen (gwc19.rs:142-160; a repeated (polynomial, shift) stays
//                     twice in its set, as in gwc19::query_sets); Bdfg21 by the rule of ipa_multiopen_sets.h
//   kzg_plan_build    per set: the polynomials with their scalars c^j (c = v or mu), the points z shift_t, and the
//                     coefficients of r, the interpolation of the c-combined evaluations (Gwc19: one point, r = sum v^i e_i)
//   kzg_plan_finish   Bdfg21 after z': L = sum scalars[j] polys[idx[j]] - z1 h - constant, with
//                     scalars = gamma^i (Z_1(z') / Z_i(z')) mu^j, constant = sum_i gamma^i (Z_1(z') / Z_i(z')) r_i(z'), z1 = Z_1(z')
// Scalars are Fr29 in the Montgomery domain on the way (fr_host.h); what the plan keeps is canonical bytes.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>
#include <vector>
#include "fr_host.h"
#include "ipa_multiopen_sets.h"

namespace snarkv {
namespace kzgplan {

enum { kGwc19 = 0, kBdfg21 = 1 };                       // SNARKV_KZG_MOS_*
enum { kOk = 0, kBadMos, kCoincide, kTooManyPoints, kZeroZ };  // what a step found; `*bad_set` names the set

// gwc19.rs:142-160 in the shape of MultiopenSet: one shift per set, a polynomial once per query that names it
inline std::vector<MultiopenSet> gwc19_query_sets(const uint32_t* q_poly, const uint8_t* q_shift32, size_t n_queries) {
  std::vector<MultiopenSet> sets;
  for (size_t q = 0; q < n_queries; ++q) {
    MultiopenSet* home = nullptr;
    for (auto& st : sets)
      if (!home && memcmp(q_shift32 + 32 * st.shifts[0], q_shift32 + 32 * q, 32) == 0) home = &st;
    if (!home) {
      sets.push_back({{q}, {}, {}});
      home = &sets.back();
    }
    home->polys.push_back(q_poly[q]);
    home->evals.push_back({q});
  }
  return sets;
}

inline int kzg_plan_sets(int mos, const uint32_t* q_poly, const uint8_t* q_shift32, size_t n_queries,
                         std::vector<MultiopenSet>* out) {
  if (mos == kGwc19) *out = gwc19_query_sets(q_poly, q_shift32, n_queries);
  else if (mos == kBdfg21) *out = multiopen_query_sets(q_poly, q_shift32, n_queries);
  else return kBadMos;
  return kOk;
}

struct KzgPlanSet {
  std::vector<uint32_t> idx;     // the polynomials in set order: the term of c^j
  std::vector<uint8_t> scalars;  // c^j, 32 bytes each
  std::vector<uint8_t> points;   // z shift_t, m x 32
  std::vector<uint8_t> r;        // the coefficients of r, m x 32
  size_t m() const { return points.size() / 32; }
};

struct KzgPlan {
  int mos;
  std::vector<KzgPlanSet> sets;
};

// what Bdfg21 forms after z'
struct KzgPlanL {
  std::vector<uint32_t> idx;     // over the original polynomials, sets in order
  std::vector<uint8_t> scalars;  // 32 bytes each
  uint8_t constant[32];
  uint8_t z1[32];
};

inline int kzg_plan_build(int mos, const uint32_t* q_poly, const uint8_t* q_shift32, const uint8_t* q_eval32, size_t n_queries,
                          size_t n, const uint8_t* z32, const uint8_t* c32, KzgPlan* plan, size_t* bad_set) {
  std::vector<MultiopenSet> sets;
  if (kzg_plan_sets(mos, q_poly, q_shift32, n_queries, &sets) != kOk) return kBadMos;
  plan->mos = mos;
  plan->sets.assign(sets.size(), KzgPlanSet());
  size_t most = 0;
  for (const MultiopenSet& st : sets) most = st.polys.size() > most ? st.polys.size() : most;
  const Fr29 z = h_load(z32);
  const std::vector<Fr29> pc = h_powers(h_load(c32), most);
  for (size_t i = 0; i < sets.size(); ++i) {
    const MultiopenSet& st = sets[i];
    KzgPlanSet& pl = plan->sets[i];
    const size_t np = st.polys.size(), m = st.shifts.size();
    *bad_set = i;
    if (m > n) return kTooManyPoints;
    std::vector<Fr29> pts(m), vals(m, fr29_zero()), r;
    for (size_t t = 0; t < m; ++t) pts[t] = h_mul(z, h_load(q_shift32 + 32 * st.shifts[t]));
    pl.idx.assign(st.polys.begin(), st.polys.end());
    pl.scalars.resize(32 * np);
    for (size_t j = 0; j < np; ++j) {
      h_store(&pl.scalars[32 * j], pc[j]);
      for (size_t t = 0; t < m; ++t) vals[t] = h_add(vals[t], h_mul(pc[j], h_load(q_eval32 + 32 * st.evals[j][t])));
    }
    if (!h_interpolate(pts, vals, r)) return kCoincide;
    pl.points.resize(32 * m);
    pl.r.resize(32 * m);
    for (size_t t = 0; t < m; ++t) {
      h_store(&pl.points[32 * t], pts[t]);
      h_store(&pl.r[32 * t], r[t]);
    }
  }
  return kOk;
}

inline int kzg_plan_finish(const KzgPlan& plan, const uint8_t* gamma32, const uint8_t* z_prime32, KzgPlanL* out, size_t* bad_set) {
  const size_t S = plan.sets.size();
  const Fr29 zp = h_load(z_prime32);
  const std::vector<Fr29> pg = h_powers(h_load(gamma32), S);
  out->idx.clear();
  out->scalars.clear();
  Fr29 z1 = fr29_one(), constant = fr29_zero();
  for (size_t i = 0; i < S; ++i) {
    const KzgPlanSet& st = plan.sets[i];
    const size_t m = st.m();
    Fr29 zi = fr29_one(), ri = fr29_zero();
    for (size_t t = 0; t < m; ++t) zi = h_mul(zi, h_sub(zp, h_load(&st.points[32 * t])));
    *bad_set = i;
    if (h_is_zero(zi)) return kZeroZ;
    for (size_t t = m; t-- > 0;) ri = h_add(h_mul(ri, zp), h_load(&st.r[32 * t]));  // Horner
    if (i == 0) z1 = zi;
    const Fr29 f = i == 0 ? pg[0] : h_mul(pg[i], h_mul(z1, h_inv(zi)));  // gamma^i Z_1(z') / Z_i(z')
    constant = h_add(constant, h_mul(f, ri));
    for (size_t j = 0; j < st.idx.size(); ++j) {
      out->idx.push_back(st.idx[j]);
      out->scalars.resize(out->scalars.size() + 32);
      h_store(&out->scalars[out->scalars.size() - 32], h_mul(f, h_load(&st.scalars[32 * j])));
    }
  }
  h_store(out->constant, constant);
  h_store(out->z1, z1);
  return kOk;
}

}  // namespace kzgplan
}  // namespace snarkv
