// Host build of the blocked scan behind the polynomial division and evaluation (snark-verifier_amd/csrc/poly_scan.h, the
// SNARKV_HD source the device compiles), driven the way poly.hip drives it: per level the lanes of every block take the
// steps of phase 1 in lock-step from a copy of the previous step's values, the totals go one level up with the root a^B, and
// on the way down every block but the last takes its carry.  Values travel between the phases as canonical words, as between
// the kernels.  Block sizes 2, 3 and 4, chosen at run time.  Also the query-set grouping of the multi-open prover
// (csrc/ipa_multiopen_sets.h).  One library per curve (-DSNARKV_CURVE_PALLAS), built by snark-verifier_amd/build.py.
// Test infrastructure only.
#include <stdint.h>
#include <vector>
#include "../../snark-verifier_amd/csrc/ipa_multiopen_sets.h"
#include "../../snark-verifier_amd/csrc/poly_scan.h"

using namespace snarkv;

namespace {

typedef std::vector<uint32_t> Words;  // 8 per value

Fr29 load(const Words& w, size_t i) { return fr29_from_canonical(w.data() + 8 * i); }
void store(Words& w, size_t i, const Fr29& v) { fr29_to_canonical(v, w.data() + 8 * i); }

// phase 1 of one level: seq[i] <- s_i, the totals and a^B
template <uint32_t B>
void scan_blocks(Words& seq, uint32_t n, const Fr29& a, Words& totals, Fr29& a_pow_b) {
  typedef PolyScan<B> S;
  totals.assign(8 * (size_t)S::blocks(n), 0);
  for (uint32_t b = 0; b < S::blocks(n); ++b) {
    const uint32_t len = S::block_len(b, n);
    Fr29 s[B], prev[B];
    for (uint32_t t = 0; t < len; ++t) s[t] = load(seq, (size_t)b * B + t);
    Fr29 a_pow = a;
    for (uint32_t step = 0; step < S::steps(); ++step) {
      for (uint32_t t = 0; t < len; ++t) prev[t] = s[t];
      for (uint32_t t = 0; t < len; ++t)
        if (S::has_partner(t, step, len)) s[t] = poly_scan_step(prev[t], prev[t + S::distance(step)], a_pow, step);
      a_pow = fr29_mul(a_pow, a_pow);
    }
    for (uint32_t t = 0; t < len; ++t) store(seq, (size_t)b * B + t, s[t]);
    store(totals, b, s[0]);
  }
  Fr29 sq[32];
  sq[0] = a;
  for (int j = 1; j < 32; ++j) sq[j] = fr29_mul(sq[j - 1], sq[j - 1]);
  a_pow_b = poly_scan_pow(sq, B, 32);  // the device's B is a power of two: there the last square of the steps is a^B
}

// seq (n canonical values p_i) <- c_i
template <uint32_t B>
void scan(Words& seq, uint32_t n, const Fr29& a) {
  typedef PolyScan<B> S;
  Words totals;
  Fr29 a_b;
  scan_blocks<B>(seq, n, a, totals, a_b);
  if (S::blocks(n) == 1) return;
  scan<B>(totals, S::blocks(n), a_b);
  Fr29 sq[32];
  sq[0] = a;
  for (int j = 1; j < 32; ++j) sq[j] = fr29_mul(sq[j - 1], sq[j - 1]);
  for (uint32_t i = 0; i < n; ++i) {
    const uint32_t b = S::block_of(i);
    if (!S::has_carry(b, n)) continue;
    const Fr29 w = poly_scan_pow(sq, S::carry_exp(S::lane_of(i)), 32);
    store(seq, i, poly_scan_apply(load(seq, i), w, load(totals, S::carry_index(b))));
  }
}

// p(a) from the totals alone
template <uint32_t B>
void eval(Words& seq, uint32_t n, const Fr29& a, uint32_t* out) {
  Words totals;
  Fr29 a_b;
  scan_blocks<B>(seq, n, a, totals, a_b);
  if (PolyScan<B>::blocks(n) == 1) {
    for (int w = 0; w < 8; ++w) out[w] = totals[w];
    return;
  }
  eval<B>(totals, PolyScan<B>::blocks(n), a_b, out);
}

}  // namespace

extern "C" {

const char* hp_curve() {
#if defined(SNARKV_CURVE_PALLAS)
  return "pallas";
#else
  return "bn254";
#endif
}

// coeffs: n x 8 words, root: 8 words; quot: (n - 1) x 8 words, rem and value: 8 words each.  block in {2, 3, 4}; 0 otherwise.
int hp_div_linear(const uint32_t* coeffs, uint32_t n, const uint32_t* root, uint32_t block, uint32_t* quot, uint32_t* rem,
                  uint32_t* value) {
  if (n == 0 || block < 2 || block > 4) return 0;
  const Fr29 a = fr29_from_canonical(root);
  Words c(coeffs, coeffs + 8 * (size_t)n), e(c);
  if (block == 2) scan<2>(c, n, a), eval<2>(e, n, a, value);
  if (block == 3) scan<3>(c, n, a), eval<3>(e, n, a, value);
  if (block == 4) scan<4>(c, n, a), eval<4>(e, n, a, value);
  for (int w = 0; w < 8; ++w) rem[w] = c[w];
  for (size_t w = 8; w < c.size(); ++w) quot[w - 8] = c[w];
  return 1;
}

// The grouping as a flat list of u32: S, then per set: shifts m, polynomials np, m query indices (the shifts), np polynomial
// indices, np x m query indices (the evaluations).  Returns the words needed; writes at most `cap` of them.
size_t hp_query_sets(const uint32_t* q_poly, const uint8_t* q_shift32, size_t n_queries, uint32_t* out, size_t cap) {
  std::vector<uint32_t> flat;
  const std::vector<MultiopenSet> sets = multiopen_query_sets(q_poly, q_shift32, n_queries);
  flat.push_back((uint32_t)sets.size());
  for (const MultiopenSet& st : sets) {
    flat.push_back((uint32_t)st.shifts.size());
    flat.push_back((uint32_t)st.polys.size());
    for (size_t q : st.shifts) flat.push_back((uint32_t)q);
    for (uint32_t p : st.polys) flat.push_back(p);
    for (const auto& ev : st.evals)
      for (size_t q : ev) flat.push_back((uint32_t)q);
  }
  for (size_t i = 0; i < flat.size() && i < cap; ++i) out[i] = flat[i];
  return flat.size();
}

}  // extern "C"
