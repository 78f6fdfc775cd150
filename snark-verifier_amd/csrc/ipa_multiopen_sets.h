// The query sets of the Bgh19 multi-open scheme (reference snark-verifier/src/pcs/ipa/multiopen/bgh19.rs:155-215, the rule of
// bdfg21.rs:121-171; oracle/kzg.py::bdfg21_query_sets): per polynomial the distinct shifts in first-seen order, then the
// polynomials whose shift SETS are equal share a set, which keeps the shift order of its first polynomial; the evaluations of
// the others are re-ordered to it.  Plain host C++ over the call's three parallel arrays; shifts and evaluations are named by
// the index of the query that carries them.  Included by ipa_multiopen.hip and by tests/hosttest/hosttest_poly.cpp.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>
#include <vector>

namespace snarkv {

struct MultiopenSet {
  std::vector<size_t> shifts;              // per shift: the first query that carries it
  std::vector<uint32_t> polys;             // in the order they joined
  std::vector<std::vector<size_t>> evals;  // per polynomial, per shift of the set: the query whose evaluation it is
};

inline std::vector<MultiopenSet> multiopen_query_sets(const uint32_t* q_poly, const uint8_t* q_shift32, size_t n_queries) {
  auto same = [&](size_t a, size_t b) { return memcmp(q_shift32 + 32 * a, q_shift32 + 32 * b, 32) == 0; };
  struct PolyShifts {
    uint32_t poly;
    std::vector<size_t> queries;  // one per distinct shift, first seen
  };
  std::vector<PolyShifts> per_poly;
  for (size_t q = 0; q < n_queries; ++q) {
    PolyShifts* ent = nullptr;
    for (auto& e : per_poly)
      if (e.poly == q_poly[q]) ent = &e;
    if (!ent) {
      per_poly.push_back({q_poly[q], {}});
      ent = &per_poly.back();
    }
    bool seen = false;
    for (size_t o : ent->queries) seen = seen || same(o, q);
    if (!seen) ent->queries.push_back(q);  // a repeated (polynomial, shift) keeps its first evaluation
  }
  std::vector<MultiopenSet> sets;
  for (const auto& e : per_poly) {
    MultiopenSet* home = nullptr;
    std::vector<size_t> order;  // per shift of the set: which of e's queries
    for (auto& st : sets) {
      if (st.shifts.size() != e.queries.size()) continue;
      order.clear();
      for (size_t s : st.shifts)
        for (size_t q : e.queries)
          if (same(s, q)) order.push_back(q);
      if (order.size() == st.shifts.size()) {  // shifts are distinct on both sides: equal sets
        home = &st;
        break;
      }
    }
    if (!home) {
      sets.push_back({e.queries, {}, {}});
      home = &sets.back();
      order = e.queries;
    }
    home->polys.push_back(e.poly);
    home->evals.push_back(order);
  }
  return sets;
}

}  // namespace snarkv
