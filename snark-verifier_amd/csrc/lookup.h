// The lookup argument's sort and permuted columns (include/snarkv_lookup.h): the key and its comparison, the merge-path
// partition, the rank of an element in the in-tile merge, the geometry of a merge pass, the flags of halo2's
// permute_expression_pair and the arithmetic of the count scans.  Same source for the kernels of lookup.hip and for the
// host (tests/hosttest/hosttest_lookup.cpp, with tiles and blocks of 2, 3, 4 and 8), as poly_prod.h.
//
// Keys.  A key is the canonical integer of an element, 8 words, least significant first.  The order is numeric: lk_less is one
// borrow chain over the eight words with no early exit, so every comparison costs the same whatever the data.  Equal keys
// are identical words (lk_canon reduces every input on its way in), so no merge here needs to be stable.
//
// The tie rule.  Where a run `a` (the left one, earlier in memory) is merged with a run `b`, an element of `a` comes before
// an equal element of `b`: "a first".  Every place that decides an order states it through the same two tests:
//   lk_merge_path   a[i] is among the first `diag` merged elements iff !(b[diag - 1 - i] < a[i])
//   lk_take_a       the serial merge of a lane takes from a iff !(b < a)
//   lk_tile_dest    an element of a goes behind the elements of b that are < it, one of b behind those of a that are <= it
// so the chunk borders of a merge pass and the lanes inside a chunk cut the same merged sequence.
//
// A sorter of a generic sequence takes a "getter": any object g with g(i) -> LkKey.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include "fr29.h"
#include "poly_prod.h"

namespace snarkv {

struct LkKey {
  uint32_t w[8];
};

// a < b as integers: the borrow out of a - b
SNARKV_HD bool lk_less(const LkKey& a, const LkKey& b) {
  uint32_t borrow = 0;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const uint64_t t = (uint64_t)a.w[i] - (uint64_t)b.w[i] - (uint64_t)borrow;
    borrow = (uint32_t)(t >> 63);
  }
  return borrow != 0;
}
SNARKV_HD bool lk_equal(const LkKey& a, const LkKey& b) {
  uint32_t d = 0;
#pragma unroll
  for (int i = 0; i < 8; ++i) d |= a.w[i] ^ b.w[i];
  return d == 0;
}
// 8 words below 2^256 -> the canonical words of their residue: in and out through the Montgomery form, which takes any
// value below 2^256 < 8r (fr29.h)
SNARKV_HD LkKey lk_canon(const uint32_t w[8]) {
  LkKey k;
  fr29_to_canonical(fr29_from_canonical(w), k.w);
  return k;
}

// How many elements of x[lo, hi) (sorted) come before `key`: those < key, and with `ties` those == key as well.
template <class G>
SNARKV_HD uint32_t lk_count_before(const G& x, uint32_t lo, uint32_t hi, const LkKey& key, bool ties) {
  const uint32_t first = lo;
  while (lo < hi) {
    const uint32_t mid = lo + (hi - lo) / 2;
    const LkKey m = x(mid);
    if (ties ? !lk_less(key, m) : lk_less(m, key)) lo = mid + 1;
    else hi = mid;
  }
  return lo - first;
}

// The merge of the sorted runs a (na elements) and b (nb elements): how many of its first `diag` elements come from a.
// 0 <= diag <= na + nb.  The candidates i lie in [max(0, diag - nb), min(diag, na)], so a(mid) and b(diag - 1 - mid) exist.
template <class GA, class GB>
SNARKV_HD uint32_t lk_merge_path(const GA& a, uint32_t na, const GB& b, uint32_t nb, uint32_t diag) {
  uint32_t lo = diag > nb ? diag - nb : 0u, hi = diag < na ? diag : na;
  while (lo < hi) {
    const uint32_t mid = lo + (hi - lo) / 2;
    if (!lk_less(b(diag - 1u - mid), a(mid))) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}
// one step of a serial merge: does the next element come from a?
SNARKV_HD bool lk_take_a(bool has_a, bool has_b, const LkKey& ka, const LkKey& kb) { return has_a && (!has_b || !lk_less(kb, ka)); }

// The in-tile merge by ranks.  A tile of `len` elements consists of sorted runs of `run` elements (the last may be short);
// the runs are merged in pairs.  -> where the element `key` at position i goes: its pair's base, plus its index in its own
// run, plus the number of elements of the other run that come before it.
template <class G>
SNARKV_HD uint32_t lk_tile_dest(const G& x, uint32_t len, uint32_t run, uint32_t i, const LkKey& key) {
  const uint32_t base = i / (2u * run) * (2u * run);
  const uint32_t mid = base + run < len ? base + run : len, end = base + 2u * run < len ? base + 2u * run : len;
  if (i < mid) return i + lk_count_before(x, mid, end, key, false);
  return base + (i - mid) + lk_count_before(x, base, mid, key, true);
}

// A merge pass over n elements in sorted runs of `run` (a multiple of `chunk`): output chunk c is made of a = [a0, a0 + na)
// and b = [b0, b0 + nb) of the source, from the diagonal `diag` of their merge on.  nb = 0: the odd run at the end, carried
// over unchanged.  A chunk never spans two pairs because 2 run is a multiple of chunk.
struct LkMergeGeom {
  uint32_t a0, na, b0, nb, diag;
};
SNARKV_HD LkMergeGeom lk_merge_geom(uint32_t n, uint32_t run, uint32_t chunk, uint32_t c) {
  LkMergeGeom g;
  const uint32_t start = c * chunk, base = start / (2u * run) * (2u * run);
  const uint32_t mid = n - base > run ? base + run : n, end = n - base > 2u * run ? base + 2u * run : n;
  g.a0 = base, g.na = mid - base, g.b0 = mid, g.nb = end - mid, g.diag = start - base;
  return g;
}
// the merge passes a sort of n elements takes after its tiles are sorted
SNARKV_HD uint32_t lk_passes(uint32_t n, uint32_t tile) {
  uint32_t p = 0;
  for (uint64_t run = tile; run < n; run *= 2) ++p;
  return p;
}

// halo2's permute_expression_pair.  a = A' (the sorted input), s = the sorted table, both u elements.  The flags of index i:
//   kLkRepeated   row i of A' repeats the value of row i - 1: its table row is filled from the leftovers
//   kLkLeftover   element i of the sorted table is not taken by a first row: it is not the first of its value, or its value
//                 does not occur in A' (a binary search in A', only made for the first of a value)
constexpr uint32_t kLkRepeated = 1u, kLkLeftover = 2u;
template <class GA, class GS>
SNARKV_HD uint32_t lk_flags(const GA& a, const GS& s, uint32_t u, uint32_t i) {
  const LkKey ai = a(i), si = s(i);
  uint32_t f = 0;
  if (i > 0 && lk_equal(a(i - 1u), ai)) f |= kLkRepeated;
  bool used = false;
  if (i == 0 || !lk_equal(s(i - 1u), si)) {
    const uint32_t p = lk_count_before(a, 0u, u, si, false);
    used = p < u && lk_equal(a(p), si);
  }
  if (!used) f |= kLkLeftover;
  return f;
}
// The leftovers in order are halo2's remaining table values, ascending with multiplicity; halo2 pops its list of repeated
// rows, so the first leftover goes to the LAST repeated row: the repeated row with `rank` repeated rows before it, of
// `repeated` in all, takes leftover repeated - 1 - rank, which lies in [0, repeated) whatever the input.
SNARKV_HD uint32_t lk_leftover_of(uint32_t repeated, uint32_t rank) { return repeated - 1u - rank; }

// The counts that are scanned: repeated rows and leftovers, side by side.
struct LkCount {
  uint32_t rep, left;
};
SNARKV_HD LkCount lk_count_of(uint32_t flags) {
  LkCount c;
  c.rep = flags & kLkRepeated ? 1u : 0u, c.left = flags & kLkLeftover ? 1u : 0u;
  return c;
}
SNARKV_HD LkCount lk_add(const LkCount& a, const LkCount& b) {
  LkCount c;
  c.rep = a.rep + b.rep, c.left = a.left + b.left;
  return c;
}
struct LkAdd {  // as the step of poly_prod.h's wg_scan
  SNARKV_HD LkCount operator()(const LkCount& a, const LkCount& b) const { return lk_add(a, b); }
};
// status[0..3] from the totals: every distinct input value is one first row; each one the table holds uses up one table
// element, so the leftovers exceed the repeated rows by the number of distinct input values the table lacks
SNARKV_HD void lk_status(const LkCount& total, uint32_t u, uint32_t* status) {
  status[0] = total.left - total.rep;
  status[1] = u - total.rep;
  status[2] = 0;
  status[3] = 0;
}
// The additive scan has the level structure of poly_prod.h's scans: blocks of T lanes with E consecutive elements each
// (ProdBlock), bottom up the totals of the blocks, top down the exclusive prefix of a block plus its carry.
// the E counts of a lane -> their exclusive prefixes within the lane and the lane's total
template <uint32_t E>
SNARKV_HD void lk_lane_prefix(const LkCount* x, LkCount* p, LkCount& total) {
  LkCount acc;
  acc.rep = 0, acc.left = 0;
#pragma unroll
  for (uint32_t j = 0; j < E; ++j) {
    p[j] = acc;
    acc = lk_add(acc, x[j]);
  }
  total = acc;
}

}  // namespace snarkv
