// Host build of the blocked product scans behind the grand product and the batch inversion
// (snark-verifier_amd/csrc/poly_prod.h, the SNARKV_HD source the device compiles), driven the way poly_prod.hip drives it:
// bottom up the totals of every level but the last, top down every block recomputes its prefixes (and suffixes) from what it
// reads, the lanes of a block taking the steps of the workgroup scan in lock-step from a copy of the previous step's values.
// Values travel between the levels as canonical words, as between the kernels, and a level above 0 runs in place.  Blocks of
// 2 and 3 elements are T = 2 and 3 lanes of one element; the block of 4 is two lanes of two elements on the data and two
// lanes of one on the totals, as the device has several elements per lane at level 0 only.  One library per curve
// (-DSNARKV_CURVE_PALLAS), built by snark-verifier_amd/build.py.  Test infrastructure only.
#include <stddef.h>
#include <stdint.h>
#include <vector>
#include "../../snark-verifier_amd/csrc/poly_prod.h"

using namespace snarkv;

namespace {

typedef std::vector<uint32_t> Words;  // 8 per value

Fr29 load(const Words& w, size_t i) { return fr29_from_canonical(w.data() + 8 * i); }
void store(Words& w, size_t i, const Fr29& v) { fr29_to_canonical(v, w.data() + 8 * i); }

template <uint32_t T, bool RIGHT>
void wg_scan(Fr29* s) {
  typedef ProdBlock<T, 1> S;
  Fr29 prev[T];
  for (uint32_t step = 0; step < S::steps(); ++step) {
    for (uint32_t t = 0; t < T; ++t) prev[t] = s[t];
    for (uint32_t t = 0; t < T; ++t)
      if (RIGHT ? S::has_right(t, step) : S::has_left(t, step))
        s[t] = prod_scan_step(prev[t], prev[RIGHT ? t + S::distance(step) : t - S::distance(step)]);
  }
}

template <uint32_t T, uint32_t E>
struct Level {
  typedef ProdBlock<T, E> S;

  static void load_block(const Words& in, uint32_t b, uint32_t len, bool nz, Fr29 x[T][E], bool zero[T][E]) {
    for (uint32_t t = 0; t < T; ++t)
      for (uint32_t j = 0; j < E; ++j) {
        x[t][j] = S::has(t, j, len) ? load(in, S::index(b, t, j)) : fr29_one();
        zero[t][j] = nz && prod_is_zero(x[t][j]);
        if (zero[t][j]) x[t][j] = fr29_one();
      }
  }

  // k_prod_up
  static void up(const Words& in, uint32_t n, bool nz, Words& totals) {
    totals.assign(8 * (size_t)S::blocks(n), 0);
    for (uint32_t b = 0; b < S::blocks(n); ++b) {
      Fr29 x[T][E], p[T][E], s[T];
      bool zero[T][E];
      load_block(in, b, S::block_len(b, n), nz, x, zero);
      for (uint32_t t = 0; t < T; ++t) prod_lane_prefix<E>(x[t], p[t], s[t]);
      wg_scan<T, false>(s);
      store(totals, b, s[T - 1]);
    }
  }

  // k_prod_down; seq is read and written block by block
  static void prod_down(const Words& in, uint32_t n, const uint32_t* carries, uint32_t stride, Words& out, uint32_t* total) {
    for (uint32_t b = 0; b < S::blocks(n); ++b) {
      const uint32_t len = S::block_len(b, n);
      Fr29 x[T][E], p[T][E], s[T];
      bool zero[T][E];
      load_block(in, b, len, false, x, zero);
      const Fr29 carry = carries ? fr29_from_canonical(carries + 8 * (size_t)b * stride) : fr29_one();
      for (uint32_t t = 0; t < T; ++t) prod_lane_prefix<E>(x[t], p[t], s[t]);
      wg_scan<T, false>(s);
      for (uint32_t t = 0; t < T; ++t) {
        const Fr29 before = t ? fr29_mul(carry, s[t - 1]) : carry;
        Fr29 o[E];
        prod_lane_outputs<E>(before, p[t], o);
        for (uint32_t j = 0; j < E; ++j)
          if (S::has(t, j, len)) store(out, S::index(b, t, j), o[j]);
      }
      if (total && b + 1 == S::blocks(n)) fr29_to_canonical(fr29_mul(carry, s[T - 1]), total);
    }
  }

  // k_inv_down; w = nullptr: the top
  static void inv_down(const Words& in, uint32_t n, const uint32_t* w, bool nz, Words& out, uint32_t* inversions) {
    for (uint32_t b = 0; b < S::blocks(n); ++b) {
      const uint32_t len = S::block_len(b, n);
      Fr29 x[T][E], m[T][E], left[T], right[T];
      bool zero[T][E];
      load_block(in, b, len, nz, x, zero);
      for (uint32_t t = 0; t < T; ++t) {
        prod_lane_others<E>(x[t], m[t], left[t]);
        right[t] = left[t];
      }
      wg_scan<T, false>(left);
      wg_scan<T, true>(right);
      Fr29 wb;
      if (w) {
        wb = fr29_from_canonical(w + 8 * (size_t)b);
      } else {
        wb = prod_inv(left[T - 1]);
        *inversions += 1;
      }
      for (uint32_t t = 0; t < T; ++t) {
        Fr29 around = t ? left[t - 1] : fr29_one();
        if (t + 1 < T) around = fr29_mul(around, right[t + 1]);
        around = fr29_mul(around, wb);
        Fr29 o[E];
        prod_lane_inverses<E>(around, m[t], zero[t], o);
        for (uint32_t j = 0; j < E; ++j)
          if (S::has(t, j, len)) store(out, S::index(b, t, j), o[j]);
      }
    }
  }
};

// the sequences of the levels above 0 and the lengths of all, as levels_of of poly_prod.hip
template <uint32_t T, uint32_t E>
struct Plan {
  std::vector<uint32_t> len;
  std::vector<Words> seq;  // seq[l] for l >= 1; seq[0] unused
  explicit Plan(uint32_t n) {
    uint32_t m = n;
    for (;;) {
      len.push_back(m);
      const uint32_t blocks = len.size() == 1 ? ProdBlock<T, E>::blocks(m) : ProdBlock<T, 1>::blocks(m);
      if (blocks == 1) break;
      m = blocks;
    }
    seq.resize(len.size());
  }
  void sweep_up(const Words& in, bool nz) {
    for (size_t l = 0; l + 1 < len.size(); ++l) {
      if (l == 0) Level<T, E>::up(in, len[0], nz, seq[1]);
      else Level<T, 1>::up(seq[l], len[l], false, seq[l + 1]);
    }
  }
};

template <uint32_t T, uint32_t E>
uint32_t grand_product(const Words& f, uint32_t n, const uint32_t* start, Words& out, uint32_t* total) {
  Plan<T, E> pl(n);
  pl.sweep_up(f, false);
  for (size_t l = pl.len.size(); l-- > 0;) {
    const bool top = l + 1 == pl.len.size();
    const uint32_t* carries = top ? start : pl.seq[l + 1].data();
    if (l > 0) Level<T, 1>::prod_down(pl.seq[l], pl.len[l], carries, top ? 0 : 1, pl.seq[l], top ? total : nullptr);
    else Level<T, E>::prod_down(f, n, carries, top ? 0 : 1, out, top ? total : nullptr);
  }
  return (uint32_t)pl.len.size();
}

template <uint32_t T, uint32_t E>
uint32_t batch_invert(const Words& in, uint32_t n, Words& out, uint32_t* inversions) {
  Plan<T, E> pl(n);
  pl.sweep_up(in, true);
  for (size_t l = pl.len.size(); l-- > 0;) {
    const bool top = l + 1 == pl.len.size();
    const uint32_t* w = top ? nullptr : pl.seq[l + 1].data();
    if (l > 0) Level<T, 1>::inv_down(pl.seq[l], pl.len[l], w, false, pl.seq[l], inversions);
    else Level<T, E>::inv_down(in, n, w, true, out, inversions);
  }
  return (uint32_t)pl.len.size();
}

}  // namespace

extern "C" {

const char* hpp_curve() {
#if defined(SNARKV_CURVE_PALLAS)
  return "pallas";
#else
  return "bn254";
#endif
}

// f: n x 8 words, start: 8 words or null; out: n x 8 words (may be f), total: 8 words.  block in {2, 3, 4}.
// Returns the number of levels, 0 for a bad argument.
uint32_t hpp_grand_product(const uint32_t* f, uint32_t n, const uint32_t* start, uint32_t block, uint32_t* out, uint32_t* total) {
  if (n == 0 || block < 2 || block > 4) return 0;
  Words in(f, f + 8 * (size_t)n), o(8 * (size_t)n, 0xAAAAAAAAu);
  uint32_t levels = 0;
  if (block == 2) levels = grand_product<2, 1>(in, n, start, o, total);
  if (block == 3) levels = grand_product<3, 1>(in, n, start, o, total);
  if (block == 4) levels = grand_product<2, 2>(in, n, start, o, total);
  for (size_t w = 0; w < o.size(); ++w) out[w] = o[w];
  return levels;
}

// in: n x 8 words; out: n x 8 words (may be in); *inversions: how many field inversions the call made
uint32_t hpp_batch_invert(const uint32_t* in, uint32_t n, uint32_t block, uint32_t* out, uint32_t* inversions) {
  if (n == 0 || block < 2 || block > 4) return 0;
  Words i(in, in + 8 * (size_t)n), o(8 * (size_t)n, 0xAAAAAAAAu);
  uint32_t levels = 0;
  *inversions = 0;
  if (block == 2) levels = batch_invert<2, 1>(i, n, o, inversions);
  if (block == 3) levels = batch_invert<3, 1>(i, n, o, inversions);
  if (block == 4) levels = batch_invert<2, 2>(i, n, o, inversions);
  for (size_t w = 0; w < o.size(); ++w) out[w] = o[w];
  return levels;
}

// one factor of the affine product, prod_affine_term as k_prod_affine calls it: a + beta b + gamma (has_b) or a + gamma,
// times `acc`; all canonical words
void hpp_affine_step(const uint32_t* acc, const uint32_t* a, const uint32_t* b, const uint32_t* beta, const uint32_t* gamma,
                     uint32_t has_b, uint32_t* out) {
  const Fr29 g = fr29_from_canonical(gamma), av = fr29_from_canonical(a);
  const Fr29 t = has_b ? prod_affine_term(av, prod_raw(b), prod_scalar_for_raw(fr29_from_canonical(beta)), g)
                       : prod_affine_term(av, g);
  fr29_to_canonical(fr29_mul(fr29_from_canonical(acc), t), out);
}

}  // extern "C"
