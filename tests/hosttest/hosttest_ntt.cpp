// Host build of the transform behind snarkv_ntt_dev (snark-verifier_amd/csrc/ntt_plan.h and ntt_tile.h, the SNARKV_HD source the
// device compiles), driven the way ntt.hip drives it: the tables of powers by ntt_table_entry, then pass by pass, tile by
// tile: every slot of a tile is loaded into the tile's buffer, the lanes take the butterflies of a level one after the other
// (the pairs of a level are disjoint, so no copy between levels is needed), every slot is stored.  Values travel between the
// passes as canonical words, through a working buffer, as between the kernels.  Tile sizes 2^1, 2^2, 2^3 and the device's
// 2^9, chosen at run time.  Every input of a multiplier in the tile's arithmetic is recorded, so that a test can hold the
// largest against the bound ntt_tile.h states.  One library per curve (-DSNARKV_CURVE_PALLAS), built by
// snark-verifier_amd/build.py.  Test infrastructure only.
#include <math.h>
#include <stdint.h>
#include <vector>
#include "../../snark-verifier_amd/csrc/fr29.h"

namespace {
double g_max_ratio = 0.0;  // largest |value| / r seen at a multiplier input since the last reset
void probe(const snarkv::Fr29& x) {
  constexpr int32_t rl[9] = SNARKV_FR29_P_LIMBS;
  long double v = 0, r = 0;
  for (int i = 8; i >= 0; --i) {
    v = v * 536870912.0L + x.v[i];
    r = r * 536870912.0L + rl[i];
  }
  const double q = (double)fabsl(v / r);
  if (q > g_max_ratio) g_max_ratio = q;
}
}  // namespace
#define SNARKV_NTT_PROBE(x) probe(x)
#include "../../snark-verifier_amd/csrc/ntt_plan.h"
#include "../../snark-verifier_amd/csrc/ntt_tile.h"

using namespace snarkv;

namespace {

typedef std::vector<Fr29> Table;

Table table(const Fr29& base, uint32_t pre, uint32_t count, const Fr29& scale) {
  Table t(count);
  for (uint32_t j = 0; j < count; ++j) t[j] = ntt_table_entry(base, pre, j, scale);
  return t;
}

// ntt.hip's enqueue and k_ntt_pass for one polynomial
template <uint32_t T, uint32_t C>
void transform(const uint32_t* in, uint32_t* out, uint32_t k, bool inverse, const uint32_t* shift) {
  typedef NttPlan<T, C> Plan;
  const Plan plan(k);
  const uint32_t h = plan.split_bits(), n_lo = 1u << h, n_hi = 1u << (k - h);
  const Table tile_tw = table(ntt_root_squared(inverse, SNARKV_FR_TWO_ADICITY - T), 0, 1u << (T - 1), fr29_one());
  const Fr29 n_inv = ntt_table_entry(fr29_one(), 0, 0, ntt_n_inverse(k));
  Table w_lo, w_hi, s_lo, s_hi;
  if (plan.passes > 1) {
    const Fr29 w = ntt_root_squared(inverse, SNARKV_FR_TWO_ADICITY - k);
    w_lo = table(w, 0, n_lo, ntt_factor_out());
    w_hi = table(w, h, n_hi, fr29_one());
  }
  if (shift) {
    const Fr29 s = fr29_from_canonical(shift);
    s_lo = table(s, 0, n_lo, inverse ? ntt_n_inverse(k) : ntt_factor_in());
    s_hi = table(s, h, n_hi, fr29_one());
  }
  std::vector<uint32_t> work(8 * ((size_t)1 << k));
  for (uint32_t p = 0; p < plan.passes; ++p) {
    const uint32_t* src = p == 0 ? in : work.data();
    uint32_t* dst = plan.last(p) ? out : work.data();
    const uint32_t slots = plan.slots(p);
    for (uint32_t g = 0; g < plan.tiles(p); ++g) {
      Fr29 buf[1u << T];
      for (uint32_t slot = 0; slot < slots; ++slot) {
        const uint32_t j = plan.load_index(p, g, slot);
        const Fr29 f = p == 0 && shift && !inverse ? ntt_factor(s_lo.data(), s_hi.data(), j, h) : ntt_factor_in();
        buf[plan.load_lds(p, slot)] = ntt_load(src + 8 * (size_t)j, f);
      }
      for (uint32_t level = 0; level < plan.t[p]; ++level)
        for (uint32_t lane = 0; lane < slots / 2; ++lane)
          ntt_butterfly(buf, plan.bfly_top(p, level, lane), plan.bfly_distance(p, level), tile_tw[plan.bfly_twiddle(p, level, lane)],
                        level);
      uint32_t tile_out[8 << T];  // a pass before the last runs in place: store the tile after all of it is computed
      uint32_t at[1u << T];
      for (uint32_t slot = 0; slot < slots; ++slot) {
        const uint32_t i = plan.store_index(p, g, slot);
        Fr29 f = ntt_factor_out();
        if (!plan.last(p)) f = ntt_factor(w_lo.data(), w_hi.data(), plan.twiddle_exp(p, g, slot), h);
        else if (inverse && shift) f = ntt_factor(s_lo.data(), s_hi.data(), i, h);
        else if (inverse) f = n_inv;
        ntt_store(buf[plan.store_lds(p, slot)], f, tile_out + 8 * slot);
        at[slot] = i;
      }
      for (uint32_t slot = 0; slot < slots; ++slot)
        for (int w = 0; w < 8; ++w) dst[8 * (size_t)at[slot] + w] = tile_out[8 * slot + w];
    }
  }
}

template <uint32_t T, uint32_t C>
uint32_t plan_of(uint32_t k, uint32_t* t, uint32_t* c) {
  const NttPlan<T, C> plan(k);
  for (uint32_t p = 0; p < plan.passes; ++p) t[p] = plan.t[p], c[p] = plan.c[p];
  return plan.passes;
}

// per (tile, slot) of pass p, tile-major: the index loaded, the index stored, the LDS place on load and on store
template <uint32_t T, uint32_t C>
void indices_of(uint32_t k, uint32_t p, uint32_t* load, uint32_t* store, uint32_t* lds_load, uint32_t* lds_store) {
  const NttPlan<T, C> plan(k);
  size_t o = 0;
  for (uint32_t g = 0; g < plan.tiles(p); ++g)
    for (uint32_t slot = 0; slot < plan.slots(p); ++slot, ++o) {
      load[o] = plan.load_index(p, g, slot);
      store[o] = plan.store_index(p, g, slot);
      lds_load[o] = plan.load_lds(p, slot);
      lds_store[o] = plan.store_lds(p, slot);
    }
}

}  // namespace

// the tile sizes the library was built for: (T, C) as NttPlan takes them; the last one is the device's (ntt.hip)
#define HN_DISPATCH(T_, CALL)          \
  switch (T_) {                        \
    case 1: CALL(1, 0); break;         \
    case 2: CALL(2, 1); break;         \
    case 3: CALL(3, 1); break;         \
    case 9: CALL(9, 2); break;         \
    default: return 0;                 \
  }

extern "C" {

const char* hn_curve() {
#if defined(SNARKV_CURVE_PALLAS)
  return "pallas";
#else
  return "bn254";
#endif
}

uint32_t hn_two_adicity() { return SNARKV_FR_TWO_ADICITY; }
double hn_bound() { return kNttBound; }
int hn_reduce_after(uint32_t level) { return ntt_reduce_after(level) ? 1 : 0; }
void hn_reset_max() { g_max_ratio = 0.0; }
double hn_max() { return g_max_ratio; }

// in, out: 2^k x 8 words (out may not be in); shift: 8 words or null.  0 when the tile size is not one of 1, 2, 3, 9.
int hn_ntt(const uint32_t* in, uint32_t* out, uint32_t k, uint32_t direction, const uint32_t* shift, uint32_t tile_bits) {
#define CALL(T, C) transform<T, C>(in, out, k, direction != 0, shift)
  HN_DISPATCH(tile_bits, CALL)
#undef CALL
  return 1;
}

// -> the number of passes (0: unknown tile size); t and c take the levels and the column bits of each
uint32_t hn_plan(uint32_t k, uint32_t tile_bits, uint32_t* t, uint32_t* c) {
  uint32_t passes = 0;
#define CALL(T, C) passes = plan_of<T, C>(k, t, c)
  HN_DISPATCH(tile_bits, CALL)
#undef CALL
  return passes;
}

// four arrays of 2^k entries
int hn_pass_indices(uint32_t k, uint32_t tile_bits, uint32_t p, uint32_t* load, uint32_t* store, uint32_t* lds_load,
                    uint32_t* lds_store) {
#define CALL(T, C) indices_of<T, C>(k, p, load, store, lds_load, lds_store)
  HN_DISPATCH(tile_bits, CALL)
#undef CALL
  return 1;
}

}  // extern "C"
