// The quotient polynomial on the extended coset (include/snarkv_quotient.h): zero-padding in front of the forward transform,
// the gate program run at every row, the division by the vanishing polynomial, and the four in one call.  Same source for
// both curves, as poly_prod.hip; the arithmetic and its bounds are in quotient.h.
//   k_quot_pad     out[p][i] = coeffs[p][i] for i < n, zero above: the words as they stand
//   k_quot_eval    one row per lane: the program and the constants are uniform over the launch and come through uniform
//                  loads (an instruction is decoded once per wave, its operand kinds are wave-uniform branches); a column
//                  read at a rotation is consecutive across the lanes, the wrap is in the index (quot_row)
//   k_quot_table   the 2^e values of the vanishing polynomial on the coset, canonical words, for the batch inversion
//   k_quot_div     out[i] = in[i] table[i mod 2^e]
// and the coset-at-a-time route (include/snarkv_quotient_cosets.h): the same program on one coset of the small domain after
// the other, over a work buffer of n_cols * n elements, and
//   k_quot_join_tables  the tables of powers the join reads, into the slot's program and constant regions, which the stream has
//                       done with by then
//   k_quot_join    one workgroup per tile of consecutive t by all 2^e cosets (1024 Fr29, 36 KiB of LDS): load times W^(-j t)
//                  and the inverted vanishing entry, e radix-2 levels across the cosets with a barrier each, store times
//                  s^-T 2^-e.  A tile reads and writes the same 2^e rows of t, so in place is safe.  Consecutive lanes take
//                  consecutive t of one coset.  The arithmetic is quotient.h's.
//
// The register file.  16 registers of 9 limbs are indexed by the instruction, at run time, so they cannot live in VGPRs.
// They are in private memory: `Fr29 regs[16]`, 576 bytes per lane, which the compiler lays out dword-interleaved over the
// lanes of a wave, so a register read is 9 coalesced dword accesses at a wave-uniform offset and stays in the vector cache.
// The alternative, LDS limb-major, takes 36 KiB per wave: four waves per CU, one per SIMD, and the multiplier chain of
// fr29_mul is latency-bound at that occupancy (fr29.h).  Private memory leaves the occupancy to the VGPRs.  A register access
// is 36 dword accesses per instruction next to the 162 64-bit multiply-adds of one product.  Neither choice has been
// measured against the other; DESIGN.md 3j has the resource table and the record of this one.
#include <string.h>
#include <vector>
#include "ctx.hpp"
#include "ipa_prover.hpp"
#include "poly_args.hpp"
#include "quotient.h"
#include "../../include/snarkv_ntt.h"
#include "../../include/snarkv_quotient.h"
#include "../../include/snarkv_quotient_cosets.h"

namespace snarkv {

constexpr uint32_t kQuotThreads = 256;
constexpr size_t kQuotMaxCount = 65535;  // columns per transform launch (snarkv_ntt.h)

// layout of the context's SLOT_QUOTIENT
enum : size_t {
  QS_PROG = 0,                                                          // the staged program
  QS_CONSTS = QS_PROG + sizeof(snarkv_quot_instr) * SNARKV_QUOT_MAX_INSTR,  // the constants, Fr29 in the Montgomery domain
  QS_TABLE = (QS_CONSTS + sizeof(Fr29) * SNARKV_QUOT_MAX_CONSTS + 255) & ~(size_t)255,  // the vanishing table, 32 bytes each
  QS_END = QS_TABLE + 32 * ((size_t)1 << SNARKV_QUOT_MAX_E),
};
static_assert(sizeof(snarkv_quot_instr) == 16, "the instruction format of the header");
static_assert(sizeof(Fr29) * JT_END <= QS_TABLE, "the join's tables lie in front of the vanishing table");

struct QuotColsDev {
  const uint32_t* __restrict__ p;
  __device__ __forceinline__ Fr29 load(size_t index) const { return ld_fr(p + 8 * index); }
};

// count x 2^log_n out of count x 2^k; the grid's y is the polynomial
__global__ void __launch_bounds__(kQuotThreads) k_quot_pad(const uint32_t* __restrict__ in, uint32_t k, uint32_t log_n,
                                                           uint32_t* __restrict__ out) {
  const uint32_t i = blockIdx.x * kQuotThreads + threadIdx.x;
  if (i >> log_n) return;
  uint4 a = make_uint4(0, 0, 0, 0), b = a;
  if (!(i >> k)) {
    const uint4* src = reinterpret_cast<const uint4*>(in + 8 * (((size_t)blockIdx.y << k) + i));
    a = src[0], b = src[1];
  }
  uint4* dst = reinterpret_cast<uint4*>(out + 8 * (((size_t)blockIdx.y << log_n) + i));
  dst[0] = a;
  dst[1] = b;
}

__global__ void __launch_bounds__(kQuotThreads) k_quot_eval(const uint32_t* __restrict__ cols, uint32_t log_n, uint32_t e,
                                                            const snarkv_quot_instr* __restrict__ prog, uint32_t n_instr,
                                                            const Fr29* __restrict__ consts, uint32_t* __restrict__ out) {
  const uint32_t row = blockIdx.x * kQuotThreads + threadIdx.x;
  if (row >> log_n) return;
  const QuotColsDev c = {cols};
  Fr29 regs[SNARKV_QUOT_REGS];
#pragma unroll 1
  for (uint32_t pc = 0; pc < n_instr; ++pc) quot_step(prog[pc], regs, consts, c, row, e, log_n);
  st_fr(out + 8 * (size_t)row, regs[prog[n_instr - 1].dst & (SNARKV_QUOT_REGS - 1u)]);
}

__global__ void __launch_bounds__(kQuotThreads) k_quot_table(Fr29 s_to_n, Fr29 root, uint32_t count, uint32_t* __restrict__ out) {
  const uint32_t j = blockIdx.x * kQuotThreads + threadIdx.x;
  if (j < count) st_fr(out + 8 * (size_t)j, quot_vanishing_entry(s_to_n, root, j));
}

// `in` may be `out`: every element is read by the thread that writes it
__global__ void __launch_bounds__(kQuotThreads) k_quot_div(const uint32_t* in, uint32_t log_n, const uint32_t* __restrict__ table,
                                                           uint32_t mask, uint32_t* out) {
  const uint32_t i = blockIdx.x * kQuotThreads + threadIdx.x;
  if (i >> log_n) return;
  st_fr(out + 8 * (size_t)i, fr29_mul(ld_fr(in + 8 * (size_t)i), ld_fr(table + 8 * (size_t)(i & mask))));
}

__global__ void __launch_bounds__(kQuotThreads) k_quot_join_tables(Fr29 w_inv, Fr29 s_inv, Fr29 om_inv, uint32_t e,
                                                                   const uint32_t* __restrict__ inv_words, Fr29* __restrict__ out) {
  const uint32_t idx = blockIdx.x * kQuotThreads + threadIdx.x;
  if (idx < JT_END) out[idx] = quot_join_table_entry(idx, w_inv, s_inv, om_inv, e, inv_words);
}

// in[j][t] -> out[t + q n]; `in` may be `out`.  The grid's x is the tile: n >> tile_bits of them.
__global__ void __launch_bounds__(kQuotThreads) k_quot_join(const uint32_t* in, uint32_t k, uint32_t e, uint32_t tile_bits,
                                                            const Fr29* __restrict__ tab, uint32_t* out) {
  __shared__ Fr29 buf[1u << kQuotJoinTileBits];
  const uint32_t lane = threadIdx.x, t0 = blockIdx.x << tile_bits, slots = 1u << (tile_bits + e);
#pragma unroll 1
  for (uint32_t slot = lane; slot < slots; slot += kQuotThreads) {
    const uint4* src = reinterpret_cast<const uint4*>(in + 8 * quot_join_in_index(slot, t0, k, tile_bits));
    const uint4 a = src[0], b = src[1];
    const uint32_t w[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
    buf[quot_join_in_slot(slot, e, tile_bits)] = quot_join_in(w, tab, slot, t0, k, e, tile_bits);
  }
  __syncthreads();
#pragma unroll 1
  for (uint32_t level = 0; level < e; ++level) {
#pragma unroll 1
    for (uint32_t b = lane; b < slots / 2; b += kQuotThreads) quot_join_butterfly(buf, tab, b, level, e, tile_bits);
    __syncthreads();
  }
#pragma unroll 1
  for (uint32_t slot = lane; slot < slots; slot += kQuotThreads) {
    const size_t T = quot_join_out_index(slot, t0, k, tile_bits);
    uint32_t w[8];
    quot_join_out(buf[slot], tab, (uint32_t)T, k, e, w);
    uint4* dst = reinterpret_cast<uint4*>(out + 8 * T);
    dst[0] = make_uint4(w[0], w[1], w[2], w[3]);
    dst[1] = make_uint4(w[4], w[5], w[6], w[7]);
  }
}

namespace {

uint32_t blocks_of(uint32_t log_n) { return (uint32_t)((((size_t)1 << log_n) + kQuotThreads - 1) / kQuotThreads); }

// the bytes of `count` columns of 2^(k + e) elements for the overlap checks, which come before the lengths': no wrap for an
// absurd shape
size_t ext_bytes(uint32_t k, uint32_t e, size_t count) {
  const uint64_t lg = (uint64_t)k + e;
  const size_t col = lg > 40 ? (size_t)1 << 45 : (size_t)32 << lg;
  return count > ((size_t)1 << 62) / col ? (size_t)1 << 62 : col * count;
}

bool bad_shift(const char* call, const uint8_t* s32) {
  if (s32 && !is_zero32(s32)) return false;
  set_last_error("%s: a shift that is %s", call, s32 ? "zero" : "null");
  return true;
}

int check_shape(uint32_t k, uint32_t e) {
  return e > SNARKV_QUOT_MAX_E || (uint64_t)k + e > SNARKV_API(ntt_max_k)() ? SNARKV_ERR_LENGTH : SNARKV_OK;
}

// every program fault of the header; without columns (n_cols = 0) there is nothing to index: the call is empty
int check_program(const char* call, const snarkv_quot_instr* prog, size_t n_instr, size_t n_consts, size_t n_cols) {
  uint32_t written = 0;
  for (size_t pc = 0; pc < n_instr; ++pc) {
    const snarkv_quot_instr& in = prog[pc];
    const char* fault = nullptr;
    if (in.op > SNARKV_QUOT_FMA) fault = "an unknown op";
    else if (in.zero != 0) fault = "the reserved field is not zero";
    else if (in.op != SNARKV_QUOT_FMA && in.c != 0) fault = "c is not zero on a two-operand op";
    else if (in.dst >= SNARKV_QUOT_REGS) fault = "the destination is no register";
    const uint32_t words[3] = {in.a, in.b, in.c};
    for (uint32_t o = 0; !fault && o < quot_operands(in.op); ++o) {
      const uint32_t w = words[o], kind = quot_kind(w);
      if (kind == kQuotKindReg) {
        if (quot_index(w) >= SNARKV_QUOT_REGS) fault = "an operand names no register";
        else if (!(written >> quot_index(w) & 1u)) fault = "a register is read before it is written";
      } else if (kind == kQuotKindConst) {
        if (quot_index(w) >= n_consts) fault = "a constant index beyond n_consts";
      } else if (kind == kQuotKindCol) {
        if (n_cols && quot_col(w) >= n_cols) fault = "a column index beyond n_cols";
      } else {
        fault = "an operand of kind 3";
      }
    }
    if (fault) {
      set_last_error("%s: instruction %zu: %s", call, pc, fault);
      return SNARKV_ERR_ARG;
    }
    written |= 1u << in.dst;
  }
  return SNARKV_OK;
}

int check_program_lengths(size_t n_cols, size_t n_instr, size_t n_consts) {
  return n_instr > SNARKV_QUOT_MAX_INSTR || n_consts > SNARKV_QUOT_MAX_CONSTS || n_cols > SNARKV_QUOT_MAX_COLS ? SNARKV_ERR_LENGTH
                                                                                                                  : SNARKV_OK;
}

int slot_of(snarkv_ctx* ctx, uint8_t** scr) {
  void* d;
  SNARKV_TRY(ctx_reserve(ctx, SLOT_QUOTIENT, QS_END, &d));
  *scr = (uint8_t*)d;
  return SNARKV_OK;
}

// The enqueue steps; arguments are taken as checked.  The slot has one size, so it does not move between the steps.

int quot_enqueue_extend(snarkv_ctx* ctx, const void* d_coeffs, uint32_t k, uint32_t e, size_t count, const uint32_t* shift,
                        void* d_out) {
  const uint32_t log_n = k + e;
  for (size_t p0 = 0; p0 < count; p0 += kQuotMaxCount) {  // the transform takes 65 535 polynomials per call
    const size_t c = count - p0 < kQuotMaxCount ? count - p0 : kQuotMaxCount;
    const uint8_t* in = (const uint8_t*)d_coeffs + ((p0 * 32) << k);
    uint8_t* out = (uint8_t*)d_out + ((p0 * 32) << log_n);
    hipLaunchKernelGGL(k_quot_pad, dim3(blocks_of(log_n), (uint32_t)c), dim3(kQuotThreads), 0, ctx->stream, (const uint32_t*)in, k,
                       log_n, (uint32_t*)out);
    SNARKV_HIP(hipGetLastError());
    SNARKV_TRY(ntt_enqueue(ctx, out, out, log_n, c, false, shift));
  }
  return SNARKV_OK;
}

// the program and the constants into the slot
int quot_stage_program(snarkv_ctx* ctx, const snarkv_quot_instr* prog, size_t n_instr, const uint8_t* consts32, size_t n_consts) {
  uint8_t* scr;
  SNARKV_TRY(slot_of(ctx, &scr));
  std::vector<Fr29> consts(n_consts);
  for (size_t j = 0; j < n_consts; ++j) {
    uint32_t w[8];
    memcpy(w, consts32 + 32 * j, 32);
    consts[j] = fr29_from_canonical(w);
  }
  // host arrays in pageable memory: the copies have left them when hipMemcpyAsync returns
  SNARKV_HIP(hipMemcpyAsync(scr + QS_PROG, prog, sizeof(snarkv_quot_instr) * n_instr, hipMemcpyHostToDevice, ctx->stream));
  if (n_consts)
    SNARKV_HIP(hipMemcpyAsync(scr + QS_CONSTS, consts.data(), sizeof(Fr29) * n_consts, hipMemcpyHostToDevice, ctx->stream));
  return SNARKV_OK;
}

// the staged program over n_cols columns of 2^log_n values; a rotation is rot 2^e rows
int quot_launch_eval(snarkv_ctx* ctx, const void* d_cols, uint32_t log_n, uint32_t e, size_t n_instr, void* d_out) {
  uint8_t* scr;
  SNARKV_TRY(slot_of(ctx, &scr));
  hipLaunchKernelGGL(k_quot_eval, dim3(blocks_of(log_n)), dim3(kQuotThreads), 0, ctx->stream, (const uint32_t*)d_cols, log_n, e,
                     (const snarkv_quot_instr*)(scr + QS_PROG), (uint32_t)n_instr, (const Fr29*)(scr + QS_CONSTS),
                     (uint32_t*)d_out);
  SNARKV_HIP(hipGetLastError());
  return SNARKV_OK;
}

int quot_enqueue_eval(snarkv_ctx* ctx, const void* d_cols, uint32_t k, uint32_t e, const snarkv_quot_instr* prog, size_t n_instr,
                      const uint8_t* consts32, size_t n_consts, void* d_out) {
  SNARKV_TRY(quot_stage_program(ctx, prog, n_instr, consts32, n_consts));
  return quot_launch_eval(ctx, d_cols, k + e, e, n_instr, d_out);
}

// the 2^e inverted values of the vanishing polynomial into the slot's table: canonical words
int quot_enqueue_table(snarkv_ctx* ctx, uint32_t k, uint32_t e, const uint32_t* shift, uint32_t** table_out) {
  uint8_t* scr;
  SNARKV_TRY(slot_of(ctx, &scr));
  uint32_t* table = (uint32_t*)(scr + QS_TABLE);
  const uint32_t entries = 1u << e;
  hipLaunchKernelGGL(k_quot_table, dim3((entries + kQuotThreads - 1) / kQuotThreads), dim3(kQuotThreads), 0, ctx->stream,
                     quot_shift_to_n(fr29_from_canonical(shift), k), quot_coset_root(e), entries, table);
  SNARKV_HIP(hipGetLastError());
  SNARKV_TRY(prod_batch_invert_enqueue(ctx, table, entries, table));  // the one field inversion of the call
  *table_out = table;
  return SNARKV_OK;
}

int quot_enqueue_div(snarkv_ctx* ctx, const void* d_in, uint32_t k, uint32_t e, const uint32_t* shift, void* d_out) {
  uint32_t* table;
  SNARKV_TRY(quot_enqueue_table(ctx, k, e, shift, &table));
  const uint32_t entries = 1u << e, log_n = k + e;
  hipLaunchKernelGGL(k_quot_div, dim3(blocks_of(log_n)), dim3(kQuotThreads), 0, ctx->stream, (const uint32_t*)d_in, log_n,
                     (const uint32_t*)table, entries - 1u, (uint32_t*)d_out);
  SNARKV_HIP(hipGetLastError());
  return SNARKV_OK;
}

// The way back from the 2^e cosets (quotient.h): every coset's values to coefficients by one inverse transform of size k
// over all of them, d_vals -> d_out, then the join over d_out in place.  Its tables go into the slot's program and constant
// regions: whatever kernel read a program there is ahead on the stream.  d_inv: the 2^e canonical factors g_j on the device,
// or null for one.
int quot_enqueue_join(snarkv_ctx* ctx, const void* d_vals, uint32_t k, uint32_t e, const uint32_t* shift_inv, const uint32_t* d_inv,
                      void* d_out) {
  SNARKV_TRY(ntt_enqueue(ctx, d_vals, d_out, k, (size_t)1 << e, true, nullptr));
  uint8_t* scr;
  SNARKV_TRY(slot_of(ctx, &scr));
  Fr29* tab = (Fr29*)(scr + QS_PROG);
  hipLaunchKernelGGL(k_quot_join_tables, dim3((JT_END + kQuotThreads - 1) / kQuotThreads), dim3(kQuotThreads), 0, ctx->stream,
                     ntt_root_squared(true, SNARKV_FR_TWO_ADICITY - (k + e)), fr29_from_canonical(shift_inv),
                     ntt_root_squared(true, SNARKV_FR_TWO_ADICITY - e), e, d_inv, tab);
  SNARKV_HIP(hipGetLastError());
  const uint32_t tile_bits = quot_join_tile_bits(k, e);
  hipLaunchKernelGGL(k_quot_join, dim3(1u << (k - tile_bits)), dim3(kQuotThreads), 0, ctx->stream, (const uint32_t*)d_out, k, e,
                     tile_bits, (const Fr29*)tab, (uint32_t*)d_out);
  SNARKV_HIP(hipGetLastError());
  return SNARKV_OK;
}

}  // namespace

}  // namespace snarkv

using namespace snarkv;

extern "C" {

int SNARKV_API(poly_extend_dev)(snarkv_ctx* ctx, const void* d_coeffs32, uint32_t k, uint32_t e, size_t count,
                                const uint8_t* shift32, void* d_out32) {
  if (!ctx || !aligned16(d_coeffs32) || !aligned16(d_out32) || bad_shift("poly_extend", shift32)) return SNARKV_ERR_ARG;
  if (overlap(d_out32, ext_bytes(k, e, count), d_coeffs32, ext_bytes(k, 0, count)))
    return refuse_overlap("poly_extend", "out is disjoint from the coefficients");
  if (!below_r(shift32)) return SNARKV_ERR_ENCODING;
  if (count == 0) return SNARKV_ERR_EMPTY;
  SNARKV_TRY(check_shape(k, e));
  if (count > kQuotMaxCount) return SNARKV_ERR_LENGTH;
  SNARKV_HIP(hipSetDevice(ctx->device));
  uint32_t shift[8];
  memcpy(shift, shift32, 32);
  return quot_enqueue_extend(ctx, d_coeffs32, k, e, count, shift, d_out32);
}

int SNARKV_API(quotient_eval_dev)(snarkv_ctx* ctx, const void* d_cols32, uint32_t k, uint32_t e, size_t n_cols,
                                  const snarkv_quot_instr* prog, size_t n_instr, const uint8_t* consts32, size_t n_consts,
                                  void* d_out32) {
  if (!ctx || !aligned16(d_cols32) || !aligned16(d_out32) || !prog || (n_consts && !consts32)) return SNARKV_ERR_ARG;
  SNARKV_TRY(check_program("quotient_eval", prog, n_instr, n_consts, n_cols));
  if (overlap(d_out32, ext_bytes(k, e, 1), d_cols32, ext_bytes(k, e, n_cols)))
    return refuse_overlap("quotient_eval", "out lies in no part of the columns");
  if (!all_below_r(consts32, n_consts)) return SNARKV_ERR_ENCODING;
  if (n_cols == 0 || n_instr == 0) return SNARKV_ERR_EMPTY;
  SNARKV_TRY(check_shape(k, e));
  SNARKV_TRY(check_program_lengths(n_cols, n_instr, n_consts));
  SNARKV_HIP(hipSetDevice(ctx->device));
  return quot_enqueue_eval(ctx, d_cols32, k, e, prog, n_instr, consts32, n_consts, d_out32);
}

int SNARKV_API(poly_div_vanishing_dev)(snarkv_ctx* ctx, const void* d_in32, uint32_t k, uint32_t e, const uint8_t* shift32,
                                       void* d_out32) {
  if (!ctx || !aligned16(d_in32) || !aligned16(d_out32) || bad_shift("poly_div_vanishing", shift32)) return SNARKV_ERR_ARG;
  if (partial_overlap(d_out32, d_in32, ext_bytes(k, e, 1)))
    return refuse_overlap("poly_div_vanishing", "out is the input itself or disjoint from it");
  if (!below_r(shift32)) return SNARKV_ERR_ENCODING;
  SNARKV_TRY(check_shape(k, e));
  SNARKV_HIP(hipSetDevice(ctx->device));
  uint32_t shift[8];
  memcpy(shift, shift32, 32);
  return quot_enqueue_div(ctx, d_in32, k, e, shift, d_out32);
}

int SNARKV_API(quotient_dev)(snarkv_ctx* ctx, const void* d_coeffs32, uint32_t k, uint32_t e, size_t n_cols,
                             const snarkv_quot_instr* prog, size_t n_instr, const uint8_t* consts32, size_t n_consts,
                             const uint8_t* shift32, const uint8_t* shift_inv32, void* d_work32, void* d_h32) {
  if (!ctx || !aligned16(d_coeffs32) || !aligned16(d_work32) || !aligned16(d_h32) || !prog || (n_consts && !consts32))
    return SNARKV_ERR_ARG;
  if (bad_shift("quotient", shift32) || bad_shift("quotient", shift_inv32)) return SNARKV_ERR_ARG;
  SNARKV_TRY(check_program("quotient", prog, n_instr, n_consts, n_cols));
  const size_t coeffs = ext_bytes(k, 0, n_cols), work = ext_bytes(k, e, n_cols), h = ext_bytes(k, e, 1);
  if (overlap(d_work32, work, d_coeffs32, coeffs) || overlap(d_h32, h, d_coeffs32, coeffs) || overlap(d_h32, h, d_work32, work))
    return refuse_overlap("quotient", "work, h and the coefficients are pairwise disjoint");
  if (!all_below_r(consts32, n_consts) || !below_r(shift32) || !below_r(shift_inv32)) return SNARKV_ERR_ENCODING;
  if (n_cols == 0 || n_instr == 0) return SNARKV_ERR_EMPTY;
  SNARKV_TRY(check_shape(k, e));
  SNARKV_TRY(check_program_lengths(n_cols, n_instr, n_consts));
  SNARKV_HIP(hipSetDevice(ctx->device));
  uint32_t shift[8], shift_inv[8];
  memcpy(shift, shift32, 32);
  memcpy(shift_inv, shift_inv32, 32);
  // the three public calls and the inverse transform, back to back
  SNARKV_TRY(quot_enqueue_extend(ctx, d_coeffs32, k, e, n_cols, shift, d_work32));
  SNARKV_TRY(quot_enqueue_eval(ctx, d_work32, k, e, prog, n_instr, consts32, n_consts, d_h32));
  SNARKV_TRY(quot_enqueue_div(ctx, d_h32, k, e, shift, d_h32));
  return ntt_enqueue(ctx, d_h32, d_h32, k + e, 1, true, shift_inv);
}

int SNARKV_API(poly_cosets_join_dev)(snarkv_ctx* ctx, const void* d_vals32, uint32_t k, uint32_t e, const uint8_t* shift_inv32,
                                     void* d_out32) {
  if (!ctx || !aligned16(d_vals32) || !aligned16(d_out32) || bad_shift("poly_cosets_join", shift_inv32)) return SNARKV_ERR_ARG;
  if (partial_overlap(d_out32, d_vals32, ext_bytes(k, e, 1)))
    return refuse_overlap("poly_cosets_join", "out is the input itself or disjoint from it");
  if (!below_r(shift_inv32)) return SNARKV_ERR_ENCODING;
  SNARKV_TRY(check_shape(k, e));
  SNARKV_HIP(hipSetDevice(ctx->device));
  uint32_t shift_inv[8];
  memcpy(shift_inv, shift_inv32, 32);
  return quot_enqueue_join(ctx, d_vals32, k, e, shift_inv, nullptr, d_out32);
}

int SNARKV_API(quotient_cosets_dev)(snarkv_ctx* ctx, const void* d_coeffs32, uint32_t k, uint32_t e, size_t n_cols,
                                    const snarkv_quot_instr* prog, size_t n_instr, const uint8_t* consts32, size_t n_consts,
                                    const uint8_t* shift32, const uint8_t* shift_inv32, void* d_work32, void* d_h32) {
  if (!ctx || !aligned16(d_coeffs32) || !aligned16(d_work32) || !aligned16(d_h32) || !prog || (n_consts && !consts32))
    return SNARKV_ERR_ARG;
  if (bad_shift("quotient_cosets", shift32) || bad_shift("quotient_cosets", shift_inv32)) return SNARKV_ERR_ARG;
  SNARKV_TRY(check_program("quotient_cosets", prog, n_instr, n_consts, n_cols));
  const size_t coeffs = ext_bytes(k, 0, n_cols), work = coeffs, h = ext_bytes(k, e, 1);  // work is one coset of every column
  if (overlap(d_work32, work, d_coeffs32, coeffs) || overlap(d_h32, h, d_coeffs32, coeffs) || overlap(d_h32, h, d_work32, work))
    return refuse_overlap("quotient_cosets", "work, h and the coefficients are pairwise disjoint");
  if (!all_below_r(consts32, n_consts) || !below_r(shift32) || !below_r(shift_inv32)) return SNARKV_ERR_ENCODING;
  if (n_cols == 0 || n_instr == 0) return SNARKV_ERR_EMPTY;
  SNARKV_TRY(check_shape(k, e));
  SNARKV_TRY(check_program_lengths(n_cols, n_instr, n_consts));
  SNARKV_HIP(hipSetDevice(ctx->device));
  uint32_t shift[8], shift_inv[8];
  memcpy(shift, shift32, 32);
  memcpy(shift_inv, shift_inv32, 32);
  // once: the program, the inverted vanishing table
  SNARKV_TRY(quot_stage_program(ctx, prog, n_instr, consts32, n_consts));
  uint32_t* table;
  SNARKV_TRY(quot_enqueue_table(ctx, k, e, shift, &table));
  // per coset j: the columns on (s W^j) H by one size-k transform each, the program there with a rotation of one row
  const Fr29 root = ntt_root_squared(false, SNARKV_FR_TWO_ADICITY - (k + e));  // W
  Fr29 coset_shift = fr29_from_canonical(shift);                               // s W^j: products only
  for (uint32_t j = 0; !(j >> e); ++j) {
    uint32_t sj[8];
    fr29_to_canonical(coset_shift, sj);
    for (size_t p0 = 0; p0 < n_cols; p0 += kQuotMaxCount) {  // the transform takes 65 535 polynomials per call
      const size_t c = n_cols - p0 < kQuotMaxCount ? n_cols - p0 : kQuotMaxCount;
      SNARKV_TRY(ntt_enqueue(ctx, (const uint8_t*)d_coeffs32 + ((p0 * 32) << k), (uint8_t*)d_work32 + ((p0 * 32) << k), k, c, false, sj));
    }
    SNARKV_TRY(quot_launch_eval(ctx, d_work32, k, 0, n_instr, (uint8_t*)d_h32 + (((size_t)j * 32) << k)));
    coset_shift = fr29_mul(coset_shift, root);
  }
  // back: every coset's values to coefficients in one call and the join across the cosets, with the division in it
  return quot_enqueue_join(ctx, d_h32, k, e, shift_inv, table, d_h32);
}

}  // extern "C"
