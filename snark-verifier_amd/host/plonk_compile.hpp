// The numerator compiler of the PLONK prover: `protocol.quotient.numerator` (an `Expression`, plonk.hpp) as a straight-line
// program of include/snarkv_quotient.h, with its constant table and its column list.  Host only; no device call.
//
//   node                          becomes
//   Polynomial(Query{poly, rot})  SNARKV_QUOT_COL(first_poly + poly, rot)
//   Constant                      an entry of the constant table (equal constants share one)
//   Challenge(i)                  an entry of the table filled at run time: `slots` lists (entry, challenge index)
//   Identity                      the column of the polynomial (0, 1, 0, ...): one extra column, in front of the protocol's
//   Lagrange(i)                   the column of l_0 at rotation -i: l_i(X) = l_0(X w^-i); one extra column for all of them
//   Negated                       SUB from the zero constant
//   Scaled                        MUL by a constant
//   Sum / Product                 ADD / MUL
//   DistributePowers              Horner with FMA, in the order of `expr_evaluate`
//
// Registers: an operand that is a leaf (a column, a constant) is named in the instruction and takes no register; of the two
// sides of a binary node the one that needs more registers is computed first (Sethi-Ullman), and the destination reuses a
// register the instruction reads.  A numerator that is a bare leaf gives `leaf + 0`.
//
// The degree: constants and challenges 0; polynomials, the identity and Lagrange polynomials 1; it adds under products and is
// the larger one under sums.  The extension is the smallest e with 2^e >= max(degree, 1).
//
// `plan_prover` adds what a whole session needs of the protocol and refuses, as InvalidProtocol naming the cause, a
// linearization, committed instances, chunk_degree != 1, a query or an evaluation of an instance polynomial and a polynomial
// index past the quotient's.
#pragma once
#include <algorithm>
#include <array>
#include <map>
#include <string>
#include <vector>

#include "../../include/snarkv_quotient.h"
#include "plonk.hpp"

namespace snarkv_host {

struct NumeratorProgram {
  std::vector<snarkv_quot_instr> prog;
  std::vector<Fr> consts;                          // challenge entries are zero until `fill` writes them
  std::vector<std::pair<size_t, size_t>> slots;    // (entry of consts, challenge index), in order of first use
  int l0_col = -1, x_col = -1;                     // the extra columns, -1 when the numerator needs none
  size_t first_poly = 0;                           // the column of the protocol's polynomial 0
  size_t n_cols = 0;                               // extra columns + the polynomials below the quotient's
  size_t degree = 0, regs = 0;
  uint32_t e = 0;

  // the constant table with the challenges in their entries, packed
  std::vector<uint8_t> fill(const std::vector<Fr>& challenges) const {
    std::vector<uint8_t> out(32 * consts.size());
    std::vector<Fr> c = consts;
    for (auto& s : slots) {
      if (s.second >= challenges.size()) throw InvalidProtocol("Missing challenge");
      c[s.first] = challenges[s.second];
    }
    for (size_t i = 0; i < c.size(); ++i) c[i].to_bytes(&out[32 * i]);
    return out;
  }
};

namespace plonk_compile_detail {

struct Compiler {
  NumeratorProgram out;
  size_t n_polys;  // the quotient's index: polynomials below it are columns
  std::map<std::array<uint8_t, 32>, uint32_t> const_at;
  std::map<size_t, uint32_t> challenge_at;
  std::map<const Expression*, unsigned> need_memo;
  bool reg_used[SNARKV_QUOT_REGS] = {};

  static bool is_leaf(const Expression& e) {
    return e.kind == Expression::Constant || e.kind == Expression::Identity || e.kind == Expression::Lagrange ||
           e.kind == Expression::Polynomial || e.kind == Expression::Challenge;
  }
  static bool is_reg(uint32_t w) { return (w >> 30) == 0; }

  // Sethi-Ullman: the registers a subtree needs when its leaves need none
  unsigned need(const Expression& e) {
    if (is_leaf(e)) return 0;
    auto it = need_memo.find(&e);
    if (it != need_memo.end()) return it->second;
    unsigned r = 1;
    switch (e.kind) {
      case Expression::Negated:
      case Expression::Scaled: r = std::max(1u, need(*e.ch.at(0))); break;
      case Expression::Sum:
      case Expression::Product: {
        const unsigned a = need(*e.ch.at(0)), b = need(*e.ch.at(1));
        r = std::max(1u, a == b ? (a ? a + 1 : 1) : std::max(a, b));
        break;
      }
      case Expression::DistributePowers: {
        if (e.ch.size() < 2) throw Panic("DistributePowers of no expressions (reference: assert!, protocol.rs:359)");
        const size_t n = e.ch.size() - 1;
        if (n == 1) {
          r = need(*e.ch[0]);
          break;
        }
        const unsigned s = need(*e.ch[n]) ? 1 : 0;  // the scalar is held while the terms are computed
        r = std::max({1u, need(*e.ch[0]), 1 + need(*e.ch[n])});
        for (size_t i = 1; i < n; ++i) r = std::max(r, 1 + s + need(*e.ch[i]));
        break;
      }
      default: break;
    }
    need_memo[&e] = r;
    return r;
  }

  uint32_t constant(const Fr& v) {
    std::array<uint8_t, 32> key;
    v.to_bytes(key.data());
    auto it = const_at.find(key);
    if (it != const_at.end()) return SNARKV_QUOT_CONST(it->second);
    if (out.consts.size() >= SNARKV_QUOT_MAX_CONSTS) throw InvalidProtocol("the numerator needs more than 1024 constants (SNARKV_QUOT_MAX_CONSTS)");
    const uint32_t at = (uint32_t)out.consts.size();
    out.consts.push_back(v);
    const_at[key] = at;
    return SNARKV_QUOT_CONST(at);
  }
  uint32_t challenge(size_t i) {
    auto it = challenge_at.find(i);
    if (it != challenge_at.end()) return SNARKV_QUOT_CONST(it->second);
    if (out.consts.size() >= SNARKV_QUOT_MAX_CONSTS) throw InvalidProtocol("the numerator needs more than 1024 constants (SNARKV_QUOT_MAX_CONSTS)");
    const uint32_t at = (uint32_t)out.consts.size();
    out.consts.push_back(Fr::zero());
    out.slots.emplace_back(at, i);
    challenge_at[i] = at;
    return SNARKV_QUOT_CONST(at);
  }
  static void check_rotation(int64_t rot, const char* what) {
    if (rot < -512 || rot > 511) throw InvalidProtocol(std::string(what) + " outside the operand's rotation field (-512 .. 511)");
  }
  uint32_t leaf(const Expression& e) {
    switch (e.kind) {
      case Expression::Constant: return constant(e.scalar);
      case Expression::Challenge: return challenge(e.index);
      case Expression::Identity: return SNARKV_QUOT_COL(out.x_col, 0);
      case Expression::Lagrange:
        check_rotation(-(int64_t)e.lagrange, "Lagrange(i) with i outside -511 .. 512: its rotation is");
        return SNARKV_QUOT_COL(out.l0_col, -e.lagrange);
      default:  // Polynomial
        check_rotation(e.query.rotation, "a rotation of the numerator is");
        return SNARKV_QUOT_COL(out.first_poly + e.query.poly, e.query.rotation);
    }
  }

  uint32_t alloc() {
    for (uint32_t r = 0; r < SNARKV_QUOT_REGS; ++r)
      if (!reg_used[r]) {
        reg_used[r] = true;
        out.regs = std::max<size_t>(out.regs, r + 1);
        return r;
      }
    throw InvalidProtocol("the numerator needs more than 16 registers (SNARKV_QUOT_REGS)");
  }
  void release(uint32_t w) {
    if (is_reg(w)) reg_used[w] = false;
  }
  // one instruction.  The destination is a register among the operands when there is one; the operands' other registers
  // are free afterwards.  `held`: the operand b is a register that lives on (Horner's scalar).
  uint32_t emit(uint8_t op, uint32_t a, uint32_t b, uint32_t c = 0, bool held = false) {
    if (out.prog.size() >= SNARKV_QUOT_MAX_INSTR) throw InvalidProtocol("the numerator needs more than 4096 instructions (SNARKV_QUOT_MAX_INSTR)");
    const bool three = op == SNARKV_QUOT_FMA;
    uint32_t dst;
    if (is_reg(a)) dst = a;
    else if (is_reg(b) && !held) dst = b;
    else if (three && is_reg(c)) dst = c;
    else dst = alloc();
    if (is_reg(a) && a != dst) reg_used[a] = false;
    if (is_reg(b) && b != dst && !held) reg_used[b] = false;
    if (three && is_reg(c) && c != dst) reg_used[c] = false;
    out.prog.push_back(snarkv_quot_instr{op, (uint8_t)dst, 0, a, b, three ? c : 0u});
    return SNARKV_QUOT_REG(dst);
  }

  uint32_t gen(const Expression& e) {
    if (is_leaf(e)) return leaf(e);
    switch (e.kind) {
      case Expression::Negated: {
        const uint32_t a = gen(*e.ch.at(0));
        return emit(SNARKV_QUOT_SUB, constant(Fr::zero()), a);
      }
      case Expression::Scaled: {
        const uint32_t a = gen(*e.ch.at(0));
        return emit(SNARKV_QUOT_MUL, a, constant(e.scalar));
      }
      case Expression::Sum:
      case Expression::Product: {
        const Expression &l = *e.ch.at(0), &r = *e.ch.at(1);
        uint32_t a, b;
        if (need(r) > need(l)) {
          b = gen(r);
          a = gen(l);
        } else {
          a = gen(l);
          b = gen(r);
        }
        return emit(e.kind == Expression::Sum ? SNARKV_QUOT_ADD : SNARKV_QUOT_MUL, a, b);
      }
      case Expression::DistributePowers: {
        if (e.ch.size() < 2) throw Panic("DistributePowers of no expressions (reference: assert!, protocol.rs:359)");
        const size_t n = e.ch.size() - 1;
        if (n == 1) return gen(*e.ch[0]);
        uint32_t acc = gen(*e.ch[0]);
        const uint32_t scalar = gen(*e.ch[n]);
        for (size_t i = 1; i < n; ++i) {
          const uint32_t t = gen(*e.ch[i]);
          acc = emit(SNARKV_QUOT_FMA, acc, scalar, t, true);  // acc * scalar + t
        }
        release(scalar);
        return acc;
      }
      default: throw Panic("bad expression kind");
    }
  }

  size_t degree(const Expression& e) {
    switch (e.kind) {
      case Expression::Constant:
      case Expression::Challenge: return 0;
      case Expression::Identity:
      case Expression::Lagrange:
      case Expression::Polynomial: return 1;
      case Expression::Negated:
      case Expression::Scaled: return degree(*e.ch.at(0));
      case Expression::Sum: return std::max(degree(*e.ch.at(0)), degree(*e.ch.at(1)));
      case Expression::Product: return degree(*e.ch.at(0)) + degree(*e.ch.at(1));
      case Expression::DistributePowers: {
        if (e.ch.size() < 2) throw Panic("DistributePowers of no expressions (reference: assert!, protocol.rs:359)");
        const size_t n = e.ch.size() - 1;
        size_t d = degree(*e.ch[0]);
        if (n == 1) return d;
        const size_t ds = degree(*e.ch[n]);
        for (size_t i = 1; i < n; ++i) d = std::max(d + ds, degree(*e.ch[i]));
        return d;
      }
    }
    throw Panic("bad expression kind");
  }
};

}  // namespace plonk_compile_detail

// the number of witness polynomials `PlonkProof::read` takes: the phases are the `zip` of the two lists
inline size_t plonk_num_witness(const PlonkProtocol& pr) {
  size_t n = 0;
  for (size_t i = 0; i < std::min(pr.num_witness.size(), pr.num_challenge.size()); ++i) n += pr.num_witness[i];
  return n;
}
inline size_t plonk_quotient_index(const PlonkProtocol& pr) {
  return pr.preprocessed.size() + pr.num_instance.size() + plonk_num_witness(pr);
}

// numerator -> program.  Throws InvalidProtocol naming the cause: a limit of snarkv_quotient.h exceeded, e > 8, a rotation
// or a Lagrange index outside the operand's field, a polynomial index at or past the quotient's.
inline NumeratorProgram compile_numerator(const PlonkProtocol& pr) {
  using namespace plonk_compile_detail;
  if (!pr.quotient.numerator) throw InvalidProtocol("the protocol has no numerator");
  const Expression& num = *pr.quotient.numerator;
  Compiler c;
  c.n_polys = plonk_quotient_index(pr);
  std::set<int32_t> lagranges;
  std::set<PQuery> queries;
  expr_collect(num, &lagranges, &queries);
  for (auto& q : queries)
    if (q.poly >= c.n_polys)
      throw InvalidProtocol("the numerator names polynomial " + std::to_string(q.poly) + ", past the quotient's index " + std::to_string(c.n_polys));
  struct HasIdentity {
    static bool in(const Expression& e) {
      if (e.kind == Expression::Identity) return true;
      for (auto& ch : e.ch)
        if (in(*ch)) return true;
      return false;
    }
  };
  size_t extra = 0;
  if (!lagranges.empty()) c.out.l0_col = (int)extra++;
  if (HasIdentity::in(num)) c.out.x_col = (int)extra++;
  c.out.first_poly = extra;
  c.out.n_cols = extra + c.n_polys;
  if (c.out.n_cols > SNARKV_QUOT_MAX_COLS) throw InvalidProtocol("the numerator needs more than 2^20 columns (SNARKV_QUOT_MAX_COLS)");
  c.out.degree = c.degree(num);
  while (((size_t)1 << c.out.e) < std::max<size_t>(c.out.degree, 1)) ++c.out.e;
  if (c.out.e > SNARKV_QUOT_MAX_E)
    throw InvalidProtocol("the numerator has degree " + std::to_string(c.out.degree) + ": the extension e > 8 (SNARKV_QUOT_MAX_E)");
  uint32_t root = c.gen(num);
  if (!Compiler::is_reg(root)) root = c.emit(SNARKV_QUOT_ADD, root, c.constant(Fr::zero()));  // a bare leaf
  return std::move(c.out);
}

// what a prover session holds of a protocol
struct ProverPlan {
  NumeratorProgram num;
  size_t n_pre = 0, n_inst = 0, n_wit = 0, q_index = 0, num_chunk = 0, phases = 0;
  size_t k = 0, n = 0, N = 0;
  size_t device_bytes = 0;  // the columns, the quotient's work buffer and h
  bool committed_instances = false;  // the option is on and the protocol has an instance_committing_key
  size_t cols_total() const { return num.first_poly + q_index + 1; }  // extra | protocol order | the quotient's slot
  // the quotient's work buffer in elements: every column on the extended coset, or on one coset of the domain at a time
  // (snarkv_quotient_cosets.h)
  size_t work_elems(bool by_cosets) const { return num.n_cols * (by_cosets ? n : N); }
  size_t device_bytes_of(bool by_cosets) const { return device_bytes - 32 * (work_elems(false) - work_elems(by_cosets)); }
};

// `committed_instances`: a protocol with an instance_committing_key is taken -- its instance polynomials are committed by the
// session and may be queried and evaluated like witness polynomials.  Off (the default), or without a key, nothing changes:
// the key is refused, and so is any query or evaluation of an instance polynomial (the verifier computes those itself).
inline ProverPlan plan_prover(const PlonkProtocol& pr, uint32_t max_k = 28, bool committed_instances = false) {
  if (pr.linearization != Linearization::None) throw InvalidProtocol("a linearization other than none is not supported by the prover");
  if (pr.instance_committing_key && !committed_instances)
    throw InvalidProtocol("an instance_committing_key (committed instances) is not supported by the prover");
  if (pr.quotient.chunk_degree != 1) throw InvalidProtocol("chunk_degree != 1 is not supported by the prover");
  ProverPlan p;
  p.committed_instances = committed_instances && pr.instance_committing_key;
  if (p.committed_instances)
    for (size_t i = 0; i < pr.num_instance.size(); ++i)
      if (pr.num_instance[i] > pr.instance_committing_key->bases.size())  // the verifier would silently truncate the column
        throw InvalidProtocol("num_instance[" + std::to_string(i) + "] = " + std::to_string(pr.num_instance[i]) + " is above the " +
                              std::to_string(pr.instance_committing_key->bases.size()) + " bases of the instance_committing_key");
  p.n_pre = pr.preprocessed.size();
  p.n_inst = pr.num_instance.size();
  p.n_wit = plonk_num_witness(pr);
  p.phases = std::min(pr.num_witness.size(), pr.num_challenge.size());
  p.q_index = plonk_quotient_index(pr);
  p.num_chunk = pr.quotient.num_chunk;
  p.k = pr.domain.k;
  const std::pair<const char*, const std::vector<PQuery>*> lists[] = {{"a query", &pr.queries}, {"an evaluation", &pr.evaluations}};
  for (auto& l : lists)
    for (auto& q : *l.second) {
      const std::string what = l.first;
      if (!p.committed_instances && q.poly >= p.n_pre && q.poly < p.n_pre + p.n_inst) throw InvalidProtocol(what + " of an instance polynomial is not supported by the prover");
      // the quotient is opened at z and has no listed evaluation: the verifier computes it from the numerator
      if (q.poly > p.q_index || (q.poly == p.q_index && (l.second == &pr.evaluations || q.rotation != 0)))
        throw InvalidProtocol(what + " names polynomial " + std::to_string(q.poly) +
                              (q.poly == p.q_index ? " (the quotient: queried at rotation 0 alone, and never among the evaluations)" : "") +
                              ", past the quotient's index " + std::to_string(p.q_index));
    }
  p.num = compile_numerator(pr);
  if (p.k + p.num.e > max_k)
    throw InvalidProtocol("k + e = " + std::to_string(p.k + p.num.e) + " is past the largest transform (" + std::to_string(max_k) + ")");
  p.n = (size_t)1 << p.k;
  p.N = (size_t)1 << (p.k + p.num.e);
  if (p.num_chunk == 0 || p.num_chunk * p.n > p.N)
    throw InvalidProtocol("num_chunk = " + std::to_string(p.num_chunk) + " does not fit the extended domain of 2^e = " +
                          std::to_string((size_t)1 << p.num.e) + " chunks");
  p.device_bytes = 32 * (p.cols_total() * p.n + p.num.n_cols * p.N + p.N);
  return p;
}

}  // namespace snarkv_host
