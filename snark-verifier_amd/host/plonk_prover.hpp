// PlonkProver<MOS, TR>: the mirror image of PlonkVerifier (plonk.hpp) -- protocol and witness polynomials in, proof bytes out.
// Driven by the protocol alone: `PlonkProof::read` fixes what is written and when, the numerator is compiled to a gate program
// (plonk_compile.hpp), and the witness polynomials arrive phase by phase from a caller who makes them with the resident-column
// calls (snarkv_ntt.h, snarkv_poly_prod.h, snarkv_lookup.h).
//
// One session for both commitment schemes.  What depends on the scheme sits in PlonkScheme<MOS, TR> below -- the session memory
// of the device library, "commit `count` resident polynomials into the point block", the width of a point in the proof, the
// opening and its length:
//   BN254 / KZG   MOS = Gwc19 or Bdfg21, TR = EvmTranscript or PoseidonTranscript; the key is the SRS
//   pallas / IPA  MOS = Bgh19, TR = Blake2bTranscript (-DSNARKV_HOST_PALLAS); the key is the resident IPA key with h and s,
//                 every commitment is blinded (one blind per polynomial, the caller's), and so is the opening
//
// A session:
//   begin    one resident buffer:  [l_0] [X] | preprocessed | instance | witness | quotient slot | h | work | small block
//            (work is n_cols * N elements; n_cols * n in a session begun with kPlonkQuotientCosets, whose finish takes the
//            quotient one coset at a time: snarkv_quotient_cosets_dev, the same bytes.)
//            The quotient (snarkv_quotient_dev) reads the columns from the extra ones up to the last witness, contiguous; the
//            opening reads from `preprocessed` on and finds the quotient at index n_pre + n_inst + n_wit.  The instance
//            polynomials are built (values in rows 0.., inverse transform); the transcript absorbs the initial state and
//            the instances as `PlonkProof::read` does.  No synchronisation.
//   phase    copy (values: and inverse-transform) into the witness columns, commit them in one batch of MSMs over the SRS,
//            write the points, squeeze the phase's challenges.  One synchronisation (none for a phase without witnesses).
//   finish   quotient -> tail check -> chunk commitments (sync 1: points and the status word) -> z -> every evaluation in one
//            batched call (sync 2) -> Q = sum (z^n)^i h_i into the quotient slot -> the verifier's own identity check on the
//            host -> MOS::create_proof (Gwc19: one more synchronisation, Bdfg21: two, Bgh19: three).
// Over IPA the session also keeps one blind per polynomial below the quotient (0 for the instance polynomials, which are never
// committed or queried -- unless begin is told to take an instance_committing_key: see begin) and forms blind(Q) = sum (z^n)^i blind(h_i) on the host, next to Q.
// The prover draws no randomness: blinding rows and the random polynomial are the caller's columns, and so are the blinds and
// the randomness of the IPA opening.
#pragma once
#include <type_traits>

#include "../../include/snarkv_ntt.h"
#include "../../include/snarkv_poly.h"
#include "../../include/snarkv_poly_batch.h"
#include "../../include/snarkv_quotient.h"
#include "../../include/snarkv_quotient_cosets.h"
#include "plonk.hpp"
#include "plonk_compile.hpp"
#if defined(SNARKV_HOST_PALLAS)
#include "../../include/snarkv_ipa_commit_blinded.h"
#include "../../include/snarkv_pallas_session.h"
#include "blake2b_transcript.hpp"
#define SNARKV_PLONK_DEV(name) snarkv_pallas_##name  // the stages of the device library this flavour is linked against
#else
#include "../../include/snarkv_plonk_prove.h"
#include "transcript.hpp"
#define SNARKV_PLONK_DEV(name) snarkv_##name
#endif

namespace snarkv_host {

constexpr const char* kPlonkUnsatisfied = "the witness does not satisfy the protocol's constraints";
enum PlonkWitnessForm { kPlonkCoeffs = 0, kPlonkValues = 1 };
constexpr uint32_t kPlonkQuotientCosets = 1u;  // SNARKV_HOST_PLONK_QUOTIENT_COSETS
constexpr uint32_t kPlonkKnownFlags = kPlonkQuotientCosets;

// halo2's ZETA: a primitive cube root of unity, g^((r - 1) / 3) with g the field's multiplicative generator (7 for BN254's
// scalar field, 5 for pallas': include/snarkv_ntt.h) -- the coset shift of the extended domain
inline Fr plonk_zeta() {
#if defined(SNARKV_HOST_PALLAS)
  constexpr uint64_t kGenerator = 5;
#else
  constexpr uint64_t kGenerator = 7;
#endif
  uint8_t b[32];
  (Fr::zero() - Fr::one()).to_bytes(b);  // r - 1
  unsigned rem = 0;
  for (int i = 31; i >= 0; --i) {
    const unsigned cur = rem * 256 + b[i];
    b[i] = (uint8_t)(cur / 3);
    rem = cur % 3;
  }
  if (rem != 0) throw Panic("3 does not divide r - 1");
  uint64_t e[4];
  memcpy(e, b, 32);
  return Fr::from_u64(kGenerator).pow(e);
}

// what finish takes over IPA, all the caller's: one blind per chunk of h, the blind of f, the n scalars of p_bar in device
// memory and the blind of p_bar's commitment (include/snarkv_ipa_multiopen.h)
struct PlonkFinishBlinds {
  const uint8_t* chunk_blinds32;
  const uint8_t* f_blind32;
  const void* d_pbar32;
  const uint8_t* omega_bar32;
};

struct PlonkProverSession {
  virtual ~PlonkProverSession() = default;
  virtual size_t num_phases() const = 0;
  virtual size_t phase_challenges(size_t phase) const = 0;
  virtual size_t phase_witnesses(size_t phase) const = 0;
  virtual size_t proof_length() const = 0;
  // Result of phase: the challenges squeezed.  blinds32: one per witness polynomial of the phase (IPA; null over KZG)
  virtual Result<std::vector<Fr>> phase(const void* d_witness, int form, const uint8_t* blinds32 = nullptr) = 0;
  virtual Result<std::vector<uint8_t>> finish(const PlonkFinishBlinds* rnd = nullptr) = 0;
};

// a key that the device refuses for its size, which only the device library can see (a shard): an argument error
struct PlonkKeyMismatch : std::runtime_error {
  using std::runtime_error::runtime_error;
};

inline void plonk_dev(int rc, const char* what) {
  if (rc < 0) throw std::runtime_error(std::string(what) + ": " + SNARKV_DEV_LAST_ERROR());
}

// The commitment scheme's side of a session.  Every PlonkScheme has
//   kPointBytes                       the width of a point in the proof
//   mem_alloc / mem_free / upload / copy / download / tail_check     the session memory of the device library
//   prepare(pr)                       what the queries mean for the opening (its number of sets)
//   opening_length(k)                 the bytes MOS::create_proof writes
//   start(t)                          before the transcript takes its first byte
//   note_blinds(first, count, b32)    keeps the blinds of `count` polynomials from the session's index `first` on (IPA)
//   commit(ctx, d_first, n, first, count, d_out64)    enqueues the commitments to `count` resident polynomials, 64 bytes each
//   open(ctx, d_polys, n, q_index, zn_powers, z, queries, rnd, t)    MOS::create_proof over the polynomials 0 .. q_index
template <class MOS, class TR>
struct PlonkScheme;

#if !defined(SNARKV_HOST_PALLAS)
template <class MOS, class TR>
struct PlonkScheme {  // KZG: the key is the SRS, nothing is blinded
  static constexpr size_t kPointBytes = std::is_same<TR, EvmTranscript>::value ? 64 : 32;
  const void* d_srs = nullptr;
  size_t n_sets = 0;

  static int mem_alloc(snarkv_ctx* c, size_t bytes, void** d) { return snarkv_plonk_session_alloc(c, bytes, d); }
  static void mem_free(snarkv_ctx* c, void* d) { snarkv_plonk_session_free(c, d); }
  static int upload(snarkv_ctx* c, void* d, const void* src, size_t bytes) { return snarkv_plonk_session_upload(c, d, src, bytes); }
  static int copy(snarkv_ctx* c, void* d, const void* d_src, size_t bytes) { return snarkv_plonk_session_copy(c, d, d_src, bytes); }
  static int download(snarkv_ctx* c, void* dst, const void* d_src, size_t bytes) { return snarkv_plonk_session_download(c, dst, d_src, bytes); }
  static int tail_check(snarkv_ctx* c, const void* d_tail, size_t count, void* d_status) { return snarkv_plonk_tail_check_dev(c, d_tail, count, d_status); }

  void prepare(const PlonkProtocol& pr, const ProverPlan&) {
    std::vector<uint32_t> qp;
    std::vector<uint8_t> qs(32 * pr.queries.size());
    for (size_t i = 0; i < pr.queries.size(); ++i) {
      qp.push_back((uint32_t)pr.queries[i].poly);
      pr.domain.rotate_scalar(Fr::one(), pr.queries[i].rotation).to_bytes(&qs[32 * i]);
    }
    plonk_dev(snarkv_kzg_multiopen_sets(std::is_same<MOS, Gwc19>::value ? SNARKV_KZG_MOS_GWC19 : SNARKV_KZG_MOS_BDFG21, qp.data(), qs.data(),
                                        qp.size(), &n_sets),
              "kzg_multiopen_sets");
  }
  size_t opening_length(size_t) const { return kPointBytes * (std::is_same<MOS, Gwc19>::value ? n_sets : 2); }
  void start(TR&) {}
  void note_blinds(size_t, size_t, const uint8_t*) {}
  Error instance_key(const InstanceCommittingKey&, size_t, size_t) { return Error{Error::InvalidProtocol, "committed instances are not supported over KZG"}; }
  void commit(snarkv_ctx* ctx, const uint8_t* d_first, size_t n, size_t, size_t count, uint8_t* d_out64) {
    std::vector<const void*> d_s(count), d_p(count, d_srs);
    std::vector<size_t> ns(count, n);
    for (size_t i = 0; i < count; ++i) d_s[i] = d_first + 32 * n * i;
    plonk_dev(snarkv_g1_msm_pippenger_many_dev(ctx, count, d_s.data(), d_p.data(), ns.data(), 0, d_out64), "g1_msm_pippenger_many");
  }
  Error open(snarkv_ctx* ctx, const uint8_t* d_polys, size_t n, size_t q_index, const std::vector<Fr>&, const Fr& z,
             const std::vector<Query<Fr>>& queries, const PlonkFinishBlinds*, TR& t) {
    const KzgOpenInput in{ctx, d_srs, d_polys, n, q_index + 1};
    auto opened = MOS::create_proof(in, z, queries, t);
    return opened.ok() ? Error{} : opened.err;
  }
};
#else
template <>
struct PlonkScheme<Bgh19, Blake2bTranscript> {  // IPA: the resident key with h and s, every commitment blinded
  static constexpr size_t kPointBytes = 32;
  const snarkv_ipa_dk* dk = nullptr;
  G1Affine h, s;
  std::vector<Fr> blinds;   // one per polynomial of the session and per chunk of h: 0 until given, 0 for instances
  size_t n_sets = 0;
  std::optional<IpaAccumulator> acc;  // of the opening, once finish has written a proof

  static int mem_alloc(snarkv_ctx* c, size_t bytes, void** d) { return snarkv_pallas_session_alloc(c, bytes, d); }
  static void mem_free(snarkv_ctx* c, void* d) { snarkv_pallas_session_free(c, d); }
  static int upload(snarkv_ctx* c, void* d, const void* src, size_t bytes) { return snarkv_pallas_session_upload(c, d, src, bytes); }
  static int copy(snarkv_ctx* c, void* d, const void* d_src, size_t bytes) { return snarkv_pallas_session_copy(c, d, d_src, bytes); }
  static int download(snarkv_ctx* c, void* dst, const void* d_src, size_t bytes) { return snarkv_pallas_session_download(c, dst, d_src, bytes); }
  static int tail_check(snarkv_ctx* c, const void* d_tail, size_t count, void* d_status) { return snarkv_pallas_poly_tail_check_dev(c, d_tail, count, d_status); }

  void prepare(const PlonkProtocol& pr, const ProverPlan& plan) {
    std::vector<Query<Fr>> qs;
    for (auto& q : pr.queries) qs.push_back(Query<Fr>{q.poly, pr.domain.rotate_scalar(Fr::one(), q.rotation), Fr::zero()});
    n_sets = bdfg21::query_sets(qs).size();  // the grouping of bgh19.rs:155-215
    blinds.resize(plan.q_index + 1 + plan.num_chunk);  // the quotient's own is formed in `open`; the chunks' follow it
  }
  size_t opening_length(size_t k) const { return 64 * k + 32 * n_sets + 160; }
  void start(Blake2bTranscript& t) { t.record_absorbed(); }  // the opening's device call continues the transcript from its bytes
  void note_blinds(size_t first, size_t count, const uint8_t* b32) {
    for (size_t i = 0; i < count; ++i)
      if (!Fr::from_bytes(b32 + 32 * i, &blinds.at(first + i))) throw Panic("non-canonical blind");
  }
  // committed instances: the verifier adds `constant` to every column's MSM, so the polynomial's blind is 1 over a constant
  // that is the key's s (anything else is no commitment of this key) and 0 without one
  Error instance_key(const InstanceCommittingKey& ick, size_t first, size_t count) {
    if (ick.constant && !(*ick.constant == s))
      return Error{Error::InvalidProtocol, "the constant of the instance_committing_key is not the key's s"};
    for (size_t i = 0; i < count; ++i) blinds.at(first + i) = ick.constant ? Fr::one() : Fr::zero();
    return Error{};
  }
  // `first`: the session's index of the first polynomial, whose blinds note_blinds has (chunk i of h: q_index + 1 + i)
  void commit(snarkv_ctx* ctx, const uint8_t* d_first, size_t n, size_t first, size_t count, uint8_t* d_out64) {
    std::vector<uint8_t> b(32 * count);
    for (size_t i = 0; i < count; ++i) blinds.at(first + i).to_bytes(&b[32 * i]);
    const int rc = snarkv_pallas_ipa_commit_blinded_batch_dev(ctx, dk, s.b, d_first, n, count, b.data(), 0, d_out64);
    if (rc == SNARKV_ERR_LENGTH) throw PlonkKeyMismatch("the key is a shard: the prover commits over the whole key of 2^k points");
    plonk_dev(rc, "ipa_commit_blinded_batch");
  }
  Error open(snarkv_ctx* ctx, const uint8_t* d_polys, size_t n, size_t q_index, const std::vector<Fr>& zn_powers, const Fr& z,
             const std::vector<Query<Fr>>& queries, const PlonkFinishBlinds* rnd, Blake2bTranscript& t) {
    if (!rnd) throw Panic("the IPA opening needs the caller's randomness");
    Fr q_blind = Fr::zero();  // blind(Q) = sum (z^n)^i blind(h_i)
    for (size_t i = 0; i < zn_powers.size(); ++i) q_blind = q_blind + zn_powers[i] * blinds.at(q_index + 1 + i);
    std::vector<Fr> below(blinds.begin(), blinds.begin() + q_index);
    below.push_back(q_blind);
    Bgh19OpenInput in{ctx, dk, &h, &s, d_polys, n, q_index + 1, &below, Fr::zero(), rnd->d_pbar32, Fr::zero()};
    if (!Fr::from_bytes(rnd->f_blind32, &in.f_blind) || !Fr::from_bytes(rnd->omega_bar32, &in.omega_bar)) throw Panic("non-canonical blind");
    auto opened = Bgh19::create_proof(in, z, queries, t);
    if (!opened.ok()) return opened.err.kind == Error::AssertionFailure ? Error::assertion(kPlonkUnsatisfied) : opened.err;
    acc = std::move(*opened.value);
    return Error{};
  }
};
#endif

template <class MOS, class TR>
struct PlonkProver : PlonkProverSession {
  using Scheme = PlonkScheme<MOS, TR>;
  static constexpr size_t kPointBytes = Scheme::kPointBytes;

  PlonkProtocol pr;
  ProverPlan plan;
  snarkv_ctx* ctx = nullptr;
  Scheme scheme;
  uint8_t* d_mem = nullptr;
  std::vector<std::vector<Fr>> instances;
  std::vector<Fr> challenges;
  TR t;
  size_t next_phase = 0, witness_done = 0;
  uint32_t flags = 0;  // kPlonk* of begin
  // byte offsets into d_mem
  size_t off_polys = 0, off_h = 0, off_work = 0, off_blk = 0;
  size_t blk_points = 0, blk_evals = 0, blk_bytes = 0;
  std::vector<int32_t> rotations;  // the distinct ones of the evaluations and the queries
  std::vector<PQuery> wanted;      // every (poly, rotation) to evaluate, the protocol's evaluations first

  static void dev(int rc, const char* what) { plonk_dev(rc, what); }
  uint8_t* col(size_t i) const { return d_mem + 32 * plan.n * i; }                      // by column of the buffer
  uint8_t* poly(size_t p) const { return d_mem + off_polys + 32 * plan.n * p; }         // by the protocol's index
  uint32_t* status() const { return (uint32_t*)(d_mem + off_blk); }
  uint8_t* commits() const { return d_mem + off_blk + 32; }

  PlonkProver() = default;
  PlonkProver(const PlonkProver&) = delete;
  ~PlonkProver() override {
    if (d_mem) Scheme::mem_free(ctx, d_mem);
  }

  // d_preprocessed: the n_pre polynomials as coefficients, n each, in the protocol's order.  `scheme` has its key already;
  // pre_blinds32: the blinds of the preprocessed polynomials' commitments (IPA; null over KZG)
  // committed_instances: plan_prover's option.  With it and a key, the n_inst instance polynomials are committed in one
  // batch (blind 1 over the key's constant, 0 without one), the points are downloaded -- ONE synchronisation, the only one of
  // begin -- and the transcript absorbs them by common_ec_point where it otherwise absorbs the scalars (proof.rs:75-108); they
  // are not proof bytes.  An identity among them is the transcript's refusal.
  Error begin(const PlonkProtocol& protocol, snarkv_ctx* c, const void* d_preprocessed, const std::vector<std::vector<Fr>>& inst,
              uint32_t session_flags = 0, const uint8_t* pre_blinds32 = nullptr, bool committed_instances = false) {
    pr = protocol;
    flags = session_flags;
    ctx = c;
    instances = inst;
    try {
      plan = plan_prover(pr, SNARKV_PLONK_DEV(ntt_max_k)(), committed_instances);
    } catch (const InvalidProtocol& e) {
      return Error{Error::InvalidProtocol, e.what()};
    }
    if (plan.k == 0) return Error{Error::InvalidProtocol, "k = 0: the polynomial X has no column of one coefficient"};
    if (pr.num_instance.size() != inst.size()) return Error{Error::InvalidInstances, ""};
    for (size_t i = 0; i < inst.size(); ++i)
      if (pr.num_instance[i] != inst[i].size() || inst[i].size() > plan.n) return Error{Error::InvalidInstances, ""};
    const size_t n = plan.n;
    // the rotations and the evaluation list
    std::set<PQuery> seen;
    for (auto* list : {&pr.evaluations, &pr.queries})
      for (auto& q : *list) {
        if (std::find(rotations.begin(), rotations.end(), q.rotation) == rotations.end()) rotations.push_back(q.rotation);
        if (q.poly != plan.q_index && seen.insert(q).second) wanted.push_back(q);
      }
    if (std::find(rotations.begin(), rotations.end(), 0) == rotations.end()) rotations.push_back(0);  // the chunks' point
    if (pr.queries.empty()) return Error{Error::InvalidProtocol, "the protocol has no queries"};
    scheme.prepare(pr, plan);
    if (pre_blinds32) scheme.note_blinds(0, plan.n_pre, pre_blinds32);
    if (plan.committed_instances) {
      Error e = scheme.instance_key(*pr.instance_committing_key, plan.n_pre, plan.n_inst);
      if (!e.ok()) return e;
    }
    // the layout
    size_t most = plan.num_chunk;
    if (plan.committed_instances) most = std::max(most, plan.n_inst);  // the point block holds the instance commitments too
    for (size_t ph = 0; ph < plan.phases; ++ph) most = std::max(most, pr.num_witness[ph]);
    off_polys = 32 * n * plan.num.first_poly;
    off_h = 32 * n * plan.cols_total();
    off_work = off_h + 32 * plan.N;
    off_blk = off_work + 32 * plan.work_elems(flags & kPlonkQuotientCosets);
    blk_points = 32 + 64 * most;
    blk_evals = blk_points + 32 * rotations.size();
    blk_bytes = blk_evals + 32 * (wanted.size() + plan.num_chunk);
    void* d = nullptr;
    dev(Scheme::mem_alloc(ctx, off_blk + blk_bytes, &d), "session_alloc");
    d_mem = (uint8_t*)d;
    // the extra columns: l_0 = (1/n, 1/n, ...) as coefficients, X = (0, 1, 0, ...)
    if (plan.num.l0_col >= 0) {
      std::vector<uint8_t> l0(32 * n);
      pr.domain.n_inv.to_bytes(l0.data());
      for (size_t i = 1; i < n; ++i) memcpy(&l0[32 * i], l0.data(), 32);
      dev(Scheme::upload(ctx, col(plan.num.l0_col), l0.data(), l0.size()), "session_upload");
    }
    if (plan.num.x_col >= 0) {
      uint8_t one[32];
      Fr::one().to_bytes(one);
      dev(Scheme::upload(ctx, col(plan.num.x_col) + 32, one, 32), "session_upload");
    }
    if (plan.n_pre) dev(Scheme::copy(ctx, poly(0), d_preprocessed, 32 * n * plan.n_pre), "session_copy");
    if (plan.n_inst) {
      std::vector<uint8_t> vals(32 * n * plan.n_inst, 0);
      for (size_t i = 0; i < inst.size(); ++i)
        for (size_t j = 0; j < inst[i].size(); ++j) inst[i][j].to_bytes(&vals[32 * (n * i + j)]);
      dev(Scheme::upload(ctx, poly(plan.n_pre), vals.data(), vals.size()), "session_upload");
      dev(SNARKV_PLONK_DEV(ntt_dev)(ctx, poly(plan.n_pre), poly(plan.n_pre), (uint32_t)plan.k, plan.n_inst, SNARKV_NTT_INVERSE, nullptr), "ntt");
    }
    // proof.rs:52-108, the prover's side
    scheme.start(t);
    if (pr.transcript_initial_state) {
      Error e = t.common_scalar(*pr.transcript_initial_state);
      if (!e.ok()) return e;
    }
    if (plan.committed_instances) {
      if (plan.n_inst == 0) return Error{};
      scheme.commit(ctx, poly(plan.n_pre), n, plan.n_pre, plan.n_inst, commits());
      std::vector<uint8_t> out(64 * plan.n_inst);
      dev(Scheme::download(ctx, out.data(), commits(), out.size()), "session_download");
      for (size_t i = 0; i < plan.n_inst; ++i) {
        Error e = t.common_ec_point(G1Affine::from_bytes(&out[64 * i]));
        if (!e.ok()) return e;
      }
      return Error{};
    }
    for (auto& column : inst)
      for (auto& x : column) {
        Error e = t.common_scalar(x);
        if (!e.ok()) return e;
      }
    return Error{};
  }

  size_t num_phases() const override { return plan.phases; }
  size_t phase_challenges(size_t ph) const override { return pr.num_challenge[ph]; }
  size_t phase_witnesses(size_t ph) const override { return pr.num_witness[ph]; }
  size_t proof_length() const override {
    return kPointBytes * (plan.n_wit + plan.num_chunk) + 32 * pr.evaluations.size() + scheme.opening_length(plan.k);
  }

  // `count` polynomials of n coefficients at d_first (the session's polynomials first ..), committed in one batch -> written
  // to the transcript
  Error commit_and_write(const uint8_t* d_first, size_t first, size_t count, uint32_t* status_out) {
    scheme.commit(ctx, d_first, plan.n, first, count, commits());
    std::vector<uint8_t> out(32 + 64 * count);
    dev(Scheme::download(ctx, out.data(), status(), out.size()), "session_download");
    if (status_out) memcpy(status_out, out.data(), 4);
    if (status_out && *status_out) return Error{};
    for (size_t i = 0; i < count; ++i) {
      Error e = t.write_ec_point(G1Affine::from_bytes(&out[32 + 64 * i]));
      if (!e.ok()) return e;
    }
    return Error{};
  }

  Result<std::vector<Fr>> phase(const void* d_witness, int form, const uint8_t* blinds32 = nullptr) override {
    using R = Result<std::vector<Fr>>;
    const size_t nw = pr.num_witness[next_phase];
    if (nw) {
      const size_t first = plan.n_pre + plan.n_inst + witness_done;
      uint8_t* dst = poly(first);
      if (blinds32) scheme.note_blinds(first, nw, blinds32);
      dev(Scheme::copy(ctx, dst, d_witness, 32 * plan.n * nw), "session_copy");
      if (form == kPlonkValues) dev(SNARKV_PLONK_DEV(ntt_dev)(ctx, dst, dst, (uint32_t)plan.k, nw, SNARKV_NTT_INVERSE, nullptr), "ntt");
      Error e = commit_and_write(dst, first, nw, nullptr);
      if (!e.ok()) return R::Err(e);
    }
    witness_done += nw;
    std::vector<Fr> out = t.squeeze_n_challenges(pr.num_challenge[next_phase]);
    challenges.insert(challenges.end(), out.begin(), out.end());
    ++next_phase;
    return R::Ok(std::move(out));
  }

  Result<std::vector<uint8_t>> finish(const PlonkFinishBlinds* rnd = nullptr) override {
    using R = Result<std::vector<uint8_t>>;
    const size_t n = plan.n, N = plan.N;
    uint8_t* d_h = d_mem + off_h;
    // 1. the quotient on the extended coset
    const Fr zeta = plonk_zeta();
    uint8_t zeta32[32], zeta_inv32[32];
    zeta.to_bytes(zeta32);
    zeta.square().to_bytes(zeta_inv32);  // zeta^3 = 1
    std::vector<uint8_t> consts;
    try {
      consts = plan.num.fill(challenges);
    } catch (const InvalidProtocol& e) {
      return R::Err(Error{Error::InvalidProtocol, e.what()});
    }
    dev((flags & kPlonkQuotientCosets ? SNARKV_PLONK_DEV(quotient_cosets_dev) : SNARKV_PLONK_DEV(quotient_dev))(ctx, d_mem, (uint32_t)plan.k, plan.num.e, plan.num.n_cols, plan.num.prog.data(), plan.num.prog.size(),
                            consts.data(), plan.num.consts.size(), zeta32, zeta_inv32, d_mem + off_work, d_h),
        "quotient");
    // 2. its coefficients from num_chunk * n on are zero, or the numerator does not vanish on the domain
    const uint32_t zero[4] = {0, 0, 0, 0};
    dev(Scheme::upload(ctx, status(), zero, 16), "session_upload");
    dev(Scheme::tail_check(ctx, d_h + 32 * n * plan.num_chunk, N - n * plan.num_chunk, status()), "tail_check");
    // 3. the chunks, committed in one batch; the status word comes with the points
    uint32_t tail = 0;
    if (rnd) scheme.note_blinds(plan.q_index + 1, plan.num_chunk, rnd->chunk_blinds32);
    Error e = commit_and_write(d_h, plan.q_index + 1, plan.num_chunk, &tail);
    if (!e.ok()) return R::Err(e);
    if (SNARKV_HOST_TRACE && tail) fprintf(stderr, "[plonk_prover] refused: h has coefficients from num_chunk * n on\n");
    if (tail) return R::Err(Error::assertion(kPlonkUnsatisfied));
    const Fr z = t.squeeze_challenge();
    // 4. every evaluation in one call: the protocol's, the queries' that are not among them, the chunks' at z
    std::vector<uint8_t> points(32 * rotations.size());
    for (size_t i = 0; i < rotations.size(); ++i) pr.domain.rotate_scalar(z, rotations[i]).to_bytes(&points[32 * i]);
    dev(Scheme::upload(ctx, d_mem + off_blk + blk_points, points.data(), points.size()), "session_upload");
    auto point_of = [&](int32_t rot) { return (uint32_t)(std::find(rotations.begin(), rotations.end(), rot) - rotations.begin()); };
    std::vector<uint32_t> q_poly, q_point;
    for (auto& q : wanted) {
      q_poly.push_back((uint32_t)q.poly);
      q_point.push_back(point_of(q.rotation));
    }
    const size_t first_chunk = plan.q_index + 1;  // h follows the quotient's slot
    for (size_t i = 0; i < plan.num_chunk; ++i) {
      q_poly.push_back((uint32_t)(first_chunk + i));
      q_point.push_back(point_of(0));
    }
    dev(SNARKV_PLONK_DEV(poly_eval_many_dev)(ctx, poly(0), n, first_chunk + plan.num_chunk, d_mem + off_blk + blk_points, rotations.size(),
                                  q_poly.data(), q_point.data(), q_poly.size(), d_mem + off_blk + blk_evals),
        "poly_eval_many");
    std::vector<uint8_t> raw(32 * q_poly.size());
    dev(Scheme::download(ctx, raw.data(), d_mem + off_blk + blk_evals, raw.size()), "session_download");
    std::map<PQuery, Fr> value;
    std::vector<Fr> chunk_at_z(plan.num_chunk);
    for (size_t i = 0; i < q_poly.size(); ++i) {
      Fr x;
      if (!Fr::from_bytes(&raw[32 * i], &x)) throw std::runtime_error("poly_eval_many: a non-canonical evaluation");
      if (i < wanted.size()) value[wanted[i]] = x;
      else chunk_at_z[i - wanted.size()] = x;
    }
    PlonkProof<MOS> proof;  // what the verifier will have read, for its own code below
    proof.challenges = challenges;
    proof.z = z;
    for (auto& q : pr.evaluations) {
      proof.evaluations.push_back(value.at(q));
      e = t.write_scalar(proof.evaluations.back());
      if (!e.ok()) return R::Err(e);
    }
    // 5. Q = sum (z^n)^i h_i into the quotient's slot
    const CommonPolyEval cpe(pr.domain, pr.langranges(), z);
    const std::vector<Fr> zn_powers = cpe.zn.powers(plan.num_chunk);
    std::vector<uint32_t> idx(plan.num_chunk);
    std::vector<uint8_t> scalars(32 * plan.num_chunk);
    Fr q_at_z = Fr::zero();
    for (size_t i = 0; i < plan.num_chunk; ++i) {
      idx[i] = (uint32_t)i;
      zn_powers[i].to_bytes(&scalars[32 * i]);
      q_at_z = q_at_z + zn_powers[i] * chunk_at_z[i];
    }
    dev(SNARKV_PLONK_DEV(poly_lincomb_dev)(ctx, d_h, n, plan.num_chunk, idx.data(), scalars.data(), plan.num_chunk, poly(plan.q_index)), "poly_lincomb");
    // 6. the verifier's identity, with the verifier's code: numerator(z) = Q(z) (z^n - 1)
    std::map<PQuery, Fr> evals = proof.evaluations_map(pr, instances, cpe);
    struct V {
      const PlonkProof<MOS>& proof;
      const CommonPolyEval& cpe;
      const std::map<PQuery, Fr>& evals;
      Fr constant(const Fr& s) { return s; }
      Fr common_identity() { return cpe.identity; }
      Fr common_lagrange(int32_t i) { return cpe.get_lagrange(i); }
      Fr poly(const PQuery& q) {
        auto it = evals.find(q);
        if (it == evals.end()) throw InvalidProtocol("Missing query");
        return it->second;
      }
      Fr challenge(size_t i) {
        if (i >= proof.challenges.size()) throw InvalidProtocol("Missing challenge");
        return proof.challenges[i];
      }
      Fr negated(const Fr& a) { return -a; }
      Fr sum(const Fr& a, const Fr& b) { return a + b; }
      Fr product(const Fr& a, const Fr& b) { return a * b; }
      Fr scaled(const Fr& a, const Fr& s) { return a * s; }
    } v{proof, cpe, evals};
    Fr numerator;
    try {
      numerator = expr_evaluate<Fr>(*pr.quotient.numerator, v);
    } catch (const InvalidProtocol& ex) {
      return R::Err(Error{Error::InvalidProtocol, ex.what()});
    }
    if (SNARKV_HOST_TRACE && numerator != q_at_z * cpe.zn_minus_one) fprintf(stderr, "[plonk_prover] refused: numerator(z) != Q(z) (z^n - 1)\n");
    if (numerator != q_at_z * cpe.zn_minus_one) return R::Err(Error::assertion(kPlonkUnsatisfied));
    // 7. the opening
    std::vector<Query<Fr>> queries;
    for (auto& q : pr.queries)
      queries.push_back(Query<Fr>{q.poly, pr.domain.rotate_scalar(Fr::one(), q.rotation), q.poly == plan.q_index ? q_at_z : value.at(q)});
    e = scheme.open(ctx, poly(0), n, plan.q_index, zn_powers, z, queries, rnd, t);
    if (SNARKV_HOST_TRACE && !e.ok()) fprintf(stderr, "[plonk_prover] refused by the opening: %s\n", e.msg.c_str());
    if (!e.ok()) return R::Err(e);
    // 8. the bytes
    return R::Ok(t.stream());
  }
};

}  // namespace snarkv_host
