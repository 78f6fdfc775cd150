// The PLONK prover session on pallas behind a handle -> libsnarkv_host_pallas_plonk_prove.so
// (include/snarkv_host_pallas_plonk_prove.h), compiled with -DSNARKV_HOST_PALLAS like capi_pallas.cpp and linked against
// libsnarkv_host_pallas.so and libsnarkv_pallas.so.  Thin, as capi.cpp's half for KZG is: argument checks, then
// `PlonkProver<Bgh19, Blake2bTranscript>` of plonk_prover.hpp, and `Result<_, Error>` / panics mapped to return codes.
#ifndef SNARKV_HOST_PALLAS
#error "compile with -DSNARKV_HOST_PALLAS"
#endif
// capi_pallas_plonk_prove_ci.cpp includes this file under other names (PROVER_T, PROVER_FN) with PROVER_CI true: the same
// session with plan_prover's committed-instances option on -> libsnarkv_host_pallas_plonk_prove_ci.so.
#ifndef PROVER_T
#include "../../include/snarkv_host_pallas_plonk_prove.h"
#define PROVER_T snarkv_host_pallas_plonk_prover
#define PROVER_FN(name) snarkv_host_pallas_plonk_prover_##name
#define PROVER_CI false
#endif

#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "capi_pallas_handles.hpp"
#include "plonk_prover.hpp"
#include "wire.hpp"

using namespace snarkv_host;

struct PROVER_T {
  PlonkProver<Bgh19, Blake2bTranscript> s;
  size_t next_phase = 0;
  bool closed = false;  // finish has returned a verdict, or a call has failed past its argument checks: only destroy is left
};

namespace {
thread_local std::string g_last_error;

static_assert(SNARKV_HOST_PALLAS_PLONK_QUOTIENT_COSETS == kPlonkQuotientCosets, "one flag word for both flavours");

int error_code(const Error& e) {
  g_last_error = e.msg;
  switch (e.kind) {
    case Error::Transcript: return SNARKV_HOST_ERR_TRANSCRIPT;
    case Error::InvalidInstances: return SNARKV_HOST_ERR_INVALID_INSTANCES;
    case Error::InvalidProtocol: return SNARKV_HOST_ERR_INVALID_PROTOCOL;
    case Error::AssertionFailure: return 0;
    default: return SNARKV_HOST_ERR_OTHER;
  }
}

int arg_error(const char* what) {
  g_last_error = what;
  return SNARKV_HOST_ERR_ARG;
}

template <class F>
int guarded(F&& f) {
  try {
    return f();
  } catch (const Panic& e) {
    g_last_error = std::string("panic: ") + e.what();
    return SNARKV_HOST_ERR_PANIC;
  } catch (const PlonkKeyMismatch& e) {
    return arg_error(e.what());
  } catch (const std::exception& e) {
    g_last_error = e.what();
    return SNARKV_HOST_ERR_DEVICE;
  }
}
}  // namespace

extern "C" {

const char* PROVER_FN(last_error)(void) { return g_last_error.c_str(); }

int PROVER_FN(plan)(const snarkv_host_pallas_protocol* protocol, uint32_t flags, uint32_t* e, size_t* n_cols,
                                         size_t* n_instr, size_t* n_consts, size_t* bytes) {
  if (!protocol) return arg_error("null argument");
  if (flags & ~kPlonkKnownFlags) return arg_error("unknown flag bit");
  return guarded([&] {
    try {
      const ProverPlan plan = plan_prover(protocol->pr, snarkv_pallas_ntt_max_k(), PROVER_CI);
      if (e) *e = plan.num.e;
      if (n_cols) *n_cols = plan.num.n_cols;
      if (n_instr) *n_instr = plan.num.prog.size();
      if (n_consts) *n_consts = plan.num.consts.size();
      if (bytes) *bytes = plan.device_bytes_of(flags & kPlonkQuotientCosets);
      return 1;
    } catch (const InvalidProtocol& ex) {
      return error_code(Error{Error::InvalidProtocol, ex.what()});
    }
  });
}

int PROVER_FN(begin)(const snarkv_host_pallas_protocol* protocol, uint32_t flags, snarkv_ctx* ctx,
                                          const snarkv_ipa_dk* dk, const uint8_t h64[64], const uint8_t s64[64],
                                          const void* d_preprocessed32, const uint8_t* pre_blinds32, const uint8_t* instances,
                                          size_t instances_len, PROVER_T** out) {
  if (!out) return arg_error("null argument");
  *out = nullptr;
  if (!protocol || !ctx || !dk || !instances) return arg_error("null argument");
  if (!h64 || !s64) return arg_error("null argument: h and s are both required, the scheme is always zero-knowledge");
  if ((!d_preprocessed32 || !pre_blinds32) && !protocol->pr.preprocessed.empty())
    return arg_error("null argument: the preprocessed polynomials come with their blinds");
  if ((uintptr_t)d_preprocessed32 % 16) return arg_error("a device address is not 16-byte aligned");
  if (flags & ~kPlonkKnownFlags) return arg_error("unknown flag bit");
  if (snarkv_pallas_ipa_dk_k(dk) != protocol->pr.domain.k) return arg_error("the key is not one of 2^k points with k the protocol's");
  return guarded([&] {
    const std::vector<std::vector<Fr>> inst = wire::parse_instances(instances, instances_len);
    auto p = std::make_unique<PROVER_T>();
    p->s.scheme.dk = dk;
    p->s.scheme.h = G1Affine::from_bytes(h64);
    p->s.scheme.s = G1Affine::from_bytes(s64);
    const Error e = p->s.begin(protocol->pr, ctx, d_preprocessed32, inst, flags, pre_blinds32, PROVER_CI);
    if (!e.ok()) return e.kind == Error::AssertionFailure ? SNARKV_HOST_ERR_OTHER : error_code(e);
    *out = p.release();
    return 1;
  });
}

int PROVER_FN(phase)(PROVER_T* p, const void* d_witness32, int form,
                                          const uint8_t* blinds32, uint8_t* challenges_out32, size_t cap, size_t* n_challenges) {
  if (!p || !n_challenges) return arg_error("null argument");
  *n_challenges = 0;
  if (p->closed) return arg_error("the session has ended: only destroy is accepted");
  if (p->next_phase >= p->s.num_phases()) return arg_error("every phase has been given: finish comes next");
  if (form != SNARKV_HOST_PALLAS_PLONK_COEFFS && form != SNARKV_HOST_PALLAS_PLONK_VALUES)
    return arg_error("unknown form of the witness polynomials");
  const size_t want = p->s.phase_challenges(p->next_phase);
  *n_challenges = want;
  if ((!d_witness32 || !blinds32) && p->s.phase_witnesses(p->next_phase)) return arg_error("null argument: the witness polynomials come with their blinds");
  if ((uintptr_t)d_witness32 % 16) return arg_error("a device address is not 16-byte aligned");
  if (want && !challenges_out32) return arg_error("null argument");
  if (cap < want) {
    g_last_error = "challenge buffer too small";
    return SNARKV_HOST_ERR_CAPACITY;
  }
  const int rc = guarded([&] {
    auto r = p->s.phase(d_witness32, form, blinds32);
    if (!r.ok()) return r.err.kind == Error::AssertionFailure ? SNARKV_HOST_ERR_OTHER : error_code(r.err);
    for (size_t i = 0; i < r.value->size(); ++i) (*r.value)[i].to_bytes(challenges_out32 + 32 * i);
    return 1;
  });
  if (rc == 1) ++p->next_phase;
  else p->closed = true;
  return rc;
}

int PROVER_FN(finish)(PROVER_T* p, const uint8_t* chunk_blinds32,
                                           const uint8_t f_blind32[32], const void* d_pbar32, const uint8_t omega_bar32[32],
                                           uint8_t* proof_out, size_t proof_cap, size_t* proof_len, uint8_t* acc_out) {
  if (!p || !proof_len) return arg_error("null argument");
  *proof_len = 0;
  if (p->closed) return arg_error("the session has ended: only destroy is accepted");
  if (p->next_phase < p->s.num_phases()) return arg_error("finish comes after the last phase");
  const size_t need = p->s.proof_length();
  if (proof_cap < need) {
    *proof_len = need;
    g_last_error = "proof buffer too small";
    return SNARKV_HOST_ERR_CAPACITY;
  }
  if (!proof_out || !acc_out || !chunk_blinds32 || !f_blind32 || !d_pbar32 || !omega_bar32) return arg_error("null argument");
  if ((uintptr_t)d_pbar32 % 16) return arg_error("a device address is not 16-byte aligned");
  p->closed = true;
  return guarded([&] {
    const PlonkFinishBlinds rnd{chunk_blinds32, f_blind32, d_pbar32, omega_bar32};
    auto r = p->s.finish(&rnd);
    if (!r.ok()) return error_code(r.err);  // an assertion failure is 0: the witness does not satisfy the constraints
    if (r.value->size() != need || !p->s.scheme.acc) throw std::runtime_error("the proof is not of the length the protocol gives");
    memcpy(proof_out, r.value->data(), need);
    const IpaAccumulator& acc = *p->s.scheme.acc;
    for (size_t j = 0; j < acc.xi.size(); ++j) acc.xi[j].to_bytes(acc_out + 32 * j);
    memcpy(acc_out + 32 * acc.xi.size(), acc.u.b, 64);
    *proof_len = need;
    return 1;
  });
}

void PROVER_FN(destroy)(PROVER_T* p) { delete p; }

}  // extern "C"
