// C ABI of the pasta flavour of the host mirror -> libsnarkv_host_pallas.so (include/snarkv_host_pallas.h), compiled
// with -DSNARKV_HOST_PALLAS: `Fr` = pallas::Scalar, the loader bound to libsnarkv_pallas.so.  Thin, as capi.cpp is:
// every function parses its byte arguments, calls the C++ mirror of the reference API (plonk.hpp / ipa.hpp /
// plonk_ipa_batch.hpp) and maps `Result<_, Error>` / panics to return codes.
#ifndef SNARKV_HOST_PALLAS
#error "compile with -DSNARKV_HOST_PALLAS"
#endif
#include "../../include/snarkv_host_pallas.h"

#include <chrono>
#include <cstring>
#include <string>

#include "blake2b_transcript.hpp"
#include "capi_pallas_handles.hpp"
#include "ipa.hpp"
#include "plonk.hpp"
#include "plonk_ipa_batch.hpp"
#include "wire.hpp"

using namespace snarkv_host;


namespace {
thread_local std::string g_last_error;

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

template <class F>
int guarded(F&& f) {
  try {
    return f();
  } catch (const Panic& e) {
    g_last_error = std::string("panic: ") + e.what();
    return SNARKV_HOST_ERR_PANIC;
  } catch (const std::exception& e) {
    g_last_error = e.what();
    return SNARKV_HOST_ERR_DEVICE;
  }
}

int arg_error(const char* what) {
  g_last_error = what;
  return SNARKV_HOST_ERR_ARG;
}

bool route_of(int decompress, IpaDecompress* out) {
  switch (decompress) {
    case SNARKV_HOST_PALLAS_DECOMPRESS_HOST: *out = IpaDecompress::Host; return true;
    case SNARKV_HOST_PALLAS_DECOMPRESS_DEVICE: *out = IpaDecompress::Device; return true;
    case SNARKV_HOST_PALLAS_DECOMPRESS_AUTO: *out = IpaDecompress::Auto; return true;
    default: return false;
  }
}

// accumulator bytes: k x xi (32 LE) | u (64)
size_t acc_stride(const IpaDecidingKey& dk) { return 32 * dk.svk.k + 64; }
std::vector<IpaAccumulator> accs_from_bytes(const IpaDecidingKey& dk, const uint8_t* b, uint32_t m) {
  const size_t k = dk.svk.k, stride = acc_stride(dk);
  std::vector<IpaAccumulator> out(m);
  for (uint32_t i = 0; i < m; ++i) {
    out[i].xi.resize(k);
    for (size_t j = 0; j < k; ++j)
      if (!Fr::from_bytes(b + i * stride + 32 * j, &out[i].xi[j])) throw Panic("non-canonical challenge in an accumulator");
    out[i].u = G1Affine::from_bytes(b + i * stride + 32 * k);
  }
  return out;
}
void put_acc(const IpaAccumulator& a, uint8_t* out) {
  for (size_t j = 0; j < a.xi.size(); ++j) a.xi[j].to_bytes(out + 32 * j);
  memcpy(out + 32 * a.xi.size(), a.u.b, 64);
}

std::function<Fr()> rng_of(const uint8_t* rand32, size_t n_rand, size_t* used) {
  return [=]() {
    if (*used >= n_rand) throw Panic("IpaAs::create_proof: rand32 ran out of scalars");
    Fr v;
    if (!Fr::from_bytes(rand32 + 32 * (*used)++, &v)) throw Panic("IpaAs::create_proof: non-canonical scalar in rand32");
    return v;
  };
}

double ms_since(std::chrono::steady_clock::time_point t0) {
  return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
}

// N x {read_proof, succinct verify}: 1 and the accumulators, or the first error's code.  t_ms (optional): read, verify.
int succinct_verify_batch(const PlonkProtocol& pr, const IpaDecidingKey& dk, const uint8_t* instances, size_t ilen,
                          const uint8_t* proofs, size_t prlen, uint32_t n, unsigned threads, IpaDecompress route,
                          std::vector<IpaAccumulator>& out, double* t_ms = nullptr) {
  const auto t0 = std::chrono::steady_clock::now();
  std::vector<std::vector<std::vector<Fr>>> insts;
  std::vector<std::vector<uint8_t>> pbytes;
  wire::split_batch(instances, ilen, proofs, prlen, n, insts, pbytes);
  if (threads == 0) threads = HostPool::get().size() + 1;
  std::vector<PlonkProof<Bgh19>> pfs;
  Error e = plonk_ipa_read_batch(dk.svk, pr, insts, pbytes, threads, route, pfs);
  if (t_ms) t_ms[0] = ms_since(t0);
  if (!e.ok()) return error_code(e);
  const auto t1 = std::chrono::steady_clock::now();
  std::vector<const PlonkProtocol*> prs(n, &pr);
  auto accs = plonk_ipa_verify_batch(dk.svk, prs, insts, pfs, threads);
  if (t_ms) t_ms[1] = ms_since(t1);
  if (!accs.ok()) return error_code(accs.err);
  out = std::move(*accs.value);
  return 1;
}

// `decide_all` with the verdict of every accumulator (IpaAs::decide_all stops at "all or not")
int decide_all(const IpaDecidingKey& dk, const std::vector<IpaAccumulator>& accs, uint8_t* ok_out) {
  if (accs.empty()) return 1;  // decide_all of nothing is Ok(()) (decider.rs:57-66)
  const size_t k = dk.svk.k;
  std::vector<uint8_t> xi(accs.size() * k * 32), u(accs.size() * 64), ok(accs.size());
  for (size_t a = 0; a < accs.size(); ++a) {
    for (size_t j = 0; j < k; ++j) accs[a].xi[j].to_bytes(&xi[(a * k + j) * 32]);
    memcpy(&u[64 * a], accs[a].u.b, 64);
  }
  snarkv_ipa_dk* h = dk.handle();
  {
    DeviceScope lock;
    if (pallas_ipa_decide_batch(h, xi.data(), u.data(), accs.size(), ok.data()) != SNARKV_OK)
      throw std::runtime_error(std::string("pallas_ipa_decide_batch: ") + snarkv_pallas_last_error());
  }
  if (ok_out) memcpy(ok_out, ok.data(), ok.size());
  for (uint8_t b : ok)
    if (!b) return error_code(Error::assertion("U == commit(G, h)"));
  return 1;
}

int copy_out(const std::vector<uint8_t>& b, uint8_t* out, size_t cap, size_t* len_out, const char* what) {
  if (len_out) *len_out = b.size();
  if (b.size() > cap || (b.size() && !out)) {
    g_last_error = what;
    return SNARKV_HOST_ERR_CAPACITY;
  }
  if (!b.empty()) memcpy(out, b.data(), b.size());
  return 1;
}
}  // namespace

extern "C" {

const char* snarkv_host_pallas_last_error(void) { return g_last_error.c_str(); }

int snarkv_host_pallas_protocol_parse(const uint8_t* bytes, size_t len, snarkv_host_pallas_protocol** out) {
  if (!bytes || !out) return arg_error("null argument");
  *out = nullptr;
  return guarded([&] {
    *out = new snarkv_host_pallas_protocol{wire::parse_protocol(bytes, len)};
    return 1;
  });
}
void snarkv_host_pallas_protocol_free(snarkv_host_pallas_protocol* p) { delete p; }

int snarkv_host_pallas_ipa_dk_create(uint32_t k, const uint8_t* g_points64, const uint8_t h[64], const uint8_t* s_or_null,
                                     snarkv_host_pallas_ipa_dk** out) {
  if (!g_points64 || !h || !out) return arg_error("null argument");
  *out = nullptr;
  if (k == 0 || k > 28) return arg_error("k out of range");
  return guarded([&] {
    auto d = std::make_unique<snarkv_host_pallas_ipa_dk>();
    const size_t n = (size_t)1 << k;
    d->dk.svk.k = k;
    d->dk.g.resize(n);
    for (size_t i = 0; i < n; ++i) d->dk.g[i] = G1Affine::from_bytes(g_points64 + 64 * i);
    d->dk.svk.g = d->dk.g[0];
    d->dk.svk.h = G1Affine::from_bytes(h);
    if (s_or_null) d->dk.svk.s = G1Affine::from_bytes(s_or_null);
    d->dk.handle();  // the committing key goes to the device now: per-key setup, not per-call work
    *out = d.release();
    return 1;
  });
}
void snarkv_host_pallas_ipa_dk_free(snarkv_host_pallas_ipa_dk* dk) { delete dk; }

int snarkv_host_pallas_plonk_succinct_verify_batch(const snarkv_host_pallas_protocol* protocol,
                                                   const snarkv_host_pallas_ipa_dk* dk, const uint8_t* instances,
                                                   size_t instances_len, const uint8_t* proofs, size_t proofs_len,
                                                   uint32_t n, unsigned host_threads, int decompress, uint8_t* accs_out,
                                                   size_t accs_cap) {
  IpaDecompress route;
  if (!route_of(decompress, &route)) return arg_error("unknown decompress route");
  if (!protocol || !dk || (n && (!instances || !proofs))) return arg_error("null argument");
  return guarded([&] {
    std::vector<IpaAccumulator> accs;
    int rc = succinct_verify_batch(protocol->pr, dk->dk, instances, instances_len, proofs, proofs_len, n, host_threads, route, accs);
    if (rc != 1) return rc;
    const size_t stride = acc_stride(dk->dk);
    if (accs_out) {
      if (stride * accs.size() > accs_cap) {
        g_last_error = "accumulator buffer too small";
        return SNARKV_HOST_ERR_CAPACITY;
      }
      for (size_t i = 0; i < accs.size(); ++i) put_acc(accs[i], accs_out + i * stride);
    }
    return 1;
  });
}

int snarkv_host_pallas_ipa_decide_all(const snarkv_host_pallas_ipa_dk* dk, const uint8_t* accs, uint32_t m, uint8_t* ok_out) {
  if (!dk || (m && !accs)) return arg_error("null argument");
  return guarded([&] { return decide_all(dk->dk, accs_from_bytes(dk->dk, accs, m), ok_out); });
}

int snarkv_host_pallas_plonk_verify(const snarkv_host_pallas_protocol* protocol, const snarkv_host_pallas_ipa_dk* dk,
                                    const uint8_t* instances, size_t instances_len, const uint8_t* proofs,
                                    size_t proofs_len, uint32_t n, unsigned host_threads, int decompress) {
  IpaDecompress route;
  if (!route_of(decompress, &route)) return arg_error("unknown decompress route");
  if (!protocol || !dk || (n && (!instances || !proofs))) return arg_error("null argument");
  return guarded([&] {
    std::vector<IpaAccumulator> accs;
    int rc = succinct_verify_batch(protocol->pr, dk->dk, instances, instances_len, proofs, proofs_len, n, host_threads, route, accs);
    if (rc != 1) return rc;
    return decide_all(dk->dk, accs, nullptr);
  });
}

int snarkv_host_pallas_ipa_as_create_proof(const snarkv_host_pallas_ipa_dk* dk, const uint8_t* accs, uint32_t m,
                                           const uint8_t* rand32, size_t n_rand, uint8_t* proof_out, size_t proof_cap,
                                           size_t* proof_len, uint8_t* acc_out) {
  if (!dk || !accs || !acc_out || (n_rand && !rand32)) return arg_error("null argument");
  return guarded([&] {
    auto instances = accs_from_bytes(dk->dk, accs, m);
    size_t used = 0;
    Blake2bTranscript t;
    auto acc = IpaAs<Bgh19>::create_proof(dk->dk, instances, t, rng_of(rand32, n_rand, &used));
    if (!acc.ok()) return error_code(acc.err);
    int rc = copy_out(t.finalize(), proof_out, proof_cap, proof_len, "proof buffer too small");
    if (rc != 1) return rc;
    put_acc(*acc.value, acc_out);
    return 1;
  });
}

int snarkv_host_pallas_ipa_as_verify(const snarkv_host_pallas_ipa_dk* dk, const uint8_t* accs, uint32_t m,
                                     const uint8_t* proof, size_t proof_len, uint8_t* acc_out) {
  if (!dk || !accs || !acc_out || (proof_len && !proof)) return arg_error("null argument");
  return guarded([&] {
    auto instances = accs_from_bytes(dk->dk, accs, m);
    Blake2bTranscript t(proof_len ? std::vector<uint8_t>(proof, proof + proof_len) : std::vector<uint8_t>());
    auto pf = IpaAs<Bgh19>::read_proof(dk->dk.svk, instances, t);
    if (!pf.ok()) return error_code(pf.err);
    if (t.remaining() != 0) {
      g_last_error = "trailing bytes after the accumulation proof";
      return SNARKV_HOST_ERR_TRAILING;
    }
    auto acc = IpaAs<Bgh19>::verify(dk->dk.svk, instances, *pf.value);
    if (!acc.ok()) return error_code(acc.err);
    put_acc(*acc.value, acc_out);
    return 1;
  });
}

int snarkv_host_pallas_aggregate(const snarkv_host_pallas_protocol* protocol, const snarkv_host_pallas_ipa_dk* dk,
                                 const uint8_t* instances, size_t instances_len, const uint8_t* proofs, size_t proofs_len,
                                 uint32_t n, unsigned host_threads, int decompress, const uint8_t* rand32, size_t n_rand,
                                 double* timings_ms, uint8_t* as_proof_out, size_t as_proof_cap, size_t* as_proof_len,
                                 uint8_t* acc_out) {
  IpaDecompress route;
  if (!route_of(decompress, &route)) return arg_error("unknown decompress route");
  if (!protocol || !dk || !instances || !proofs || n == 0 || (n_rand && !rand32)) return arg_error("null argument");
  const auto t0 = std::chrono::steady_clock::now();
  double tm[5] = {0, 0, 0, 0, 0};
  const int rc = guarded([&] {
    std::vector<IpaAccumulator> accs;
    int rc = succinct_verify_batch(protocol->pr, dk->dk, instances, instances_len, proofs, proofs_len, n, host_threads, route, accs, tm);
    if (rc != 1) return rc;
    IpaAccumulator acc;
    std::vector<uint8_t> as_proof;
    if (accs.size() == 1) {  // nothing to accumulate (the SDK's `aggregate`, aggregation.rs:121-137)
      acc = accs[0];
    } else {
      const auto t1 = std::chrono::steady_clock::now();
      size_t used = 0;
      Blake2bTranscript t;
      auto r = IpaAs<Bgh19>::create_proof(dk->dk, accs, t, rng_of(rand32, n_rand, &used));
      tm[2] = ms_since(t1);
      if (!r.ok()) return error_code(r.err);
      acc = std::move(*r.value);
      as_proof = t.finalize();
    }
    if (as_proof_len) *as_proof_len = as_proof.size();
    if (as_proof_out) {
      rc = copy_out(as_proof, as_proof_out, as_proof_cap, as_proof_len, "accumulation proof buffer too small");
      if (rc != 1) return rc;
    }
    if (acc_out) put_acc(acc, acc_out);
    const auto t2 = std::chrono::steady_clock::now();
    rc = decide_all(dk->dk, {acc}, nullptr);
    tm[3] = ms_since(t2);
    return rc;
  });
  // whatever the outcome: the stages that ran (a stage not reached, or left by an exception, stays 0) and the total
  tm[4] = ms_since(t0);
  if (timings_ms) memcpy(timings_ms, tm, sizeof tm);
  return rc;
}

}  // extern "C"
