// Test-driver entry points of the IPA layer (host/ipa.hpp), shared by the BN254 driver (test_driver.cpp:
// hd_ipa_*) and the pasta flavour (test_driver_pallas.cpp: hp_ipa_*).  The including file provides
// `guarded`, `error_code`, `make_transcript(tkind, proof, len)`, the readers of driver_parse.inc and SNARKV_DRV(name).
// ---- IPA (pcs/ipa.rs, pcs/ipa/{accumulation,decider}.rs) ----------------------------------------
//   svk        : k(u32) | zk(u32) | g0(64) | h(64) | s(64, only when zk)
//   accumulator: k x xi(32 LE) | u(64)
// Returns 1 = the check passed, 0 = `Error::AssertionFailure`, -10 Transcript, -100 panic.
namespace {
IpaSuccinctVerifyingKey parse_ipa_svk(const uint8_t* b) {
  IpaSuccinctVerifyingKey svk;
  uint32_t k, zk;
  memcpy(&k, b, 4);
  memcpy(&zk, b + 4, 4);
  svk.k = k;
  svk.g = G1Affine::from_bytes(b + 8);
  svk.h = G1Affine::from_bytes(b + 72);
  if (zk) svk.s = G1Affine::from_bytes(b + 136);
  return svk;
}
bool parse_ipa_accs(const uint8_t* b, size_t k, uint32_t m, std::vector<IpaAccumulator>* out) {
  const size_t stride = 32 * k + 64;
  for (uint32_t i = 0; i < m; ++i) {
    IpaAccumulator a;
    a.xi.resize(k);
    for (size_t j = 0; j < k; ++j)
      if (!Fr::from_bytes(b + i * stride + 32 * j, &a.xi[j])) return false;
    a.u = G1Affine::from_bytes(b + i * stride + 32 * k);
    out->push_back(std::move(a));
  }
  return true;
}
void put_ipa_acc(const IpaAccumulator& a, uint8_t* out) {
  for (size_t j = 0; j < a.xi.size(); ++j) a.xi[j].to_bytes(out + 32 * j);
  memcpy(out + 32 * a.xi.size(), a.u.b, 64);
}
}  // namespace

// `Ipa::read_proof` + `Ipa::succinct_verify` of ONE opening of `commitment` at z with value `eval`
extern "C" int SNARKV_DRV(ipa_succinct_verify)(int tkind, const uint8_t* svk_bytes, const uint8_t* commitment64,
                                      const uint8_t* z32, const uint8_t* eval32, const uint8_t* proof, size_t plen,
                                      uint8_t* acc_out) {
  return guarded([&] {
    IpaSuccinctVerifyingKey svk = parse_ipa_svk(svk_bytes);
    Fr z, ev;
    if (!Fr::from_bytes(z32, &z) || !Fr::from_bytes(eval32, &ev)) return -3;
    G1Affine c = G1Affine::from_bytes(commitment64);
    auto t = make_transcript(tkind, proof, plen);
    auto pr = Ipa::read_proof(svk, *t);
    if (!pr.ok()) return error_code(pr.err);
    auto acc = Ipa::succinct_verify(svk, MsmT::base(&c), z, ev, *pr.value);
    if (!acc.ok()) return error_code(acc.err);
    put_ipa_acc(*acc.value, acc_out);
    return 1;
  });
}

// `IpaAs::read_proof` + `IpaAs::verify` over m old accumulators
extern "C" int SNARKV_DRV(ipa_as_verify)(int tkind, const uint8_t* svk_bytes, const uint8_t* accs, uint32_t m,
                                const uint8_t* proof, size_t plen, uint8_t* acc_out) {
  return guarded([&] {
    IpaSuccinctVerifyingKey svk = parse_ipa_svk(svk_bytes);
    std::vector<IpaAccumulator> instances;
    if (!parse_ipa_accs(accs, svk.k, m, &instances)) return -3;
    auto t = make_transcript(tkind, proof, plen);
    auto pr = IpaAs<>::read_proof(svk, instances, *t);
    if (!pr.ok()) return error_code(pr.err);
    auto acc = IpaAs<>::verify(svk, instances, *pr.value);
    if (!acc.ok()) return error_code(acc.err);
    put_ipa_acc(*acc.value, acc_out);
    return 1;
  });
}

// `IpaAs::decide_all`: g = 2^k committing-key points (64 B each)
extern "C" int SNARKV_DRV(ipa_decide_all)(uint32_t k, const uint8_t* g, size_t n_g, const uint8_t* accs, uint32_t m) {
  return guarded([&] {
    IpaDecidingKey dk;
    dk.svk.k = k;
    dk.g.resize(n_g);
    for (size_t i = 0; i < n_g; ++i) dk.g[i] = G1Affine::from_bytes(g + 64 * i);
    std::vector<IpaAccumulator> instances;
    if (!parse_ipa_accs(accs, k, m, &instances)) return -3;
    return IpaAs<>::decide_all(dk, instances).ok() ? 1 : 0;
  });
}

// h_eval / h_coeffs hooks: out = h_eval(xi, z) (32) || h_coeffs(xi, 1) (2^k x 32)
extern "C" int SNARKV_DRV(ipa_h)(uint32_t k, const uint8_t* xi32, const uint8_t* z32, uint8_t* out) {
  return guarded([&] {
    std::vector<Fr> xi(k);
    Fr z;
    for (uint32_t i = 0; i < k; ++i)
      if (!Fr::from_bytes(xi32 + 32 * i, &xi[i])) return -3;
    if (!Fr::from_bytes(z32, &z)) return -3;
    h_eval(xi, z).to_bytes(out);
    auto h = h_coeffs(xi, Fr::one());
    for (size_t i = 0; i < h.size(); ++i) h[i].to_bytes(out + 32 + 32 * i);
    return 0;
  });
}

// `IpaAs<Bgh19>` as a PolynomialCommitmentScheme (bgh19.rs:26-96): read_proof + verify.
//   commitments: pack_commitments format (the Msm list);  queries: pack_queries format
extern "C" int SNARKV_DRV(ipa_bgh19_verify)(int tkind, const uint8_t* svk_bytes, const uint8_t* commitments, const uint8_t* x32,
                                   const uint8_t* queries, const uint8_t* proof, size_t plen, uint8_t* acc_out) {
  return guarded([&] {
    IpaSuccinctVerifyingKey svk = parse_ipa_svk(svk_bytes);
    Reader rc{commitments}, rq{queries};
    std::vector<std::vector<G1Affine>> store;
    std::vector<MsmT> cms;
    read_commitments(rc, store, cms);
    auto qs = read_queries(rq);
    Fr x;
    if (!Fr::from_bytes(x32, &x)) return -3;
    auto t = make_transcript(tkind, proof, plen);
    auto pr = IpaBgh19::read_proof(svk, qs, *t);
    if (!pr.ok()) return error_code(pr.err);
    auto acc = IpaBgh19::verify(svk, cms, x, qs, *pr.value);
    if (!acc.ok()) return error_code(acc.err);
    put_ipa_acc(*acc.value, acc_out);
    return 1;
  });
}

// `PlonkVerifier<IpaAs<Bgh19>>::{read_proof, verify}` (verifier/plonk.rs:94-147; the reference's
// system/halo2/test/ipa/native.rs flow): succinct verify -> IpaAccumulator -> `decide_all` (one device
// Pippenger over the 2^k committing-key points).  acc_out (if non-null): k x xi | u.
// Returns 1 accept, 0 reject (succinct check or decide failed), -10 Transcript, -11 InvalidInstances.
extern "C" int SNARKV_DRV(plonk_ipa_verify)(int tkind, const uint8_t* protocol, size_t plen, const uint8_t* instances, size_t ilen,
                                   const uint8_t* proof, size_t prlen, const uint8_t* svk_bytes, const uint8_t* g,
                                   size_t n_g, uint8_t* acc_out, int decide) {
  return guarded([&] {
    PlonkProtocol pr = parse_protocol(protocol, plen);
    IpaDecidingKey dk;
    dk.svk = parse_ipa_svk(svk_bytes);
    dk.g.resize(n_g);
    for (size_t i = 0; i < n_g; ++i) dk.g[i] = G1Affine::from_bytes(g + 64 * i);
    auto insts = parse_instances(instances, ilen);
    auto t = make_transcript(tkind, proof, prlen);
    auto pf = PlonkVerifier<Bgh19>::read_proof(dk, pr, insts, *t);
    if (!pf.ok()) return error_code(pf.err);
    auto accs = PlonkSuccinctVerifier<Bgh19>::verify(dk.svk, pr, insts, *pf.value);
    if (!accs.ok()) return error_code(accs.err);
    if (acc_out) put_ipa_acc((*accs.value)[0], acc_out);
    if (!decide) return 1;
    return PlonkVerifier<Bgh19>::verify(dk, pr, insts, *pf.value).ok() ? 1 : 0;
  });
}

// N proofs of ONE protocol over `IpaAs<Bgh19>`: read all, all succinct-check MSMs in ONE segmented launch
// (plonk_ipa_verify_batch), then `decide_all` over the N accumulators (four in flight on the device).
//   proofs: N x (u32 len || bytes);  instances: N x packed instances, concatenated
// accs_out (if non-null): N x (k x xi | u).  Returns 1 accept, 0 reject, -10 Transcript, -11 InvalidInstances.
extern "C" int SNARKV_DRV(plonk_ipa_verify_batch)(int tkind, const uint8_t* protocol, size_t plen, const uint8_t* instances,
                                                  size_t ilen, const uint8_t* proofs, size_t prlen, uint32_t n,
                                                  const uint8_t* svk_bytes, const uint8_t* g, size_t n_g, unsigned threads,
                                                  uint8_t* accs_out, int decide) {
  return guarded([&] {
    PlonkProtocol pr = parse_protocol(protocol, plen);
    IpaDecidingKey dk;
    dk.svk = parse_ipa_svk(svk_bytes);
    dk.g.resize(n_g);
    for (size_t i = 0; i < n_g; ++i) dk.g[i] = G1Affine::from_bytes(g + 64 * i);
    std::vector<std::vector<std::vector<Fr>>> insts;
    std::vector<PlonkProof<Bgh19>> pfs;
    std::vector<const PlonkProtocol*> prs(n, &pr);
    PReader ird{instances, instances + ilen};
    const uint8_t* pp = proofs;
    for (uint32_t i = 0; i < n; ++i) {
      const uint8_t* ip = ird.p;  // one proof's instances: u32 columns, then per column u32 count + values
      for (uint32_t cols = ird.u32(), c = 0; c < cols; ++c)
        for (uint32_t m = ird.u32(), j = 0; j < m; ++j) ird.fr();
      insts.push_back(parse_instances(ip, (size_t)(ird.p - ip)));
      if (pp + 4 > proofs + prlen) return -10;
      uint32_t len;
      memcpy(&len, pp, 4);
      pp += 4;
      if (pp + len > proofs + prlen) return -10;
      auto t = make_transcript(tkind, pp, len);
      pp += len;
      auto pf = PlonkVerifier<Bgh19>::read_proof(dk, pr, insts.back(), *t);
      if (!pf.ok()) return error_code(pf.err);
      pfs.push_back(std::move(*pf.value));
    }
    auto accs = plonk_ipa_verify_batch(dk.svk, prs, insts, pfs, threads);
    if (!accs.ok()) return error_code(accs.err);
    const size_t stride = 32 * dk.svk.k + 64;
    if (accs_out)
      for (size_t i = 0; i < accs.value->size(); ++i) put_ipa_acc((*accs.value)[i], accs_out + i * stride);
    if (!decide) return 1;
    return IpaAs<Bgh19>::decide_all(dk, *accs.value).ok() ? 1 : 0;
  });
}

// ---- prover (ipa.rs:39-124, accumulation.rs:148-226) on the device session --------------------------------------
// `rand32` holds the n_rand scalars `rng()` plays, in the order the prover draws them (running out is a panic).
// proof_out (cap bytes) receives the transcript's stream, *plen its length; acc_out the new accumulator (pack_acc).
namespace {
std::function<Fr()> ipa_rng_of(const uint8_t* rand32, size_t n_rand, size_t* used) {
  return [=]() {
    if (*used >= n_rand) throw Panic("ipa create_proof: rng ran out of scalars");
    Fr v;
    if (!Fr::from_bytes(rand32 + 32 * (*used)++, &v)) throw Panic("ipa create_proof: non-canonical rng scalar");
    return v;
  };
}
IpaDecidingKey ipa_dk_of(const uint8_t* svk_bytes, const uint8_t* g, size_t n_g) {
  IpaDecidingKey dk;
  dk.svk = parse_ipa_svk(svk_bytes);
  dk.g.resize(n_g);
  for (size_t i = 0; i < n_g; ++i) dk.g[i] = G1Affine::from_bytes(g + 64 * i);
  return dk;
}
int ipa_put_proof(const Transcript& t, const IpaAccumulator& acc, uint8_t* proof_out, size_t cap, size_t* plen,
                  uint8_t* acc_out) {
  std::vector<uint8_t> st = transcript_stream(t);
  *plen = st.size();
  if (st.size() > cap) return -2;
  memcpy(proof_out, st.data(), st.size());
  put_ipa_acc(acc, acc_out);
  return 1;
}
}  // namespace

extern "C" int SNARKV_DRV(ipa_create_proof)(int tkind, const uint8_t* svk_bytes, const uint8_t* g, size_t n_g,
                                            const uint8_t* p32, const uint8_t* z32, const uint8_t* omega32_or_null,
                                            const uint8_t* rand32, size_t n_rand, uint8_t* proof_out, size_t cap,
                                            size_t* plen, uint8_t* acc_out) {
  return guarded([&] {
    IpaDecidingKey dk = ipa_dk_of(svk_bytes, g, n_g);
    std::vector<Fr> p(n_g);
    for (size_t i = 0; i < n_g; ++i)
      if (!Fr::from_bytes(p32 + 32 * i, &p[i])) return -3;
    Fr z;
    if (!Fr::from_bytes(z32, &z)) return -3;
    std::optional<Fr> omega;
    if (omega32_or_null) {
      omega = Fr::zero();
      if (!Fr::from_bytes(omega32_or_null, &*omega)) return -3;
    }
    size_t used = 0;
    auto t = make_transcript(tkind, nullptr, 0);
    auto acc = Ipa::create_proof(dk, std::move(p), z, omega, *t, ipa_rng_of(rand32, n_rand, &used));
    if (!acc.ok()) return error_code(acc.err);
    return ipa_put_proof(*t, *acc.value, proof_out, cap, plen, acc_out);
  });
}

extern "C" int SNARKV_DRV(ipa_as_create_proof)(int tkind, const uint8_t* svk_bytes, const uint8_t* g, size_t n_g,
                                               const uint8_t* accs, uint32_t m, const uint8_t* rand32, size_t n_rand,
                                               uint8_t* proof_out, size_t cap, size_t* plen, uint8_t* acc_out) {
  return guarded([&] {
    IpaDecidingKey dk = ipa_dk_of(svk_bytes, g, n_g);
    std::vector<IpaAccumulator> instances;
    if (!parse_ipa_accs(accs, dk.svk.k, m, &instances)) return -3;
    size_t used = 0;
    auto t = make_transcript(tkind, nullptr, 0);
    auto acc = IpaAs<>::create_proof(dk, instances, *t, ipa_rng_of(rand32, n_rand, &used));
    if (!acc.ok()) return error_code(acc.err);
    return ipa_put_proof(*t, *acc.value, proof_out, cap, plen, acc_out);
  });
}
