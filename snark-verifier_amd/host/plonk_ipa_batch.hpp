// Batch front half of `PlonkVerifier<IpaAs<pallas::Affine, Bgh19>>` with halo2's Blake2b transcript (pasta flavour of
// the mirror only): where the compressed points of a proof sit, their decompression for the whole batch in ONE device
// launch (pallas_g1_decompress, csrc/decompress_pallas.hip), and the N `read_proof`s on the host pool.
//
// A compressed pallas point costs the host a Tonelli-Shanks square root (p - 1 = 2^32 t: blake2b_transcript.hpp
// `pallas_fp::sqrt`), 12 + 2k of them per StandardPlonk proof; nothing else in `read_proof` is heavier than a hash of
// a few hundred bytes.  The KZG flavour finds the offsets by parsing proof 0 (aggregation.hpp `decompress_hints`);
// here they follow from the protocol and k alone, so no proof is read twice.
#pragma once
#if !defined(SNARKV_HOST_PALLAS)
#error "plonk_ipa_batch.hpp belongs to the pasta flavour of the host mirror (-DSNARKV_HOST_PALLAS)"
#endif
#include <atomic>
#include <vector>

#include "../../include/snarkv_host_pallas.h"
#include "../../include/snarkv_pallas_decompress.h"
#include "blake2b_transcript.hpp"
#include "ipa.hpp"
#include "plonk.hpp"

namespace snarkv_host {

// The byte offsets of the compressed points of a `PlonkProof<Bgh19>` in its proof stream, in reading order, and the
// length of the stream: `PlonkProof::read` (proof.rs:52-168) then `Bgh19Proof::read` (bgh19.rs:98-153).  Points and
// scalars are 32 bytes each; challenges and the instances take no bytes.
struct IpaProofLayout {
  std::vector<uint32_t> point_offsets;
  size_t len = 0;
};
inline IpaProofLayout plonk_ipa_proof_layout(const PlonkProtocol& pr, size_t k) {
  IpaProofLayout l;
  size_t at = 0;
  auto points = [&](size_t n) {
    for (size_t i = 0; i < n; ++i, at += 32) l.point_offsets.push_back((uint32_t)at);
  };
  const size_t phases = std::min(pr.num_witness.size(), pr.num_challenge.size());  // `zip`
  for (size_t ph = 0; ph < phases; ++ph) points(pr.num_witness[ph]);
  points(pr.quotient.num_chunk);
  at += 32 * pr.evaluations.size();
  points(1);  // f
  std::vector<Query<Fr>> qs;  // the number of rotation sets: one q_eval each
  for (auto& q : PlonkProof<Bgh19>::empty_queries(pr)) qs.push_back(Query<Fr>{q.poly, q.shift, Fr()});
  at += 32 * bdfg21::query_sets(qs).size();
  points(1);      // S
  points(2 * k);  // L_i, R_i
  at += 64;       // c, blind
  points(1);      // G
  l.len = at;
  return l;
}

// Who takes the square roots of a batch.
enum class IpaDecompress { Host = 0, Device = 1, Auto = 2 };
// (AUTO takes the device route from SNARKV_HOST_PALLAS_DEVICE_MIN proofs on: include/snarkv_host_pallas.h cites the
// measurement)

// `read_proof` of N proofs of one protocol on the host pool.  DEVICE: the points of every proof of the layout's length
// are gathered and decompressed in one launch first, and the transcripts take the answers as hints -- a proof of another
// length, a point the device refused, the identity, or a hint that is not the decoding of the bytes read all go through
// the host's own square root, so verdicts and error texts are the host route's.  Returns the first error in proof order.
// hints_taken (optional): the number of points, over the whole batch, that a transcript decoded from the device's answer.
inline Error plonk_ipa_read_batch(const IpaSuccinctVerifyingKey& svk, const PlonkProtocol& pr,
                                  const std::vector<std::vector<std::vector<Fr>>>& insts,
                                  const std::vector<std::vector<uint8_t>>& proofs, unsigned threads, IpaDecompress route,
                                  std::vector<PlonkProof<Bgh19>>& pfs, size_t* hints_taken = nullptr) {
  const size_t n = proofs.size();
  pfs.resize(n);
  if (route == IpaDecompress::Auto)
    route = n >= (size_t)SNARKV_HOST_PALLAS_DEVICE_MIN ? IpaDecompress::Device : IpaDecompress::Host;
  IpaProofLayout lay;
  std::vector<uint8_t> pts, ok;
  std::vector<size_t> row(n, (size_t)-1);
  size_t P = 0;
  if (route == IpaDecompress::Device && n) {
    lay = plonk_ipa_proof_layout(pr, svk.k);
    P = lay.point_offsets.size();
    std::vector<size_t> who;
    for (size_t i = 0; i < n; ++i)
      if (proofs[i].size() == lay.len) row[i] = who.size(), who.push_back(i);
    if (P && !who.empty()) {
      std::vector<uint8_t> in(32 * P * who.size());
      pts.resize(64 * P * who.size());
      ok.resize(P * who.size());
      parallel_for(who.size(), threads, [&](size_t r) {
        for (size_t q = 0; q < P; ++q) memcpy(&in[32 * (r * P + q)], proofs[who[r]].data() + lay.point_offsets[q], 32);
      }, 64);
      DeviceScope dev;
      if (pallas_g1_decompress(in.data(), P * who.size(), pts.data(), ok.data()) != SNARKV_OK)
        throw std::runtime_error(std::string("pallas_g1_decompress: ") + snarkv_pallas_last_error());
    }
  }
  std::vector<Error> errs(n);
  std::atomic<size_t> taken{0};
  // an instance committing key makes `read_proof` commit to the instances on the device: such a batch is read on the
  // calling thread (pool tasks stay host-only)
  parallel_for(n, pr.instance_committing_key ? 1u : threads, [&](size_t i) {
    Blake2bTranscript t(proofs[i]);
    if (!ok.empty() && row[i] != (size_t)-1)
      t.set_point_hints(lay.point_offsets.data(), &pts[64 * P * row[i]], &ok[P * row[i]], P);
    auto pf = PlonkProof<Bgh19>::read(svk, pr, insts[i], t);
    if (!pf.ok()) errs[i] = pf.err;
    else pfs[i] = std::move(*pf.value);
    taken += t.hints_taken();
  }, 1);
  if (hints_taken) *hints_taken = taken;
  for (auto& e : errs)
    if (!e.ok()) return e;
  return Error{};
}

}  // namespace snarkv_host
