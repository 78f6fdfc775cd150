// Test driver of the PASTA flavour of the host mirror -> libsnarkv_hosttest_pallas.so (compiled with
// -DSNARKV_HOST_PALLAS: `Fr` = pallas::Scalar, the loader bound to libsnarkv_pallas.so).  It carries the
// curve-generic part of the mirror -- Msm, the native loader, the IPA layer (host/ipa.hpp), the PLONK
// verifier over `IpaAs<Bgh19>` (host/plonk.hpp) -- with halo2's
// Blake2b transcript: the reference's own `test_ipa` / `test_ipa_as` setting (pcs/ipa.rs:434-466,
// pcs/ipa/accumulation.rs:240-290, system/halo2/test/ipa/native.rs).  KZG (pairing) and the EVM / Poseidon
// transcripts stay BN254.
#ifndef SNARKV_HOST_PALLAS
#error "compile with -DSNARKV_HOST_PALLAS"
#endif
#include <cstdio>
#include <cstring>
#include <functional>
#include <memory>

#include "blake2b_transcript.hpp"
#include "ipa.hpp"
#include "plonk.hpp"
#include "plonk_ipa_batch.hpp"
#include "wire.hpp"

using namespace snarkv_host;

namespace {
#include "driver_parse.inc"

int error_code(const Error& e) {
  switch (e.kind) {
    case Error::Transcript: return -10;
    case Error::InvalidInstances: return -11;
    case Error::InvalidProtocol: return -12;
    case Error::AssertionFailure: return 0;
    default: return -13;
  }
}
int guarded(const std::function<int()>& f) {
  try {
    return f();
  } catch (const Panic& e) {
    fprintf(stderr, "panic: %s\n", e.what());
    return -100;
  } catch (const std::exception& e) {
    fprintf(stderr, "error: %s\n", e.what());
    return -101;
  }
}
std::unique_ptr<Transcript> make_transcript(int /*tkind: Blake2b only*/, const uint8_t* proof, size_t plen) {
  return std::make_unique<Blake2bTranscript>(std::vector<uint8_t>(proof, proof + plen));
}
std::vector<uint8_t> transcript_stream(const Transcript& t) { return dynamic_cast<const Blake2bTranscript&>(t).finalize(); }
}  // namespace

#define SNARKV_DRV(name) hp_##name
#include "ipa_driver.inc"

extern "C" {
// the layout pass of the batch reader (plonk_ipa_batch.hpp): the byte offsets of the compressed points of one proof of
// `protocol` under a key of size k, and the proof's length.  Returns the number of points; fills at most `cap` offsets.
int hp_plonk_ipa_point_offsets(const uint8_t* protocol, size_t plen, uint32_t k, uint32_t* offsets_out, size_t cap,
                               size_t* proof_len) {
  return guarded([&] {
    const IpaProofLayout l = plonk_ipa_proof_layout(parse_protocol(protocol, plen), k);
    for (size_t i = 0; i < l.point_offsets.size() && i < cap; ++i) offsets_out[i] = l.point_offsets[i];
    if (proof_len) *proof_len = l.len;
    return (int)l.point_offsets.size();
  });
}
// the batch reader alone (plonk_ipa_batch.hpp `plonk_ipa_read_batch`) under `route` (0 HOST, 1 DEVICE, 2 AUTO), batch
// bytes as hp_plonk_ipa_verify_batch takes them.  Returns 1 or the first error's code; *hints_taken = the number of
// compressed points of the batch whose decoding a transcript took from the device's answers.
int hp_plonk_ipa_read_batch(const uint8_t* protocol, size_t plen, const uint8_t* instances, size_t ilen,
                            const uint8_t* proofs, size_t prlen, uint32_t n, const uint8_t* svk_bytes, unsigned threads,
                            int route, size_t* hints_taken) {
  return guarded([&] {
    const PlonkProtocol pr = parse_protocol(protocol, plen);
    const IpaSuccinctVerifyingKey svk = parse_ipa_svk(svk_bytes);
    std::vector<std::vector<std::vector<Fr>>> insts;
    std::vector<std::vector<uint8_t>> pbytes;
    wire::split_batch(instances, ilen, proofs, prlen, n, insts, pbytes);
    std::vector<PlonkProof<Bgh19>> pfs;
    Error e = plonk_ipa_read_batch(svk, pr, insts, pbytes, threads, (IpaDecompress)route, pfs, hints_taken);
    return e.ok() ? 1 : error_code(e);
  });
}
// Fr = pallas::Scalar self-test hooks
void hp_fr_mul(const uint8_t* a, const uint8_t* b, uint8_t* out) {
  Fr x, y;
  Fr::from_bytes(a, &x);
  Fr::from_bytes(b, &y);
  (x * y).to_bytes(out);
}
int hp_fr_inv(const uint8_t* a, uint8_t* out) {
  Fr x, y;
  Fr::from_bytes(a, &x);
  if (!x.invert(&y)) return 0;
  y.to_bytes(out);
  return 1;
}
// BLAKE2b-512 with a 16-byte personalisation (RFC 7693), fed in `chunk`-byte pieces
void hp_blake2b(const char* person16, const uint8_t* data, size_t len, size_t chunk, uint8_t out[64]) {
  Blake2b h(64, person16);
  for (size_t o = 0; o < len; o += chunk) h.update(data + o, std::min(chunk, len - o));
  h.digest(out);
}
// a scripted transcript session: ops = sequence of bytes: 'P' read point, 'S' read scalar, 'C' squeeze;
// out = for each op the value (64 / 32 / 32 bytes).  Returns the number of ops done, or -10 at the first
// Transcript error.
int hp_transcript_script(const uint8_t* proof, size_t plen, const char* ops, size_t n_ops, uint8_t* out) {
  return guarded([&] {
    Blake2bTranscript t(std::vector<uint8_t>(proof, proof + plen));
    size_t o = 0;
    for (size_t i = 0; i < n_ops; ++i) {
      if (ops[i] == 'P') {
        auto p = t.read_ec_point();
        if (!p.ok()) return -10;
        memcpy(out + o, p.value->b, 64);
        o += 64;
      } else if (ops[i] == 'S') {
        auto s = t.read_scalar();
        if (!s.ok()) return -10;
        s.value->to_bytes(out + o);
        o += 32;
      } else {
        t.squeeze_challenge().to_bytes(out + o);
        o += 32;
      }
    }
    return (int)n_ops;
  });
}
// The prover's side with the record of the hasher's input (Blake2bTranscript::record_absorbed): ops = 's' common_scalar (32
// bytes of `data`), 'p' write_ec_point (64 bytes), 'w' write_scalar (32 bytes), 'C' squeeze.  Then the next challenge is drawn
// twice: from the transcript (next_a), and from a fresh hasher over the recorded bytes and the 0 byte of a squeeze (next_b) --
// what a device call that is handed `absorbed` does.  `tail` is appended as an opening's bytes.  Out: the recorded bytes and the
// stream.  `record` = 0 leaves the record off: it stays empty.  Returns the ops done, -10 at a Transcript error, -11 when an
// output does not fit `cap`.
int hp_transcript_record(const uint8_t* data, const char* ops, size_t n_ops, int record, const uint8_t* tail, size_t tail_len,
                         uint8_t* rec_out, size_t* rec_len, uint8_t* stream_out, size_t* stream_len, size_t cap, uint8_t* next_a,
                         uint8_t* next_b) {
  return guarded([&] {
    Blake2bTranscript t;
    if (record) t.record_absorbed();
    size_t at = 0;
    for (size_t i = 0; i < n_ops; ++i) {
      Error e;
      Fr x;
      if (ops[i] == 'p') {
        e = t.write_ec_point(G1Affine::from_bytes(data + at));
        at += 64;
      } else if (ops[i] == 'C') {
        (void)t.squeeze_challenge();
      } else {
        if (!Fr::from_bytes(data + at, &x)) return -10;
        e = ops[i] == 's' ? t.common_scalar(x) : t.write_scalar(x);
        at += 32;
      }
      if (!e.ok()) return -10;
    }
    const std::vector<uint8_t> rec = t.absorbed();
    t.squeeze_challenge().to_bytes(next_a);
    Blake2b fresh(64, "Halo2-Transcript");
    fresh.update(rec.data(), rec.size());
    const uint8_t zero = 0;
    fresh.update(&zero, 1);
    uint8_t h[64];
    fresh.digest(h);
    Blake2bTranscript::from_uniform_bytes(h).to_bytes(next_b);
    t.append_opening(tail, tail_len);
    if (rec.size() > cap || t.stream().size() > cap) return -11;
    if (!rec.empty()) memcpy(rec_out, rec.data(), rec.size());
    *rec_len = rec.size();
    if (!t.stream().empty()) memcpy(stream_out, t.stream().data(), t.stream().size());
    *stream_len = t.stream().size();
    return (int)n_ops;
  });
}
}
