// Internal: the blinded opening of a session's polynomial with halo2's Blake2b transcript on the device, once for its two
// callers: `Ipa::create_proof` in one call (ipa_create.hip) and the Bgh19 multi-open prover (ipa_multiopen.hip).  A caller
// checks its arguments, stages the call's device block, opens the session (ipa_prover.hpp) and hands both to opening_prove.
#pragma once
#include <string.h>
#include <vector>
#include "blake2b_dev.h"
#include "ipa_prover.hpp"

namespace snarkv {

// layout of a call's device block; the host stages [0, OP_STAGED), [OP_STATUS, OP_PROOF + proof length) comes back in one copy
enum : size_t {
  OP_STATE = 0,       // Blake2bState
  OP_STATUS = 256,    // kStatus* bits | the multi-open's first set whose division left a remainder (0xffffffff: none)
  OP_U = 272,         // U                                   64
  OP_XI = 336,        // xi_1..xi_k                          32 x 32
  OP_PROOF = 1360,    // what the opening writes of the proof 64 x 32 + 128
  OP_ALPHA = 3584,    // alpha                               32
  OP_OMEGA = 3616,    // omega | omega_bar                   64
  OP_SC2 = 3680,      // [1, omega_bar]                      64
  OP_PTS2 = 3744,     // [the MSM of a commitment, s]        128
  OP_OFF02 = 3872,    // {0, 2}
  OP_OFF0N = 3880,    // {0, n}                              the multi-open's, before it has a session
  OP_BLIND = 3904,    // c_bar or s (the multi-open: the commitment of f before it)  64
  OP_SC2F = 3968,     // [1, f_blind]                        64, the multi-open's
  OP_POINT = 4032,    // x_3                                 32, the multi-open's
  OP_DELTA = 4064,    // what p[0] is lowered by             32, the multi-open's
  OP_STAGED = 4096,
  OP_PARTIALS = 4096, // kIpMaxBlocks Fr29
  OP_BYTES = OP_PARTIALS + ((kIpMaxBlocks * sizeof(Fr29) + 31) / 32) * 32,  // the multi-open's variable part follows
};
static_assert(sizeof(Blake2bState) <= OP_STATUS - OP_STATE, "the transcript state has 256 bytes");
static_assert(OP_XI + 32 * 32 <= OP_PROOF && OP_PROOF + 64 * 32 + 128 <= OP_ALPHA, "k <= 32 rounds fit");
static_assert(OP_OFF0N + 8 <= OP_BLIND && OP_DELTA + 32 == OP_STAGED, "the staged slots lie side by side");
constexpr uint32_t kStatusRoundInf = 1, kStatusUInf = 2, kStatusBlindInf = 4;  // a point at infinity met the transcript

// the constants of the blinding commitment in a host image of the block: [1, omega_bar], s and {0, 2}
inline void opening_stage_blinding(uint8_t* stage, const uint8_t* omega_bar32, const uint8_t* s64) {
  const uint32_t off02[2] = {0, 2};
  stage[OP_SC2] = 1;
  memcpy(stage + OP_SC2 + 32, omega_bar32, 32);
  memcpy(stage + OP_PTS2 + 64, s64, 64);
  memcpy(stage + OP_OFF02, off02, sizeof(off02));
}

// what is written around the rounds, and in which order
enum class TranscriptOrder {
  Ipa,    // ipa.rs: c_bar, alpha, omega', xi_0 | rounds | U, c      (without p_bar: xi_0 | rounds | U, c)
  Bgh19,  // s, alpha, xi_0 | rounds | c, omega', U
};

// device buffers of one call; freed when the call leaves, after the stream has drained
struct Buffers {
  hipStream_t stream;
  std::vector<void*> all;
  bool drained = false;  // set once the call's last synchronisation has succeeded
  explicit Buffers(hipStream_t s) : stream(s) {}
  int get(void** out, size_t bytes) {
    SNARKV_TRY(device_malloc(out, bytes));
    all.push_back(*out);
    return SNARKV_OK;
  }
  ~Buffers() {
    if (!all.empty() && !drained) (void)hipStreamSynchronize(stream);  // a failure may have left work in flight
    for (void* b : all) (void)hipFree(b);
  }
};

// sets "<who>: cannot write points at infinity to the transcript (<what>)", returns SNARKV_ERR_ENCODING
int opening_infinity_error(const char* who, const char* what);

// p_bar (n scalars, host or device) to d_pbar on the context's stream; under SNARKV_FLAG_VALIDATE counts those >= r through
// `d_bad` (which synchronises) and refuses any
int opening_upload_pbar(snarkv_ctx* ctx, const char* who, void* d_pbar, const void* pbar, bool on_device, size_t n, int* d_bad);

// Everything of the opening on the session's stream, with one synchronisation at the end: blinds the session's polynomial
// with `d_pbar` (null: `Ipa` without zero knowledge), runs the k rounds and writes the proof in `order`.  `blk` is the staged
// block: the transcript state, and with p_bar OP_OMEGA, OP_SC2, OP_PTS2[1] = s and OP_OFF02.  On success what the opening
// writes of the proof is at `tail_out` (Ipa: 64 k + 64, + 64 with p_bar; Bgh19: 64 k + 128), xi_1..xi_k and U at the other
// two.  Takes the session over: freed here, after the stream has drained when anything failed.  `who` and `blind_name`
// (the first blinding point: "c_bar" / "s") go into the error texts.
int opening_prove(snarkv_ipa_prover* p, uint8_t* blk, void* d_pbar, TranscriptOrder order, const char* who,
                  const char* blind_name, uint8_t* tail_out, uint8_t* xi_out32, uint8_t* u_out64);

}  // namespace snarkv
