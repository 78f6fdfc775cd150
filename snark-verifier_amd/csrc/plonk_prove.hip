// The device side of the PLONK prover session (include/snarkv_plonk_prove.h): resident memory, stream-ordered copies, and
// the one new kernel of the flow -- is the top of the quotient zero?  Everything else the session runs is the existing
// stages' (ntt.hip, quotient.hip, poly_batch.hip, poly.hip, kzg_multiopen.hip, the Pippenger batch).  The bodies are
// session_mem.hpp's, which the pasta build has under names of its own (session.hip).
#include "session_mem.hpp"
#include "../../include/snarkv_plonk_prove.h"

using namespace snarkv;

extern "C" {

int snarkv_plonk_session_alloc(snarkv_ctx* ctx, size_t bytes, void** d_out) { return resident_alloc(ctx, bytes, d_out, "plonk_session_alloc"); }

void snarkv_plonk_session_free(snarkv_ctx* ctx, void* d_mem) { resident_free(ctx, d_mem); }

int snarkv_plonk_session_upload(snarkv_ctx* ctx, void* d_dst, const void* src, size_t bytes) { return resident_upload(ctx, d_dst, src, bytes); }

int snarkv_plonk_session_copy(snarkv_ctx* ctx, void* d_dst, const void* d_src, size_t bytes) {
  return resident_copy(ctx, d_dst, d_src, bytes, "plonk_session_copy");
}

int snarkv_plonk_session_download(snarkv_ctx* ctx, void* dst, const void* d_src, size_t bytes) { return resident_download(ctx, dst, d_src, bytes); }

int snarkv_plonk_tail_check_dev(snarkv_ctx* ctx, const void* d_tail32, size_t count, void* d_status) {
  return resident_tail_check(ctx, d_tail32, count, d_status, "plonk_tail_check");
}

}  // extern "C"
