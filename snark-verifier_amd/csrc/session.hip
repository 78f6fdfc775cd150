// The device side of a prover session on pallas (include/snarkv_pallas_session.h): the resident memory, the stream-ordered
// copies and the tail check of the BN254 session (plonk_prove.hip) under names of the pasta build.  One body for both:
// session_mem.hpp.
#include "session_mem.hpp"
#include "../../include/snarkv_pallas_session.h"

#if !defined(SNARKV_CURVE_PALLAS)
#error "a unit of the pasta build (PALLAS_UNITS): the BN254 library has these calls in plonk_prove.hip"
#endif

using namespace snarkv;

extern "C" {

int snarkv_pallas_session_alloc(snarkv_ctx* ctx, size_t bytes, void** d_out) { return resident_alloc(ctx, bytes, d_out, "pallas_session_alloc"); }

void snarkv_pallas_session_free(snarkv_ctx* ctx, void* d_mem) { resident_free(ctx, d_mem); }

int snarkv_pallas_session_upload(snarkv_ctx* ctx, void* d_dst, const void* src, size_t bytes) { return resident_upload(ctx, d_dst, src, bytes); }

int snarkv_pallas_session_copy(snarkv_ctx* ctx, void* d_dst, const void* d_src, size_t bytes) {
  return resident_copy(ctx, d_dst, d_src, bytes, "pallas_session_copy");
}

int snarkv_pallas_session_download(snarkv_ctx* ctx, void* dst, const void* d_src, size_t bytes) { return resident_download(ctx, dst, d_src, bytes); }

int snarkv_pallas_poly_tail_check_dev(snarkv_ctx* ctx, const void* d_tail32, size_t count, void* d_status) {
  return resident_tail_check(ctx, d_tail32, count, d_status, "pallas_poly_tail_check");
}

}  // extern "C"
