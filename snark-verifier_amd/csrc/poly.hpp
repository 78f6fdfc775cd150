// Internal: the enqueue steps of poly.hip (include/snarkv_poly.h) as ipa_multiopen.hip sees them.  Arguments are taken as
// checked; every step enqueues on ctx->stream and none synchronises (ctx_reserve may, when the scratch slot grows).
#pragma once
#include "ctx.hpp"

namespace snarkv {

constexpr uint32_t kPolyBlock = 256;      // coefficients per workgroup of the scan (poly_scan.h's B)
constexpr uint32_t kPolyLincombTerms = 32;  // terms per pass of the linear combination
constexpr size_t kPolyMaxLen = (size_t)1 << 30;

int poly_enqueue_lincomb(snarkv_ctx* ctx, const void* d_polys, size_t n, const uint32_t* idx, const uint8_t* scalars32,
                         size_t count, void* d_out);
int poly_enqueue_eval(snarkv_ctx* ctx, const void* d_coeffs, size_t n, const void* d_point, void* d_out);
int poly_enqueue_div_linear(snarkv_ctx* ctx, const void* d_coeffs, size_t n, const void* d_root, void* d_quot, void* d_rem);
// poly_batch.hip (include/snarkv_poly_batch.h): out[i] = polys[q_poly[i]](points[q_point[i]]), the index arrays on the host
int poly_enqueue_eval_many(snarkv_ctx* ctx, const void* d_polys, size_t n, const void* d_points, const uint32_t* q_poly,
                           const uint32_t* q_point, size_t count, void* d_out);

}  // namespace snarkv
