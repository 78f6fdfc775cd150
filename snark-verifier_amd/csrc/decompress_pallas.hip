// Batched point decompression on pallas: the pasta flavour of decompress.hip (pasta build only).
//
// Every commitment of a halo2 proof arrives compressed, and the Blake2b transcript of the IPA flavour
// (host/blake2b_transcript.hpp `read_ec_point`) pays one square root in Fp per point.  With p - 1 = 2^32 t that is a
// Tonelli-Shanks on the host; here the whole batch is one launch of lock-step lanes running the fixed-trip-count
// square root of fq29_sqrt.h:
//
//   k_g1_decompress : one lane per point.  32 bytes in = x little-endian canonical (x < p), bit 255 = parity of y
//                     (pasta_curves' `to_bytes`, as `read_ec_point` takes it); 64 bytes out = x || y canonical, or
//                     halo2curves' in-memory form under SNARKV_FLAG_MONTGOMERY.  ok = 0 for x >= p or x^3 + 5 not a
//                     square.  The all-zero encoding is the identity: 64 zero bytes, ok = 1 (x = 0 is on no point
//                     of the curve: 5 is not a square).
#include "ctx.hpp"
#include "fq.h"
#include "fq29.h"
#include "fq29_sqrt.h"

#if !defined(SNARKV_CURVE_PALLAS)
#error "decompress_pallas.hip belongs to the pasta build (build.py PALLAS_UNITS)"
#endif

namespace snarkv {

__global__ void __launch_bounds__(64) k_g1_decompress(const uint32_t* __restrict__ in, uint32_t* __restrict__ out,
                                                       uint8_t* __restrict__ ok, uint32_t n, uint32_t mont) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const uint4* src = reinterpret_cast<const uint4*>(in + (size_t)i * 8);
  const uint4 a = src[0], b = src[1];
  const uint32_t w[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
  uint32_t o[16];
  const bool good = g1_decompress_words(w, mont != 0u, o);
  uint4* dst = reinterpret_cast<uint4*>(out + (size_t)i * 16);
#pragma unroll
  for (int j = 0; j < 4; ++j) dst[j] = make_uint4(o[4 * j], o[4 * j + 1], o[4 * j + 2], o[4 * j + 3]);
  ok[i] = good ? 1 : 0;
}

int launch_g1_decompress(snarkv_ctx* ctx, const void* d_in32, size_t n, void* d_out64, void* d_ok) {
  hipLaunchKernelGGL(k_g1_decompress, dim3((uint32_t)((n + 63) / 64)), dim3(64), 0, ctx->stream, (const uint32_t*)d_in32,
                     (uint32_t*)d_out64, (uint8_t*)d_ok, (uint32_t)n, ctx->mont ? 1u : 0u);
  SNARKV_HIP(hipGetLastError());
  return SNARKV_OK;
}

}  // namespace snarkv
