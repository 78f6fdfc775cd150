// A prover session's resident memory, its stream-ordered copies and the check that the top of the quotient is zero: the bodies
// behind include/snarkv_plonk_prove.h (plonk_prove.hip, libsnarkv_amd.so) and include/snarkv_pallas_session.h (session.hip,
// libsnarkv_pallas.so).  Nothing here depends on the curve: bytes are moved and compared with zero.  `who` is the name the
// messages carry.
#pragma once
#include <algorithm>
#include "ctx.hpp"
#include "poly_args.hpp"

namespace snarkv {

// Any word of `vecs` 16-byte vectors not zero sets bit 0 of *status.  A pass over memory: 16 bytes a lane and step, the grid
// strides; a wave that saw only zeros issues no atomic, so a quotient that divides costs none at all.  The status word is read
// by the host at its next synchronisation, as k_kzg_check_rem's is.
__global__ void __launch_bounds__(256) k_plonk_tail_nonzero(const uint4* __restrict__ tail, size_t vecs, uint32_t* __restrict__ status) {
  uint32_t any = 0;
  for (size_t i = (size_t)blockIdx.x * 256u + threadIdx.x; i < vecs; i += (size_t)gridDim.x * 256u) {
    const uint4 v = tail[i];
    any |= v.x | v.y | v.z | v.w;
  }
  if (__ballot(any != 0) != 0 && (threadIdx.x & 63u) == 0) atomicOr(status, 1u);
}

inline int resident_alloc(snarkv_ctx* ctx, size_t bytes, void** d_out, const char* who) {
  if (!ctx || !d_out) return SNARKV_ERR_ARG;
  *d_out = nullptr;
  if (bytes == 0) return SNARKV_ERR_EMPTY;
  SNARKV_HIP(hipSetDevice(ctx->device));
  void* d = nullptr;
  SNARKV_HIP(hipMalloc(&d, bytes));
  const hipError_t e = hipMemsetAsync(d, 0, bytes, ctx->stream);
  if (e != hipSuccess) {
    (void)hipFree(d);
    set_last_error("%s: hipMemsetAsync -> %s", who, hipGetErrorString(e));
    return SNARKV_ERR_DEVICE;
  }
  *d_out = d;
  return SNARKV_OK;
}

inline void resident_free(snarkv_ctx* ctx, void* d_mem) {
  if (!ctx || !d_mem) return;
  if (hipSetDevice(ctx->device) != hipSuccess) return;
  (void)hipStreamSynchronize(ctx->stream);
  (void)hipFree(d_mem);
}

inline int resident_upload(snarkv_ctx* ctx, void* d_dst, const void* src, size_t bytes) {
  if (!ctx || !d_dst || !src) return SNARKV_ERR_ARG;
  if (bytes == 0) return SNARKV_OK;
  SNARKV_HIP(hipSetDevice(ctx->device));
  SNARKV_HIP(hipMemcpyAsync(d_dst, src, bytes, hipMemcpyHostToDevice, ctx->stream));  // pageable: staged before it returns
  return SNARKV_OK;
}

inline int resident_copy(snarkv_ctx* ctx, void* d_dst, const void* d_src, size_t bytes, const char* who) {
  if (!ctx || !d_dst || !d_src) return SNARKV_ERR_ARG;
  if (overlap(d_dst, bytes, d_src, bytes)) return refuse_overlap(who, "the source and the destination");
  if (bytes == 0) return SNARKV_OK;
  SNARKV_HIP(hipSetDevice(ctx->device));
  SNARKV_HIP(hipMemcpyAsync(d_dst, d_src, bytes, hipMemcpyDeviceToDevice, ctx->stream));
  return SNARKV_OK;
}

inline int resident_download(snarkv_ctx* ctx, void* dst, const void* d_src, size_t bytes) {
  if (!ctx || !dst || !d_src) return SNARKV_ERR_ARG;
  SNARKV_HIP(hipSetDevice(ctx->device));
  if (bytes) SNARKV_HIP(hipMemcpyAsync(dst, d_src, bytes, hipMemcpyDeviceToHost, ctx->stream));
  SNARKV_HIP(hipStreamSynchronize(ctx->stream));
  return SNARKV_OK;
}

inline int resident_tail_check(snarkv_ctx* ctx, const void* d_tail32, size_t count, void* d_status, const char* who) {
  if (!ctx || !aligned16(d_tail32) || !d_status || (uintptr_t)d_status % 4 != 0) return SNARKV_ERR_ARG;
  if (count > ((size_t)1 << 36)) return SNARKV_ERR_LENGTH;
  if (overlap(d_tail32, bytes_of(count), d_status, 4)) return refuse_overlap(who, "the status word and the tail");
  if (count == 0) return SNARKV_OK;
  SNARKV_HIP(hipSetDevice(ctx->device));
  const size_t vecs = 2 * count;  // the grid: one step per lane up to 2048 workgroups, strides beyond
  const uint32_t blocks = (uint32_t)std::min<size_t>((vecs + 255) / 256, 2048);
  hipLaunchKernelGGL(k_plonk_tail_nonzero, dim3(blocks), dim3(256), 0, ctx->stream, (const uint4*)d_tail32, vecs, (uint32_t*)d_status);
  SNARKV_HIP(hipGetLastError());
  return SNARKV_OK;
}

}  // namespace snarkv
