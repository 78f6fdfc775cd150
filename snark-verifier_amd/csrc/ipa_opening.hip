// The blinded opening with halo2's Blake2b transcript (blake2b_dev.h) on the device (ipa_opening.hpp): the prover session's
// rounds and folds (ipa_prover.hip, through the enqueue steps of ipa_prover.hpp) with the transcript kernels between them on
// the same stream.  Same source for both curves.  Per opening, everything enqueued before the one synchronisation at the end:
//   [p_bar] k_ipa_eval_partials + k_ipa_eval_sub   p_bar[0] -= p_bar(z), with the powers of z the session holds
//           commit                                 c_bar (Bgh19: s) = <p_bar, G> + omega_bar s
//           k_ipa_transcript_zk                    writes c_bar, squeezes alpha, writes omega' = omega + alpha omega_bar
//             Bgh19: k_mo_transcript_s             writes s, squeezes alpha, then xi_0
//           k_ipa_axpy                             p' = p + alpha p_bar
//   open    k_ipa_transcript_open                  squeezes xi_0 into the slot the session's h' = xi_0 h reads (Ipa only)
//   k x     round (session)                        L | R at SM_LR
//           k_ipa_transcript_round                 absorbs L and R, writes them compressed, squeezes xi_i, xi_i^-1
//           fold (session)
//   finish  k_ipa_transcript_finish                writes U and c
//             Bgh19: k_mo_transcript_finish        writes c, omega', U
// The transcript kernels run on one wavefront with lane 0 working: a few BLAKE2b compressions and, in the round, the 254
// squarings of xi^-1 (what k_ipa_xi_inv does for the session).  What a kernel absorbs is collected in one LDS message, so that it
// carries one copy of the compression for absorbing and one for the digest.
#include <string.h>
#include <algorithm>
#include "ipa_opening.hpp"

namespace snarkv {

__device__ __forceinline__ void st_words(uint32_t* __restrict__ p, const uint32_t (&w)[8]) {
  uint4* o = reinterpret_cast<uint4*>(p);
  o[0] = make_uint4(w[0], w[1], w[2], w[3]);
  o[1] = make_uint4(w[4], w[5], w[6], w[7]);
}

// absorbs L | R (at `lr`), writes both compressed to proof64, squeezes xi: canonical to xi_pair[0..8) and xi_out, xi^-1 to
// xi_pair[8..16).  An identity sets kStatusRoundInf and the round goes on: the kernels after it take any scalar.
__global__ void __launch_bounds__(64) k_ipa_transcript_round(const uint8_t* __restrict__ lr, uint32_t* __restrict__ xi_pair,
                                                             Blake2bState* __restrict__ st, uint8_t* __restrict__ proof64,
                                                             uint32_t* __restrict__ xi_out, uint32_t* __restrict__ status) {
  __shared__ uint8_t msg[2 * kTrPointBytes + kTrSqueezeBytes];
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  bool ok = tr_put_point(msg, lr, lr + 32);
  ok = tr_put_point(msg + kTrPointBytes, lr + 64, lr + 96) && ok;
  tr_put_squeeze(msg + 2 * kTrPointBytes);
  if (!ok) *status |= kStatusRoundInf;
  tr_compress_point(lr, lr + 32, proof64);
  tr_compress_point(lr + 64, lr + 96, proof64 + 32);
  b2b_update(*st, msg, sizeof(msg));
  uint32_t w[8];
  const Fr29 xi = tr_challenge(*st, w);
  st_words(xi_pair, w);
  st_words(xi_out, w);
  st_fr(xi_pair + 8, fr_inv(xi));
}

// ---- TranscriptOrder::Ipa ------------------------------------------------------------------------------------------------
// squeezes xi_0 (ipa.rs:71) where the session's h' = xi_0 h reads it
__global__ void __launch_bounds__(64) k_ipa_transcript_open(Blake2bState* __restrict__ st, uint32_t* __restrict__ xi0_out) {
  __shared__ uint8_t msg[kTrSqueezeBytes];
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  tr_put_squeeze(msg);
  b2b_update(*st, msg, sizeof(msg));
  uint32_t w[8];
  (void)tr_challenge(*st, w);
  st_words(xi0_out, w);
}

// ipa.rs:62-66: writes c_bar, squeezes alpha (canonical to alpha_out), writes omega' = omega + alpha omega_bar
__global__ void __launch_bounds__(64) k_ipa_transcript_zk(const uint8_t* __restrict__ cbar, const uint32_t* __restrict__ omegas,
                                                          Blake2bState* __restrict__ st, uint8_t* __restrict__ proof64,
                                                          uint32_t* __restrict__ alpha_out, uint32_t* __restrict__ status) {
  __shared__ uint8_t msg[kTrPointBytes + kTrSqueezeBytes + kTrScalarBytes];
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  if (!tr_put_point(msg, cbar, cbar + 32)) *status |= kStatusBlindInf;
  tr_put_squeeze(msg + kTrPointBytes);
  tr_compress_point(cbar, cbar + 32, proof64);
  uint32_t w[8];
  // two passes through the one absorbing site: c_bar and the challenge's prefix, then omega'
  const uint8_t* part = msg;
  size_t part_len = kTrPointBytes + kTrSqueezeBytes;
#pragma unroll 1
  for (int pass = 0; pass < 2; ++pass) {
    b2b_update(*st, part, part_len);
    if (pass == 0) {
      const Fr29 alpha = tr_challenge(*st, w);
      st_words(alpha_out, w);
      const Fr29 op = fr29_add(ld_fr(omegas), fr29_mul(alpha, ld_fr(omegas + 8)));
      fr29_to_canonical(op, w);
      uint8_t* sc = msg + kTrPointBytes + kTrSqueezeBytes;
      sc[0] = 0x02;
      for (int i = 0; i < 32; ++i) {
        const uint8_t b = (uint8_t)(w[i >> 2] >> (8 * (i & 3)));
        sc[1 + i] = b;
        proof64[32 + i] = b;
      }
      part = sc;
      part_len = kTrScalarBytes;
    }
  }
}

// ipa.rs:119-120: writes U = the last base and c = the last coefficient; U also to u_out
__global__ void __launch_bounds__(64) k_ipa_transcript_finish(const uint8_t* __restrict__ u, const uint8_t* __restrict__ c,
                                                              Blake2bState* __restrict__ st, uint8_t* __restrict__ proof64,
                                                              uint8_t* __restrict__ u_out, uint32_t* __restrict__ status) {
  __shared__ uint8_t msg[kTrPointBytes + kTrScalarBytes];
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  if (!tr_put_point(msg, u, u + 32)) *status |= kStatusUInf;
  tr_put_scalar(msg + kTrPointBytes, c);
  tr_compress_point(u, u + 32, proof64);
  for (int i = 0; i < 32; ++i) proof64[32 + i] = c[i];
  for (int i = 0; i < 64; ++i) u_out[i] = u[i];
  b2b_update(*st, msg, sizeof(msg));
}

// ---- TranscriptOrder::Bgh19 ----------------------------------------------------------------------------------------------
// before the rounds: writes s, squeezes alpha (canonical to alpha_out), squeezes xi_0 into the slot the session's
// h' = xi_0 h reads.  Two passes through the one absorbing site.
__global__ void __launch_bounds__(64) k_mo_transcript_s(const uint8_t* __restrict__ s64, Blake2bState* __restrict__ st,
                                                        uint8_t* __restrict__ proof32, uint32_t* __restrict__ alpha_out,
                                                        uint32_t* __restrict__ xi0_out, uint32_t* __restrict__ status) {
  __shared__ uint8_t msg[kTrPointBytes + 2 * kTrSqueezeBytes];
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  if (!tr_put_point(msg, s64, s64 + 32)) *status |= kStatusBlindInf;
  tr_put_squeeze(msg + kTrPointBytes);
  tr_put_squeeze(msg + kTrPointBytes + kTrSqueezeBytes);
  tr_compress_point(s64, s64 + 32, proof32);
  const uint8_t* part = msg;
  size_t part_len = kTrPointBytes + kTrSqueezeBytes;
  uint32_t* out = alpha_out;
#pragma unroll 1
  for (int pass = 0; pass < 2; ++pass) {
    b2b_update(*st, part, part_len);
    uint32_t w[8];
    (void)tr_challenge(*st, w);
    st_words(out, w);
    part = msg + kTrPointBytes + kTrSqueezeBytes;
    part_len = kTrSqueezeBytes;
    out = xi0_out;
  }
}

// ... and after them: writes c = the last coefficient, omega' = omega + alpha omega_bar, U = the last base; U also to u_out
__global__ void __launch_bounds__(64) k_mo_transcript_finish(const uint8_t* __restrict__ u, const uint8_t* __restrict__ c,
                                                             const uint32_t* __restrict__ omegas,
                                                             const uint32_t* __restrict__ alpha, Blake2bState* __restrict__ st,
                                                             uint8_t* __restrict__ proof128, uint8_t* __restrict__ u_out,
                                                             uint32_t* __restrict__ status) {
  __shared__ uint8_t msg[2 * kTrScalarBytes + kTrPointBytes];
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  tr_put_scalar(msg, c);
  const Fr29 op = fr29_add(ld_fr(omegas), fr29_mul(ld_fr(alpha), ld_fr(omegas + 8)));
  uint32_t w[8];
  fr29_to_canonical(op, w);
  uint8_t* sc = msg + kTrScalarBytes;
  sc[0] = 0x02;
  for (int i = 0; i < 32; ++i) {
    const uint8_t b = (uint8_t)(w[i >> 2] >> (8 * (i & 3)));
    sc[1 + i] = b;
    proof128[32 + i] = b;
  }
  if (!tr_put_point(msg + 2 * kTrScalarBytes, u, u + 32)) *status |= kStatusUInf;
  for (int i = 0; i < 32; ++i) proof128[i] = c[i];
  tr_compress_point(u, u + 32, proof128 + 64);
  for (int i = 0; i < 64; ++i) u_out[i] = u[i];
  b2b_update(*st, msg, sizeof(msg));
}

// ---- the blinding, either order ----------------------------------------------------------------------------------------
// per-workgroup partial sums of <p_bar, zs> = p_bar(z)
__global__ void __launch_bounds__(kIpThreads) k_ipa_eval_partials(const uint32_t* __restrict__ pbar, const uint32_t* __restrict__ zs,
                                                                  uint32_t n, Fr29* __restrict__ partials) {
  __shared__ Fr29 sh[kIpThreads];
  Fr29 acc = fr29_zero();
  for (uint32_t j = blockIdx.x * kIpThreads + threadIdx.x; j < n; j += gridDim.x * kIpThreads)
    acc = fr_add_red(acc, fr29_mul(ld_fr(pbar + 8 * (size_t)j), ld_fr(zs + 8 * (size_t)j)));
  sh[threadIdx.x] = acc;
  __syncthreads();
  for (uint32_t s = kIpThreads / 2; s > 0; s >>= 1) {
    if (threadIdx.x < s) sh[threadIdx.x] = fr_add_red(sh[threadIdx.x], sh[threadIdx.x + s]);
    __syncthreads();
  }
  if (threadIdx.x == 0) partials[blockIdx.x] = sh[0];
}

// p_bar[0] -= the sum of the partials (ipa.rs:56-57)
__global__ void __launch_bounds__(kIpThreads) k_ipa_eval_sub(const Fr29* __restrict__ partials, uint32_t blocks,
                                                             uint32_t* __restrict__ pbar) {
  __shared__ Fr29 sh[kIpThreads];
  Fr29 acc = fr29_zero();
  for (uint32_t b = threadIdx.x; b < blocks; b += kIpThreads) acc = fr_add_red(acc, partials[b]);
  sh[threadIdx.x] = acc;
  __syncthreads();
  for (uint32_t s = kIpThreads / 2; s > 0; s >>= 1) {
    if (threadIdx.x < s) sh[threadIdx.x] = fr_add_red(sh[threadIdx.x], sh[threadIdx.x + s]);
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    Fr29 d = ld_fr(pbar);  // (-r/2, 3r/2) minus (-r/8, 9r/8): within fr29_to_canonical's 8 r
#pragma unroll
    for (int i = 0; i < 9; ++i) d.v[i] -= sh[0].v[i];
    st_fr(pbar, d);
  }
}

// coeffs[j] += alpha pbar[j]   (ipa.rs:68)
__global__ void __launch_bounds__(256) k_ipa_axpy(uint32_t* __restrict__ coeffs, const uint32_t* __restrict__ pbar,
                                                  const uint32_t* __restrict__ alpha_canon, uint32_t n) {
  const uint32_t j = blockIdx.x * 256u + threadIdx.x;
  if (j >= n) return;
  const Fr29 alpha = ld_fr(alpha_canon);
  const size_t o = 8 * (size_t)j;
  st_fr(coeffs + o, fr29_add(ld_fr(coeffs + o), fr29_mul(alpha, ld_fr(pbar + o))));
}

namespace {

// p_bar[0] -= p_bar(z), the blinding point = commit(p_bar, omega_bar), the transcript up to alpha, p' = p + alpha p_bar
int enqueue_blinding(snarkv_ipa_prover* p, uint8_t* blk, void* d_pbar, TranscriptOrder order) {
  snarkv_ctx* ctx = p->ctx;
  hipStream_t s = ctx->stream;
  const size_t n = (size_t)1 << p->k;
  Blake2bState* st = (Blake2bState*)(blk + OP_STATE);
  uint32_t *status = (uint32_t*)(blk + OP_STATUS), *alpha = (uint32_t*)(blk + OP_ALPHA);
  const uint32_t blocks = (uint32_t)std::min<size_t>(kIpMaxBlocks, (n + kIpThreads - 1) / kIpThreads);
  hipLaunchKernelGGL(k_ipa_eval_partials, dim3(blocks), dim3(kIpThreads), 0, s, (const uint32_t*)d_pbar,
                     (const uint32_t*)p->d_zs, (uint32_t)n, (Fr29*)(blk + OP_PARTIALS));
  hipLaunchKernelGGL(k_ipa_eval_sub, dim3(1), dim3(kIpThreads), 0, s, (const Fr29*)(blk + OP_PARTIALS), blocks,
                     (uint32_t*)d_pbar);
  SNARKV_HIP(hipGetLastError());
  {
    SNARKV_WIRE_FORM(ctx);
    SNARKV_TRY(ipa_enqueue_commit(ctx, p->d_key, d_pbar, n, p->d_small + SM_OFFN + 8 * p->k, blk + OP_PTS2, blk + OP_SC2,
                                  blk + OP_OFF02, blk + OP_BLIND, true));
  }
  if (order == TranscriptOrder::Ipa)
    hipLaunchKernelGGL(k_ipa_transcript_zk, dim3(1), dim3(64), 0, s, (const uint8_t*)(blk + OP_BLIND),
                       (const uint32_t*)(blk + OP_OMEGA), st, blk + OP_PROOF, alpha, status);
  else
    hipLaunchKernelGGL(k_mo_transcript_s, dim3(1), dim3(64), 0, s, (const uint8_t*)(blk + OP_BLIND), st, blk + OP_PROOF, alpha,
                       (uint32_t*)(p->d_small + SM_COMB_S + 32), status);
  hipLaunchKernelGGL(k_ipa_axpy, dim3((uint32_t)((n + 255) / 256)), dim3(256), 0, s, (uint32_t*)p->d_coeffs,
                     (const uint32_t*)d_pbar, (const uint32_t*)alpha, (uint32_t)n);
  SNARKV_HIP(hipGetLastError());
  return SNARKV_OK;
}

// everything of one opening on the session's stream; `host` receives [OP_STATUS, OP_PROOF + len) after the one synchronisation
int enqueue_and_wait(snarkv_ipa_prover* p, uint8_t* blk, void* d_pbar, TranscriptOrder order, size_t len,
                     std::vector<uint8_t>& host) {
  const bool ipa = order == TranscriptOrder::Ipa;
  if (!ipa && !d_pbar) return SNARKV_ERR_ARG;  // Bgh19 is zero-knowledge
  hipStream_t s = p->ctx->stream;
  const uint32_t k = p->k;
  uint8_t* sm = p->d_small;
  Blake2bState* st = (Blake2bState*)(blk + OP_STATE);
  uint32_t* status = (uint32_t*)(blk + OP_STATUS);
  uint8_t* proof = blk + OP_PROOF + (ipa ? (d_pbar ? 64 : 0) : 32);  // behind c_bar | omega', or behind s
  SNARKV_TRY(session_fold_staging(p));  // every allocation before the first kernel
  SNARKV_TRY(session_enqueue_powers(p));
  if (d_pbar) SNARKV_TRY(enqueue_blinding(p, blk, d_pbar, order));
  if (ipa) {
    hipLaunchKernelGGL(k_ipa_transcript_open, dim3(1), dim3(64), 0, s, st, (uint32_t*)(sm + SM_COMB_S + 32));
    SNARKV_HIP(hipGetLastError());
  }
  SNARKV_TRY(session_enqueue_hprime(p));
  for (uint32_t i = 0; i < k; ++i) {
    SNARKV_TRY(session_enqueue_round(p));
    hipLaunchKernelGGL(k_ipa_transcript_round, dim3(1), dim3(64), 0, s, (const uint8_t*)(sm + SM_LR), (uint32_t*)(sm + SM_XI),
                       st, proof + 64 * i, (uint32_t*)(blk + OP_XI + 32 * i), status);
    SNARKV_HIP(hipGetLastError());
    SNARKV_TRY(session_enqueue_fold(p));
    p->rounds += 1;
  }
  if (ipa)
    hipLaunchKernelGGL(k_ipa_transcript_finish, dim3(1), dim3(64), 0, s, (const uint8_t*)p->d_bases,
                       (const uint8_t*)p->d_coeffs, st, proof + 64 * k, blk + OP_U, status);
  else
    hipLaunchKernelGGL(k_mo_transcript_finish, dim3(1), dim3(64), 0, s, (const uint8_t*)p->d_bases, (const uint8_t*)p->d_coeffs,
                       (const uint32_t*)(blk + OP_OMEGA), (const uint32_t*)(blk + OP_ALPHA), st, proof + 64 * k, blk + OP_U,
                       status);
  SNARKV_HIP(hipGetLastError());
  host.resize(OP_PROOF - OP_STATUS + len);
  SNARKV_HIP(hipMemcpyAsync(host.data(), blk + OP_STATUS, host.size(), hipMemcpyDeviceToHost, s));
  SNARKV_HIP(hipStreamSynchronize(s));  // the only one of the opening
  return SNARKV_OK;
}

}  // namespace

int opening_infinity_error(const char* who, const char* what) {
  set_last_error("%s: cannot write points at infinity to the transcript (%s)", who, what);
  return SNARKV_ERR_ENCODING;
}

int opening_upload_pbar(snarkv_ctx* ctx, const char* who, void* d_pbar, const void* pbar, bool on_device, size_t n, int* d_bad) {
  if (hipMemcpyAsync(d_pbar, pbar, n * 32, on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, ctx->stream) !=
      hipSuccess) {
    set_last_error("%s: upload failed", who);
    return SNARKV_ERR_DEVICE;
  }
  if (!(ctx->flags & SNARKV_FLAG_VALIDATE)) return SNARKV_OK;
  int bad = 0;
  SNARKV_TRY(count_bad(ctx, d_pbar, n, d_bad, &bad));
  if (bad) {
    set_last_error("%s: %d of %zu scalars of p_bar are not canonical", who, bad, n);
    return SNARKV_ERR_ENCODING;
  }
  return SNARKV_OK;
}

int opening_prove(snarkv_ipa_prover* p, uint8_t* blk, void* d_pbar, TranscriptOrder order, const char* who,
                  const char* blind_name, uint8_t* tail_out, uint8_t* xi_out32, uint8_t* u_out64) {
  const size_t k = p->k;
  const size_t len = 64 * k + (order == TranscriptOrder::Bgh19 ? 128 : (d_pbar ? 128 : 64));
  std::vector<uint8_t> host;
  const int rc = enqueue_and_wait(p, blk, d_pbar, order, len, host);
  if (rc == SNARKV_OK) session_free(p);
  else session_close(p);  // a failure may have left work in flight
  if (rc != SNARKV_OK) return rc;
  uint32_t status;
  memcpy(&status, host.data(), 4);
  if (status)
    return opening_infinity_error(who, status & kStatusBlindInf ? blind_name : (status & kStatusRoundInf ? "L or R of a round" : "U"));
  memcpy(u_out64, &host[OP_U - OP_STATUS], 64);
  memcpy(xi_out32, &host[OP_XI - OP_STATUS], 32 * k);
  memcpy(tail_out, &host[OP_PROOF - OP_STATUS], len);
  return SNARKV_OK;
}

}  // namespace snarkv
