// `Ipa::create_proof` in one call (include/snarkv_ipa_create.h): the prover session's rounds and folds (ipa_prover.hip, through
// the enqueue steps of ipa_prover.hpp) with halo2's Blake2b transcript (blake2b_dev.h) between them on the same stream.  Same
// source for both curves.  Per proof, everything enqueued before the one synchronisation at the end:
//   [zk]    k_ipa_eval_partials + k_ipa_eval_sub   p_bar[0] -= p_bar(z), with the powers of z the session holds
//           commit                                 c_bar = <p_bar, G> + omega_bar s
//           k_ipa_transcript_zk                    writes c_bar, squeezes alpha, writes omega' = omega + alpha omega_bar
//           k_ipa_axpy                             p' = p + alpha p_bar
//   open    k_ipa_transcript_open                  squeezes xi_0 into the slot the session's h' = xi_0 h reads
//   k x     round (session)                        L | R at SM_LR
//           k_ipa_transcript_round                 absorbs L and R, writes them compressed, squeezes xi_i, xi_i^-1
//           fold (session)
//   finish  k_ipa_transcript_finish                writes U and c
// The transcript kernels run on one wavefront with lane 0 working: a few BLAKE2b compressions and, in the round, the 254
// squarings of xi^-1 (what k_ipa_xi_inv does for the session).  What a kernel absorbs is collected in one LDS message, so that it
// carries one copy of the compression for absorbing and one for the digest.
#include <string.h>
#include <algorithm>
#include <vector>
#include "blake2b_dev.h"
#include "ipa_prover.hpp"
#include "../../include/snarkv_ipa_create.h"

namespace snarkv {

// layout of the call's device buffer; [CR_STATUS, CR_PROOF + proof length) comes back in one copy
enum : size_t {
  CR_STATE = 0,       // Blake2bState
  CR_STATUS = 256,    // kStatus* bits
  CR_U = 272,         // U                           64
  CR_XI = 336,        // xi_1..xi_k                  32 x 32
  CR_PROOF = 1360,    // the proof bytes             64 x 32 + 128
  CR_ALPHA = 3584,    // alpha                       32
  CR_OMEGA = 3616,    // omega | omega_bar           64
  CR_SC2 = 3680,      // [1, omega_bar]              64
  CR_PTS2 = 3744,     // [<p_bar, G>, s]             128
  CR_OFF02 = 3872,    // {0, 2}
  CR_CBAR = 3904,     // c_bar                       64
  CR_STAGED = 4096,   // what the host stages
  CR_PARTIALS = 4096, // kIpMaxBlocks Fr29
  CR_BYTES = CR_PARTIALS + kIpMaxBlocks * sizeof(Fr29),
};
static_assert(sizeof(Blake2bState) <= CR_STATUS - CR_STATE, "the transcript state has 256 bytes");
constexpr uint32_t kStatusRoundInf = 1, kStatusUInf = 2, kStatusCbarInf = 4;  // a point at infinity met the transcript

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
  if (!tr_put_point(msg, cbar, cbar + 32)) *status |= kStatusCbarInf;
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

struct CreateArgs {
  const uint8_t *h64, *s64, *z32, *omega32, *omega_bar32, *absorbed;
  const void *coeffs, *pbar;
  bool on_device;
  size_t n, absorbed_len;
};

// everything of one proof on the context's stream; `host` receives [CR_STATUS, CR_PROOF + need) after the one synchronisation
int create_enqueue_and_wait(snarkv_ctx* ctx, const snarkv_ipa_dk* dk, const CreateArgs& a, bool zk, size_t need,
                            snarkv_ipa_prover* p, uint8_t* cr, void* d_pbar, std::vector<uint8_t>& host) {
  hipStream_t s = ctx->stream;
  const size_t n = a.n;
  const uint32_t k = dk->k;
  uint8_t* sm = p->d_small;
  Blake2bState* st = (Blake2bState*)(cr + CR_STATE);
  uint32_t* status = (uint32_t*)(cr + CR_STATUS);
  uint8_t* proof = cr + CR_PROOF;
  SNARKV_TRY(session_fold_staging(p));  // every allocation before the first kernel
  SNARKV_TRY(session_enqueue_powers(p));
  if (zk) {
    const uint32_t blocks = (uint32_t)std::min<size_t>(kIpMaxBlocks, (n + kIpThreads - 1) / kIpThreads);
    hipLaunchKernelGGL(k_ipa_eval_partials, dim3(blocks), dim3(kIpThreads), 0, s, (const uint32_t*)d_pbar,
                       (const uint32_t*)p->d_zs, (uint32_t)n, (Fr29*)(cr + CR_PARTIALS));
    hipLaunchKernelGGL(k_ipa_eval_sub, dim3(1), dim3(kIpThreads), 0, s, (const Fr29*)(cr + CR_PARTIALS), blocks,
                       (uint32_t*)d_pbar);
    SNARKV_HIP(hipGetLastError());
    {
      SNARKV_WIRE_FORM(ctx);
      SNARKV_TRY(ipa_enqueue_commit(ctx, dk->d_points, d_pbar, n, sm + SM_OFFN + 8 * k, cr + CR_PTS2, cr + CR_SC2,
                                    cr + CR_OFF02, cr + CR_CBAR, true));
    }
    hipLaunchKernelGGL(k_ipa_transcript_zk, dim3(1), dim3(64), 0, s, (const uint8_t*)(cr + CR_CBAR),
                       (const uint32_t*)(cr + CR_OMEGA), st, proof, (uint32_t*)(cr + CR_ALPHA), status);
    hipLaunchKernelGGL(k_ipa_axpy, dim3((uint32_t)((n + 255) / 256)), dim3(256), 0, s, (uint32_t*)p->d_coeffs,
                       (const uint32_t*)d_pbar, (const uint32_t*)(cr + CR_ALPHA), (uint32_t)n);
    SNARKV_HIP(hipGetLastError());
    proof += 64;
  }
  hipLaunchKernelGGL(k_ipa_transcript_open, dim3(1), dim3(64), 0, s, st, (uint32_t*)(sm + SM_COMB_S + 32));
  SNARKV_HIP(hipGetLastError());
  SNARKV_TRY(session_enqueue_hprime(p));
  for (uint32_t i = 0; i < k; ++i) {
    SNARKV_TRY(session_enqueue_round(p));
    hipLaunchKernelGGL(k_ipa_transcript_round, dim3(1), dim3(64), 0, s, (const uint8_t*)(sm + SM_LR), (uint32_t*)(sm + SM_XI),
                       st, proof + 64 * i, (uint32_t*)(cr + CR_XI + 32 * i), status);
    SNARKV_HIP(hipGetLastError());
    SNARKV_TRY(session_enqueue_fold(p));
    p->rounds += 1;
  }
  hipLaunchKernelGGL(k_ipa_transcript_finish, dim3(1), dim3(64), 0, s, (const uint8_t*)p->d_bases, (const uint8_t*)p->d_coeffs,
                     st, proof + 64 * k, cr + CR_U, status);
  SNARKV_HIP(hipGetLastError());
  host.resize(CR_PROOF - CR_STATUS + need);
  SNARKV_HIP(hipMemcpyAsync(host.data(), cr + CR_STATUS, host.size(), hipMemcpyDeviceToHost, s));
  SNARKV_HIP(hipStreamSynchronize(s));  // the only one of the call
  return SNARKV_OK;
}

int create_proof(snarkv_ctx* ctx, const snarkv_ipa_dk* dk, const CreateArgs& a, uint8_t* proof_out, size_t proof_cap,
                 size_t* proof_len, uint8_t* xi_out32, uint8_t* u_out64) {
  if (!ctx || !dk || !a.h64 || !a.coeffs || !a.z32 || !proof_out || !proof_len || !xi_out32 || !u_out64 ||
      (a.absorbed_len && !a.absorbed))
    return SNARKV_ERR_ARG;
  *proof_len = 0;
  const int given = (a.s64 != nullptr) + (a.omega32 != nullptr) + (a.pbar != nullptr) + (a.omega_bar32 != nullptr);
  if (given != 0 && given != 4) {
    set_last_error("ipa_create_proof: s, omega, p_bar and omega_bar come together (zk) or not at all");
    return SNARKV_ERR_ARG;
  }
  const bool zk = given == 4;
  if (dk->device != ctx->device) return SNARKV_ERR_ARG;
  if (dk->first != 0 || dk->count != ((size_t)1 << dk->k) || dk->k < 1 || dk->k > 30) return SNARKV_ERR_LENGTH;
  if (a.n != dk->count) return SNARKV_ERR_LENGTH;
  const uint32_t k = dk->k;
  const size_t need = 64 * (size_t)k + 64 + (zk ? 64 : 0);
  if (proof_cap < need) {
    *proof_len = need;
    set_last_error("ipa_create_proof: the proof has %zu bytes, proof_cap is %zu", need, proof_cap);
    return SNARKV_ERR_LENGTH;
  }
  const bool validate = (ctx->flags & SNARKV_FLAG_VALIDATE) != 0;
  if (validate && (!host_canonical(a.z32) || (zk && (!host_canonical(a.omega32) || !host_canonical(a.omega_bar32))))) {
    set_last_error("ipa_create_proof: z, omega or omega_bar is not canonical");
    return SNARKV_ERR_ENCODING;
  }
  SNARKV_HIP(hipSetDevice(ctx->device));
  // what the host stages: the transcript after the caller's prefix, and the constants of the zk commitment
  std::vector<uint8_t> st(CR_STAGED, 0);
  {
    Blake2bState hs;
    tr_init(hs);
    b2b_update(hs, a.absorbed, a.absorbed_len);
    memcpy(&st[CR_STATE], &hs, sizeof(hs));
  }
  if (zk) {
    memcpy(&st[CR_OMEGA], a.omega32, 32);
    memcpy(&st[CR_OMEGA + 32], a.omega_bar32, 32);
    st[CR_SC2] = 1;
    memcpy(&st[CR_SC2 + 32], a.omega_bar32, 32);
    memcpy(&st[CR_PTS2 + 64], a.s64, 64);
    const uint32_t off02[2] = {0, 2};
    memcpy(&st[CR_OFF02], off02, sizeof(off02));
  }
  snarkv_ipa_prover* p = nullptr;
  SNARKV_TRY(session_open(ctx, dk, a.coeffs, a.on_device, a.n, a.z32, a.h64, nullptr, "ipa_create_proof", &p));
  void *d_cr = nullptr, *d_pbar = nullptr;
  std::vector<uint8_t> host;
  int rc = device_malloc(&d_cr, CR_BYTES);
  if (rc == SNARKV_OK && zk) rc = device_malloc(&d_pbar, a.n * 32);
  if (rc == SNARKV_OK && hipMemcpyAsync(d_cr, st.data(), st.size(), hipMemcpyHostToDevice, ctx->stream) != hipSuccess) {
    set_last_error("ipa_create_proof: upload failed");
    rc = SNARKV_ERR_DEVICE;
  }
  if (rc == SNARKV_OK && zk) {
    if (hipMemcpyAsync(d_pbar, a.pbar, a.n * 32, a.on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice,
                       ctx->stream) != hipSuccess) {
      set_last_error("ipa_create_proof: upload failed");
      rc = SNARKV_ERR_DEVICE;
    } else if (validate) {
      int bad = 0;
      rc = count_bad(ctx, d_pbar, a.n, (int*)(p->d_small + SM_BAD), &bad);
      if (rc == SNARKV_OK && bad) {
        set_last_error("ipa_create_proof: %d of %zu scalars of p_bar are not canonical", bad, a.n);
        rc = SNARKV_ERR_ENCODING;
      }
    }
  }
  if (rc == SNARKV_OK) rc = create_enqueue_and_wait(ctx, dk, a, zk, need, p, (uint8_t*)d_cr, d_pbar, host);
  if (rc == SNARKV_OK) session_free(p);
  else session_close(p);  // a failure may have left work in flight
  if (d_cr) (void)hipFree(d_cr);
  if (d_pbar) (void)hipFree(d_pbar);
  if (rc != SNARKV_OK) return rc;
  uint32_t status;
  memcpy(&status, host.data(), 4);
  if (status) {
    set_last_error("ipa_create_proof: cannot write points at infinity to the transcript (%s)",
                   status & kStatusCbarInf ? "c_bar" : (status & kStatusRoundInf ? "L or R of a round" : "U"));
    return SNARKV_ERR_ENCODING;
  }
  memcpy(u_out64, &host[CR_U - CR_STATUS], 64);
  memcpy(xi_out32, &host[CR_XI - CR_STATUS], 32 * (size_t)k);
  memcpy(proof_out, &host[CR_PROOF - CR_STATUS], need);
  *proof_len = need;
  return SNARKV_OK;
}

}  // namespace
}  // namespace snarkv

using namespace snarkv;

extern "C" {

int SNARKV_API(ipa_create_proof)(snarkv_ctx* ctx, const snarkv_ipa_dk* dk, const uint8_t h64[64], const uint8_t* s64,
                                 const uint8_t* coeffs32, size_t n, const uint8_t z32[32], const uint8_t* omega32,
                                 const uint8_t* pbar32, const uint8_t* omega_bar32, const uint8_t* absorbed,
                                 size_t absorbed_len, uint8_t* proof_out, size_t proof_cap, size_t* proof_len,
                                 uint8_t* xi_out32, uint8_t u_out64[64]) {
  const CreateArgs a = {h64, s64, z32, omega32, omega_bar32, absorbed, coeffs32, pbar32, false, n, absorbed_len};
  return create_proof(ctx, dk, a, proof_out, proof_cap, proof_len, xi_out32, u_out64);
}

int SNARKV_API(ipa_create_proof_dev)(snarkv_ctx* ctx, const snarkv_ipa_dk* dk, const uint8_t h64[64], const uint8_t* s64,
                                     const void* d_coeffs32, size_t n, const uint8_t z32[32], const uint8_t* omega32,
                                     const void* d_pbar32, const uint8_t* omega_bar32, const uint8_t* absorbed,
                                     size_t absorbed_len, uint8_t* proof_out, size_t proof_cap, size_t* proof_len,
                                     uint8_t* xi_out32, uint8_t u_out64[64]) {
  const CreateArgs a = {h64, s64, z32, omega32, omega_bar32, absorbed, d_coeffs32, d_pbar32, true, n, absorbed_len};
  return create_proof(ctx, dk, a, proof_out, proof_cap, proof_len, xi_out32, u_out64);
}

}  // extern "C"
