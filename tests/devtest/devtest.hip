// Device build of the raw-record operations of tests/hosttest/curve_ops.h: one trivial kernel per operation, one lane per
// record, and a C launcher per kernel (device pointers + count in, HIP status out).  Built by snark-verifier_amd/build.py in
// four flavours: {BN254, pallas} x {asm multiplier bodies, -DSNARKV_NO_SMAD_ASM}; the BN254 flavours also hold the pairing
// decider's lane pieces and its two rounds (k_wt_round, k_coop3_round).  Test infrastructure only: no product symbol lives here.
#include <hip/hip_runtime.h>
#include "../hosttest/curve_ops.h"

namespace snarkv {
namespace devtest {

constexpr int kBlock = 256;

#define DT_KERNEL(name, IN, OUT)                                                      \
  __global__ __launch_bounds__(kBlock) void k_##name(const int32_t* in, int32_t* out, int n) { \
    const int i = blockIdx.x * kBlock + threadIdx.x;                                  \
    if (i >= n) return;                                                               \
    int32_t a[IN], r[OUT];                                                            \
    for (int j = 0; j < IN; ++j) a[j] = in[(size_t)i * IN + j];                       \
    rawops::op_##name(a, r);                                                          \
    for (int j = 0; j < OUT; ++j) out[(size_t)i * OUT + j] = r[j];                    \
  }
SNARKV_RAW_OPS(DT_KERNEL)
SNARKV_RAW_DECIDER_OPS(DT_KERNEL)
#undef DT_KERNEL

// jac29_double_quad next to jac29_double: record i is held uniformly by the four lanes 4i .. 4i+3 (an aligned quad); every
// lane of the grid runs the doubling (records past the end are clamped to the last one, so no lane of a quad is missing
// from the DPP exchange) and lane (i & 3) of quad i stores, so all four lane positions get looked at.
// in: x, y, z (27 words); out: quad x, y, z then plain x, y, z (54 words)
__global__ __launch_bounds__(kBlock) void k_jac29_double_quad(const int32_t* in, int32_t* out, int n) {
  const int lane = blockIdx.x * kBlock + threadIdx.x;
  const int i = lane >> 2;
  const int src = i < n ? i : n - 1;
  Fq29 x = rawops::ldq(in + (size_t)src * 27), y = rawops::ldq(in + (size_t)src * 27 + 9),
       z = rawops::ldq(in + (size_t)src * 27 + 18);
  Fq29 px = x, py = y, pz = z;
  jac29_double_quad(x, y, z, (uint32_t)(lane & 3));
  jac29_double(px, py, pz);
  if (i < n && (lane & 3) == (i & 3)) {
    int32_t* o = out + (size_t)i * 54;
    rawops::stq(x, o);
    rawops::stq(y, o + 9);
    rawops::stq(z, o + 18);
    rawops::stq(px, o + 27);
    rawops::stq(py, o + 36);
    rawops::stq(pz, o + 45);
  }
}

#if !defined(SNARKV_CURVE_PALLAS)
// One round of k_decide_w (decider.hip) on a raw record, one workgroup = one duo per record: the record's A and B go into
// LDS as Fq29P values at 0 and 24, dst is 48; then wt_task_c, group8_sum, wt_squeeze, row_ror:8, wt_write exactly in the
// order of the product kernel's loop body.
__global__ __launch_bounds__(128) void k_wt_round(const int32_t* in, int32_t* out, int n) {
  __shared__ Fq29P lds[72];
  const int tid = threadIdx.x, lane = tid & 63, half = tid >> 6;
  const int rec = blockIdx.x;
  if (rec >= n) return;
  const int32_t* r = in + (size_t)rec * kWtRoundIn;
  for (int j = tid; j < 48 * 9; j += 128) lds[j / 9].v[j % 9] = r[j];
  for (int j = tid; j < 24 * 9; j += 128) lds[48 + j / 9].v[j % 9] = 0;
  WtOp op;
  op.a = 0, op.b = 24, op.dst = 48, op.kind = (uint8_t)r[432], op.flags = (uint8_t)r[433];
  __syncthreads();
  const WtLaneC LC = wt_lane_c(half, lane);
  const Fq29 own = wt_squeeze(group8_sum(wt_task_c(lds, op, LC)));
  Fq29 other;  // the other u-component of the same power of w: 8 lanes away in the row
#pragma unroll
  for (int q = 0; q < 9; ++q) other.v[q] = (int32_t)dpp_u32<0x128>((uint32_t)own.v[q]);  // row_ror:8
  wt_write(lds, op, half, lane, own, other);
  __syncthreads();
  for (int j = tid; j < 24 * 9; j += 128) out[(size_t)rec * kWtRoundOut + j] = lds[48 + j / 9].v[j % 9];
}

// One round of k_decide (decider.hip coop_mul_b) on a raw record: A and B in LDS; with mode 1 B is a sparse line whose
// w^0 and w^1 come from LDS and whose w^3 is read from global memory, as the kernel reads cw from the key.
__global__ __launch_bounds__(128) void k_coop3_round(const int32_t* in, int32_t* out, int n) {
  __shared__ Fq29 a[12], b[12];
  const int tid = threadIdx.x;
  const int rec = blockIdx.x;
  if (rec >= n) return;
  const int32_t* r = in + (size_t)rec * kCoop3RoundIn;
  for (int j = tid; j < 12 * 9; j += 128) a[j / 9].v[j % 9] = r[j], b[j / 9].v[j % 9] = r[108 + j];
  const bool line = r[216] != 0;
  __syncthreads();
  const Coop3Lane L = coop3_lane(tid);
  Fq29 val = fq29_zero();
  if (L.active) {
    const Fq29& a0 = a[2 * L.i1];
    const Fq29& a1 = a[2 * L.i1 + 1];
    const int c0 = 2 * L.i2 + L.e, c1 = 2 * L.i2 + 1 - L.e;
    if (!line) {
      val = coop3_product(L.e, a0, a1, b[c0], b[c1]);
    } else if (L.i2 < 2 || L.i2 == 3) {
      Fq29 y0, y1;
      if (L.i2 < 2) {
        y0 = b[c0];
        y1 = b[c1];
      } else {
        y0 = rawops::ldq(r + 108 + 9 * (6 + L.e));
        y1 = rawops::ldq(r + 108 + 9 * (7 - L.e));
      }
      val = coop3_product(L.e, a0, a1, y0, y1);
    }
  }
  Fq29 lo, hi;
#pragma unroll
  for (int i = 0; i < 9; ++i) {
    lo.v[i] = L.high ? 0 : val.v[i];
    hi.v[i] = L.high ? val.v[i] : 0;
  }
  lo = group8_sum(lo);
  hi = group8_sum(hi);
  Fq29 hp;  // the high sum of the other u-power: 8 lanes away in the same row
#pragma unroll
  for (int i = 0; i < 9; ++i) hp.v[i] = (int32_t)dpp_u32<0x128>((uint32_t)hi.v[i]);  // row_ror:8
  if ((tid & 7) == 0 && L.k < 6) rawops::stq(coop3_finalize(L.e, lo, hi, hp), out + (size_t)rec * kCoop3RoundOut + 9 * (2 * L.k + L.e));
}
#endif

static int finish() {
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return (int)e;
  return (int)hipDeviceSynchronize();
}

}  // namespace devtest
}  // namespace snarkv

extern "C" {
const char* dt_curve() { return SNARKV_CURVE_NAME; }
int dt_asm_bodies() {
#if defined(SNARKV_NO_SMAD_ASM)
  return 0;
#else
  return 1;
#endif
}
#define DT_LAUNCH(name, IN, OUT)                                                                          \
  int dt_##name(const int32_t* in, int32_t* out, int n) {                                                 \
    if (n <= 0) return 0;                                                                                 \
    snarkv::devtest::k_##name<<<dim3((n + snarkv::devtest::kBlock - 1) / snarkv::devtest::kBlock),        \
                                dim3(snarkv::devtest::kBlock), 0, 0>>>(in, out, n);                       \
    return snarkv::devtest::finish();                                                                     \
  }                                                                                                       \
  int dt_##name##_io() { return (IN << 16) | OUT; }
SNARKV_RAW_OPS(DT_LAUNCH)
SNARKV_RAW_DECIDER_OPS(DT_LAUNCH)
#undef DT_LAUNCH
#if !defined(SNARKV_CURVE_PALLAS)
int dt_wt_round(const int32_t* in, int32_t* out, int n) {
  if (n <= 0) return 0;
  snarkv::devtest::k_wt_round<<<dim3(n), dim3(128), 0, 0>>>(in, out, n);
  return snarkv::devtest::finish();
}
int dt_wt_round_io() { return (kWtRoundIn << 16) | kWtRoundOut; }
int dt_coop3_round(const int32_t* in, int32_t* out, int n) {
  if (n <= 0) return 0;
  snarkv::devtest::k_coop3_round<<<dim3(n), dim3(128), 0, 0>>>(in, out, n);
  return snarkv::devtest::finish();
}
int dt_coop3_round_io() { return (kCoop3RoundIn << 16) | kCoop3RoundOut; }
#endif
int dt_jac29_double_quad(const int32_t* in, int32_t* out, int n) {
  if (n <= 0) return 0;
  const int lanes = 4 * n;
  snarkv::devtest::k_jac29_double_quad<<<dim3((lanes + snarkv::devtest::kBlock - 1) / snarkv::devtest::kBlock),
                                         dim3(snarkv::devtest::kBlock), 0, 0>>>(in, out, n);
  return snarkv::devtest::finish();
}
}
