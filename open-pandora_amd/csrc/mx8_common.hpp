// The MXFP8 / e4m3 quantisation rule as device code, shared by the MXFP8 GEMM and quantiser (mx8.hip), the fp8 attention's
// MXFP8 output (attn_fp8.hpp) and the GroupNorm-apply quantiser (norm.hip).  The rule itself: include/pandora_mi355x.h, "MXFP8"; restated in numpy by tests/test_mx8_cpu.py.
#pragma once
#include "common.hpp"

namespace pm {

// Scale exponent of a block with amax a (finite): X = clamp(ceil(log2(a / 448)), -127, 127), exactly: a = 1.m * 2^e gives
// X = e - 8 + (1.m > 1.75).  f32 subnormal a (and a = 0) give -127 (E8M0 code 0).
__device__ __forceinline__ int mx8_exp(float amax) {
  const uint32_t b = __float_as_uint(amax);
  const int e = (int)((b >> 23) & 0xff);
  if (e == 0) return -127;
  const int X = e - 135 + ((b & 0x7fffff) > 0x600000u ? 1 : 0);
  return X < -127 ? -127 : (X > 127 ? 127 : X);
}
// 2^-X as an f32 (X in [-127, 120] for finite inputs: always a normal number)
__device__ __forceinline__ float mx8_inv_scale(int X) { return __uint_as_float((uint32_t)(127 - X) << 23); }
// e4m3fn code of y (|y| <= 448, finite), round to nearest even, subnormals (steps of 2^-9) included.  In software so that the
// result does not depend on the hardware converter's tie / subnormal handling.
__device__ __forceinline__ uint32_t e4m3_rne(float y) {
  uint32_t b = __float_as_uint(y);
  const uint32_t s = (b >> 24) & 0x80u;
  b &= 0x7fffffffu;
  if (b >= 0x3c800000u) {  // |y| >= 2^-6: normal
    b += 0x7ffffu + ((b >> 20) & 1u);
    return s | (((b >> 23) - 120u) << 3) | ((b >> 20) & 7u);
  }
  return s | (uint32_t)__builtin_rintf(__uint_as_float(b) * 512.0f);  // 8 -> 0x08 = 2^-6, the smallest normal
}
__device__ __forceinline__ bool finite_f(float v) { return fabsf(v) <= 3.402823466e38f; }  // (false for NaN)

// One block of 32 values spread over 4 lanes (8 each) that differ in lane-index bits O1 and O2: E8M0 code of the block and the
// 8 e4m3 codes of this lane (two little-endian words).  A block holding a NaN or an Inf: code 0xFF and NaN (0x7F) elements.
template <int O1, int O2>
__device__ __forceinline__ uint32_t mx8_block(const float (&v)[8], uint32_t& w0, uint32_t& w1) {
  float amax = 0.f;
  int bad = 0;
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    amax = fmaxf(amax, fabsf(v[e]));
    bad |= finite_f(v[e]) ? 0 : 1;
  }
  amax = fmaxf(amax, __shfl_xor(amax, O1, 64));
  amax = fmaxf(amax, __shfl_xor(amax, O2, 64));
  bad |= __shfl_xor(bad, O1, 64);
  bad |= __shfl_xor(bad, O2, 64);
  if (bad) {
    w0 = w1 = 0x7f7f7f7fu;
    return 0xffu;
  }
  const int X = mx8_exp(amax);
  const float inv = mx8_inv_scale(X);
  uint32_t c[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) c[e] = e4m3_rne(v[e] * inv);  // (exact product: a power of two, result >= 2^-126 or irrelevant)
  w0 = c[0] | (c[1] << 8) | (c[2] << 16) | (c[3] << 24);
  w1 = c[4] | (c[5] << 8) | (c[6] << 16) | (c[7] << 24);
  return (uint32_t)(X + 127);
}

// e4m3fn code of ANY f32 (the packed fp8 attention operands, include/pandora_mi355x.h "packed fp8 attention operands"):
// clamp to +-448 (infinities included), then e4m3_rne; NaN -> 0x7F.
__device__ __forceinline__ uint32_t e4m3_sat(float y) {
  if (y != y) return 0x7fu;
  return e4m3_rne(fminf(fmaxf(y, -448.f), 448.f));
}

}  // namespace pm
