// The MXFP8 / e4m3 quantisation rule as device code, shared by the MXFP8 GEMM and quantiser (mx8.hip) and the fp8 attention's
// MXFP8 output (attn.hip).  The rule itself: include/pandora_mi355x.h, "MXFP8"; restated in numpy by tests/test_mx8_cpu.py.
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

// e4m3fn code of ANY f32 (the packed fp8 attention operands, include/pandora_mi355x.h "packed fp8 attention operands"):
// clamp to +-448 (infinities included), then e4m3_rne; NaN -> 0x7F.
__device__ __forceinline__ uint32_t e4m3_sat(float y) {
  if (y != y) return 0x7fu;
  return e4m3_rne(fminf(fmaxf(y, -448.f), 448.f));
}

}  // namespace pm
