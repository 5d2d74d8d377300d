// Shared device helpers for the gfx950 kernels (wave64, MFMA, LDS).  gfx950 only: no portability
// layers.  See include/pandora_mi355x.h for the C-ABI.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>
#include <atomic>
#include "../../include/pandora_mi355x.h"
#ifdef PM_DIAG
#include "../../include/pandora_mi355x_diag.h"
#endif

namespace pm {

// Tuning overrides and diagnosis switches exist only in the -DPM_DIAG build (libpandora_mi355x_diag.so, build.py
// --diag): the SHIPPED library reads no environment variable and carries no mutable process-wide state besides
// write-once per-device caches (re-entrant, no global mutable state; gradio calls from a worker thread).
#ifdef PM_DIAG
inline const char* diag_env(const char* name) { return getenv(name); }
constexpr bool PM_DIAG_BUILD = true;
#else
inline const char* diag_env(const char*) { return nullptr; }
constexpr bool PM_DIAG_BUILD = false;
#endif

typedef _Float16 f16;
typedef __bf16 bf16;

typedef __attribute__((ext_vector_type(8))) _Float16 f16x8;
typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;
typedef __attribute__((ext_vector_type(4))) _Float16 f16x4;
typedef __attribute__((ext_vector_type(4))) __bf16 bf16x4;
typedef __attribute__((ext_vector_type(4))) float f32x4;
typedef __attribute__((ext_vector_type(16))) float f32x16;
typedef __attribute__((ext_vector_type(4))) unsigned int u32x4;
typedef __attribute__((ext_vector_type(2))) unsigned int u32x2;
typedef __attribute__((ext_vector_type(4))) short s16x4;

template <typename T> struct Vec;
template <> struct Vec<f16> {
  typedef f16x8 v8;
  typedef f16x4 v4;
};
template <> struct Vec<bf16> {
  typedef bf16x8 v8;
  typedef bf16x4 v4;
};

// 16-byte bag of eight 16-bit elements, reinterpretable as the MFMA operand vector.
template <typename T> union Pack8 {
  u32x4 u;
  typename Vec<T>::v8 v;
  T e[8];
};
template <typename T> union Pack4 {
  u32x2 u;
  typename Vec<T>::v4 v;
  T e[4];
};

template <typename T> __device__ __forceinline__ float to_f32(T x) { return static_cast<float>(x); }
template <typename T> __device__ __forceinline__ T from_f32(float x) { return static_cast<T>(x); }

__device__ __forceinline__ f32x4 mfma16(f16x8 a, f16x8 b, f32x4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, c, 0, 0, 0);
}
__device__ __forceinline__ f32x4 mfma16(bf16x8 a, bf16x8 b, f32x4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0);
}
__device__ __forceinline__ f32x16 mfma32(f16x8 a, f16x8 b, f32x16 c) {
  return __builtin_amdgcn_mfma_f32_32x32x16_f16(a, b, c, 0, 0, 0);
}
__device__ __forceinline__ f32x16 mfma32(bf16x8 a, bf16x8 b, f32x16 c) {
  return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0);
}

__device__ __forceinline__ float silu_f(float x) {
  return x * __builtin_amdgcn_rcpf(1.0f + __expf(-x));
}
// erf-GELU (attention.py:422, F.gelu default): gelu(x) = x Phi(x) = relu(x) - |x| Q(|x|), Q(t) = 0.5 erfc(t / sqrt 2).
// r06: Q(t) = 2^P(t) with P a degree-5 weighted-minimax fit of log2 Q on t >= 0 (weights = what an error of
// P costs in erf and in gelu; tools/erf_fit.py): |erf error| <= 9e-7, |gelu error| <= 8e-7 over the reals (P -> -inf, so the
// tail is exactly relu), ONE transcendental (v_exp_f32) and 8 full-rate ops - the Abramowitz-Stegun 7.1.26 form it replaces
// (v_exp + v_rcp + 14 ops, 1.5e-7) cost as many issue cycles per element as the whole K = 320 MFMA loop of a GEGLU tile.
// NaN propagates (relu as h + |h|); x = +-inf gives NaN (inf * 0) where the old form gave +inf / -0.
__device__ __forceinline__ float gelu_q_exp2(float t) {  // log2 of 0.5 erfc(t / sqrt 2), t >= 0
  float p = fmaf(-0.0005101419295911639f, t, 0.007342507309409537f);
  p = fmaf(p, t, -0.052463149158147024f);
  p = fmaf(p, t, -0.45932433014520657f);
  p = fmaf(p, t, -1.151073326450374f);
  return fmaf(p, t, -1.0000011294044768f);
}
__device__ __forceinline__ float gelu_erf_f(float x) {
  const float t = fabsf(x);
  const float q = __builtin_amdgcn_exp2f(gelu_q_exp2(t));
  const float h = 0.5f * x;
  return fmaf(-t, q, h + fabsf(h));
}
// erf itself through the same fit (tests: pm_debug_erf against an f64 erf, max abs <= 1e-5)
__device__ __forceinline__ float erf_fast_f(float z) {
  const float q = __builtin_amdgcn_exp2f(gelu_q_exp2(fabsf(z) * 1.41421356237309504880f));
  return copysignf(fmaf(-2.0f, q, 1.0f), z);
}

__device__ __forceinline__ u32x4 ld_global16(const void* p) {
  return *reinterpret_cast<const u32x4*>(p);
}
__device__ __forceinline__ void st_global16(void* p, u32x4 v) { *reinterpret_cast<u32x4*>(p) = v; }

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
  return v;
}

// ---- host: what every launcher needs of the current device.  The caches are write-once per slot (a race writes the same value
// twice); a device index outside them is served without a cache - queried / set on every call, never folded onto another slot.
constexpr int MAX_DEVICES = 64;
constexpr int MAX_LDS_KERNELS = 96;  // kernel instantiations that ask for more than 64 KiB of dynamic LDS (diagnostics build: ~50)

inline int current_device() {
  int dev = -1;
  return hipGetDevice(&dev) == hipSuccess ? dev : -1;
}

inline int num_cus() {
  static std::atomic<int> cus[MAX_DEVICES] = {};
  const int dev = current_device();
  const bool cached = dev >= 0 && dev < MAX_DEVICES;
  int n = cached ? cus[dev].load(std::memory_order_relaxed) : 0;
  if (n == 0) {
    if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev < 0 ? 0 : dev) != hipSuccess || n < 1) n = 256;
    if (cached) cus[dev].store(n, std::memory_order_relaxed);
  }
  return n;
}

// Allow kernel `fn` `bytes` of dynamic LDS on the current device (the attribute is per kernel AND per device; a process may drive
// several GPUs).  Set once per (kernel, device); a kernel or device the table has no room for gets it set on every call.
inline void raise_dynamic_lds(const void* fn, int bytes) {
  struct Slot {
    std::atomic<const void*> fn;
    std::atomic<bool> raised[MAX_DEVICES];
  };
  static Slot table[MAX_LDS_KERNELS] = {};
  const int dev = current_device();
  std::atomic<bool>* raised = nullptr;
  for (int i = 0; i < MAX_LDS_KERNELS && dev >= 0 && dev < MAX_DEVICES; ++i) {
    const void* owner = nullptr;  // the first free slot is claimed for `fn`
    if (table[i].fn.compare_exchange_strong(owner, fn) || owner == fn) {
      raised = &table[i].raised[dev];
      break;
    }
  }
  if (raised != nullptr && raised->load(std::memory_order_acquire)) return;
  (void)hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
  if (raised != nullptr) raised->store(true, std::memory_order_release);
}

inline int check_launch() { return hipGetLastError() == hipSuccess ? PM_OK : PM_E_LAUNCH; }

#define PM_DISPATCH_DTYPE(dtype, T, ...)  \
  do {                                    \
    if ((dtype) == PM_F16) {              \
      typedef pm::f16 T;                  \
      __VA_ARGS__;                        \
    } else if ((dtype) == PM_BF16) {      \
      typedef pm::bf16 T;                 \
      __VA_ARGS__;                        \
    } else {                              \
      return PM_E_DTYPE;                  \
    }                                     \
  } while (0)

}  // namespace pm
