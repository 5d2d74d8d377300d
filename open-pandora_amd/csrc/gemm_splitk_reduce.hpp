// The two split-K reduce kernels (second pass of a split pm_gemm / conv call); included by gemm.hip.
#pragma once
#include "gemm_common.hpp"

namespace pm {

// split-K second pass: out = epi(sum_s ws[s]) ; one thread per 4 consecutive columns
template <typename T>
__global__ __launch_bounds__(256) void splitk_reduce_kernel(const GemmParams p) {
  const int n4 = (p.N + 3) >> 2;
  const int64_t total = (int64_t)p.M * n4;
  const int64_t slab = (int64_t)p.M * p.N;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int64_t m = i / n4;
    const int n = (int)(i - m * n4) * 4;
    const float* src = p.ws + m * p.N + n;
    float v[4] = {0.f, 0.f, 0.f, 0.f};
    const bool vec = (n + 4 <= p.N) && ((p.N & 3) == 0);
    for (int s = 0; s < p.splits; ++s) {
      if (vec) {
        const f32x4 t = *reinterpret_cast<const f32x4*>(src + s * slab);
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] += t[e];
      } else {
        for (int e = 0; e < 4 && n + e < p.N; ++e) v[e] += src[s * slab + e];
      }
    }
    for (int e = 0; e < 4 && n + e < p.N; ++e) {
      float x = p.bias_mul ? v[e] * p.bias[n + e] : v[e] + (p.bias ? p.bias[n + e] : 0.f);
      if (p.act == PM_ACT_SILU) x = silu_f(x);
      if (p.act == PM_ACT_GELU) x = gelu_erf_f(x);
      if (p.R) x += p.res32 ? reinterpret_cast<const float*>(p.R)[m * p.ldr + n + e]
                            : to_f32(reinterpret_cast<const T*>(p.R)[m * p.ldr + n + e]);
      if (p.out32)
        reinterpret_cast<float*>(p.C)[m * p.ldc + n + e] = x;
      else
        reinterpret_cast<T*>(p.C)[m * p.ldc + n + e] = from_f32<T>(x);
    }
  }
}

// split-K second pass that also emits the fused GroupNorm column sums: grid (ceil(M/16), ceil(N/256)); the 256
// threads of a block are 64 column quads x 4 row lanes: a thread owns 4 consecutive columns of rows rl, rl+4,
// rl+8, rl+12 of a 16-row block (all its slab loads are independent and issued up front), sums the slabs in
// slab order, applies the epilogue, stores, and accumulates {sum, sum of squares} of exactly the values stored;
// the 4 row lanes are combined through LDS in lane order -> colstats [ceil(M/16)][N][2] (deterministic).
// (N % 4 == 0; the deep levels whose output has too few tiles to run unsplit are exactly the ones whose
// GroupNorms would otherwise need a separate statistics pass + finalize: 60 of the 166 per forward.)
template <typename T>
__global__ __launch_bounds__(256) void splitk_reduce_stats_kernel(const GemmParams p) {
  __shared__ float red[4][64][8];
  const int cq4 = threadIdx.x & 63, rl = threadIdx.x >> 6;
  const int n = (blockIdx.y * 64 + cq4) * 4;
  const int r0 = blockIdx.x * 16;
  const int64_t slab = (int64_t)p.M * p.N;
  const bool ncol = n < p.N;
  float cs[4] = {0.f, 0.f, 0.f, 0.f}, cq[4] = {0.f, 0.f, 0.f, 0.f};
  if (ncol) {
    f32x4 bias4 = f32x4{0.f, 0.f, 0.f, 0.f};
    if (p.bias) bias4 = *reinterpret_cast<const f32x4*>(p.bias + n);
    f32x4 v[4];
    bool live[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int m = r0 + rl + 4 * u;
      live[u] = m < p.M;
      v[u] = *reinterpret_cast<const f32x4*>(p.ws + (int64_t)(live[u] ? m : 0) * p.N + n);
    }
    for (int sidx = 1; sidx < p.splits; ++sidx) {
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int m = r0 + rl + 4 * u;
        const f32x4 t = *reinterpret_cast<const f32x4*>(p.ws + sidx * slab + (int64_t)(live[u] ? m : 0) * p.N + n);
#pragma unroll
        for (int e = 0; e < 4; ++e) v[u][e] += t[e];
      }
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      if (!live[u]) continue;
      const int m = r0 + rl + 4 * u;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        float x = p.bias_mul ? v[u][e] * bias4[e] : v[u][e] + bias4[e];
        if (p.act == PM_ACT_SILU) x = silu_f(x);
        if (p.act == PM_ACT_GELU) x = gelu_erf_f(x);
        v[u][e] = x;
      }
      if (p.R) {
        if (p.res32) {
          const f32x4 rr = *reinterpret_cast<const f32x4*>(reinterpret_cast<const float*>(p.R) + (int64_t)m * p.ldr + n);
#pragma unroll
          for (int e = 0; e < 4; ++e) v[u][e] += rr[e];
        } else {
          Pack4<T> rr;
          rr.u = *reinterpret_cast<const u32x2*>(reinterpret_cast<const T*>(p.R) + (int64_t)m * p.ldr + n);
#pragma unroll
          for (int e = 0; e < 4; ++e) v[u][e] += to_f32(rr.e[e]);
        }
      }
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        cs[e] += v[u][e];
        cq[e] = fmaf(v[u][e], v[u][e], cq[e]);
      }
      if (p.out32) {
        *reinterpret_cast<f32x4*>(reinterpret_cast<float*>(p.C) + (int64_t)m * p.ldc + n) = v[u];
      } else {
        Pack4<T> ov;
#pragma unroll
        for (int e = 0; e < 4; ++e) ov.e[e] = from_f32<T>(v[u][e]);
        *reinterpret_cast<u32x2*>(reinterpret_cast<T*>(p.C) + (int64_t)m * p.ldc + n) = ov.u;
      }
    }
  }
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    red[rl][cq4][2 * e] = cs[e];
    red[rl][cq4][2 * e + 1] = cq[e];
  }
  __syncthreads();
  if (rl == 0 && p.colstats != nullptr && p.gs_ni > 0) {
    // r06: GroupNorm totals by integer atomics (gemm_common.hpp).  This wave's 64 lanes hold 4 consecutive columns each, in
    // lane order; a 4-run can straddle a group boundary (10 or 30 channels per group): the part in the run's FIRST group goes
    // through the segmented wave sum, the rest (at most one lane per boundary) is added directly
    float o[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) o[e] = ((red[0][cq4][e] + red[1][cq4][e]) + red[2][cq4][e]) + red[3][cq4][e];
    const int cpg = p.N >> 5;
    const int g0 = ncol ? n / cpg : -1;
    float s0 = 0.f, q0 = 0.f, s1 = 0.f, q1 = 0.f;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const bool first = (n + e) / cpg == g0;
      s0 += first ? o[2 * e] : 0.f;
      q0 += first ? o[2 * e + 1] : 0.f;
      s1 += first ? 0.f : o[2 * e];
      q1 += first ? 0.f : o[2 * e + 1];
    }
    long long* base = reinterpret_cast<long long*>(p.colstats) + (int64_t)(r0 / p.gs_rows) * 32 * 4 * GS_STRIDE;
    gs_wave_add(base, s0, q0, g0, cq4);
    if (ncol && (n + 3) / cpg != g0 && n + 3 < p.N) {
      gs_atomic_add(base + (int64_t)(g0 + 1) * 4 * GS_STRIDE, s1);
      gs_atomic_add(base + ((int64_t)(g0 + 1) * 4 + 2) * GS_STRIDE, q1);
    }
  } else if (rl == 0 && ncol && p.colstats != nullptr) {
    float o[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) o[e] = ((red[0][cq4][e] + red[1][cq4][e]) + red[2][cq4][e]) + red[3][cq4][e];
    float* dst = p.colstats + ((int64_t)blockIdx.x * p.N + n) * 2;
    *reinterpret_cast<f32x4*>(dst) = f32x4{o[0], o[1], o[2], o[3]};
    *reinterpret_cast<f32x4*>(dst + 4) = f32x4{o[4], o[5], o[6], o[7]};
  }
}

}  // namespace pm
