// tattn_kernel; included by attn.hip.
#pragma once
#include "attn_common.hpp"

namespace pm {
// Temporal self-attention: at every (pixel, head) a (Fq x Fk <= 16 x 16) attention over the frame
// axis, head dim 64.  HBM-bound (0.1 % of the FLOPs) - the job is to touch q, k, v, o once with wide
// loads and keep the arithmetic off the VALU:
//   one wave per (pixel, head) problem at a time, several problems per wave;
//   S^T = K . Q^T   2 x v_mfma_f32_16x16x32: both operands are 16-byte row pieces loaded straight from
//                   global memory in fragment order (lane = (frame, d-chunk)), no LDS;
//   softmax over the 16 keys: 4 scores per lane + two cross-lane exchanges (lane ^ 16, lane ^ 32);
//   O^T = V^T . P^T 4 x v_mfma_f32_16x16x16 (K = 16 keys, no padding): the S^T accumulator IS the P^T
//                   operand (same lane map), V^T fragments come from a wave-private 2 KiB LDS image of
//                   the [16 frames][64] V tile (filled by DMA) through ds_read_b64_tr_b16.
struct TAttnParams {
  const void* q;
  const void* k;
  const void* v;
  void* o;
  int64_t ldq, ldk, ldo;
  int Fq, Fk, P, heads;
  float scale_log2e;
  int nprob;  // P * heads
};

__device__ __forceinline__ f32x4 mfma16k16(f16x4 a, f16x4 b, f32x4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x16f16(a, b, c, 0, 0, 0);
}
__device__ __forceinline__ f32x4 mfma16k16(bf16x4 a, bf16x4 b, f32x4 c) {
  union { bf16x4 v; s16x4 s; } ua, ub;
  ua.v = a;
  ub.v = b;
  return __builtin_amdgcn_mfma_f32_16x16x16bf16_1k(ua.s, ub.s, c, 0, 0, 0);
}

template <typename T>
__global__ __launch_bounds__(256) void tattn_kernel(const TAttnParams p) {
  __shared__ __attribute__((aligned(16))) char smem[4 * 2048];  // one V image per wave
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  char* const vimg = smem + wave * 2048;
  const int fr = lane & 15, g = lane >> 4;  // fragment row (frame / d) and k-group
  const int64_t qfs = (int64_t)p.P * p.ldq, kfs = (int64_t)p.P * p.ldk, ofs = (int64_t)p.P * p.ldo;
  const T* Qg = reinterpret_cast<const T*>(p.q);
  const T* Kg = reinterpret_cast<const T*>(p.k);
  const T* Vg = reinterpret_cast<const T*>(p.v);
  T* Og = reinterpret_cast<T*>(p.o);
  const int fq_row = fr < p.Fq ? fr : p.Fq - 1;  // clamp: rows >= Fq are computed and dropped
  const int fk_row = fr < p.Fk ? fr : p.Fk - 1;
  // DMA of the V tile: instruction j fills keys 8j..8j+7 (lane i -> key 8j + i/8, physical 16-byte
  // slot i%8); the slot is XOR-ed by ((key>>1)&3)<<1 on the SOURCE side (conflict-free tr reads)
  const int dkey = lane >> 3, dslot = lane & 7;
  // transposed-read addresses: lane i of a 16-lane group supplies row (key 4g + i/4), columns 4(i&3)..
  const int tkey = 4 * g + (fr >> 2);
  const int tsw = ((tkey >> 1) & 3) << 1;

  const int waves_total = gridDim.x * 4;
  for (int prob = blockIdx.x * 4 + wave; prob < p.nprob; prob += waves_total) {
    const int pix = prob / p.heads, head = prob - pix * p.heads;
    const T* qp = Qg + (int64_t)pix * p.ldq + head * 64;
    const T* kp = Kg + (int64_t)pix * p.ldk + head * 64;
    const T* vp = Vg + (int64_t)pix * p.ldk + head * 64;
    // V tile -> LDS (2 x 1 KiB)
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      int key = 8 * j + dkey;
      const int lslot = dslot ^ (((key >> 1) & 3) << 1);
      if (key > p.Fk - 1) key = p.Fk - 1;
      __builtin_amdgcn_global_load_lds((glb_void*)(vp + key * kfs + lslot * 8), (lds_void*)(vimg + j * 1024), 16, 0, 0);
    }
    // S^T = K . Q^T
    f32x4 st = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      Pack8<T> kf, qf;
      kf.u = ld_global16(kp + fk_row * kfs + 32 * ks + 8 * g);
      qf.u = ld_global16(qp + fq_row * qfs + 32 * ks + 8 * g);
      st = mfma16(kf.v, qf.v, st);
    }
    // st[r] = score(key = 4g + r, query = fr); softmax over keys in base 2
    float sc[4], mx = -INFINITY;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      sc[r] = (4 * g + r < p.Fk) ? st[r] * p.scale_log2e : -INFINITY;
      mx = fmaxf(mx, sc[r]);
    }
    mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
    mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
    float l = 0.f;
    Pack4<T> pf;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const float e = __builtin_amdgcn_exp2f(sc[r] - mx);
      l += e;
      pf.e[r] = from_f32<T>(e);
    }
    l += __shfl_xor(l, 16, 64);
    l += __shfl_xor(l, 32, 64);
    const float inv = __builtin_amdgcn_rcpf(l);
    // O^T = V^T . P^T
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // the V image has landed (wave-private: no barrier)
    T* op = Og + (int64_t)pix * p.ldo + head * 64 + fr * ofs;
#pragma unroll
    for (int db = 0; db < 4; ++db) {
      const int chunk = (2 * db + ((fr & 3) >> 1)) ^ tsw;
      union { s16x4 s; typename Vec<T>::v4 v; } vf;
      vf.s = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(vimg + tkey * 128 + chunk * 16 + (fr & 1) * 8));
      f32x4 ot = {0.f, 0.f, 0.f, 0.f};
      ot = mfma16k16(vf.v, pf.v, ot);
      // ot[r] = O[query fr][d = 16 db + 4g + r]
      Pack4<T> ov;
#pragma unroll
      for (int r = 0; r < 4; ++r) ov.e[r] = from_f32<T>(ot[r] * inv);
      if (fr < p.Fq) *reinterpret_cast<u32x2*>(op + 16 * db + 4 * g) = ov.u;
    }
  }
}

}  // namespace pm
