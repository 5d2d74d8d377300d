// Shared definitions of the head-dim-64 attention kernels (attn_cross / attn_self / attn_fp8.hpp: 32x32 MFMA forms, one unit
// with the host side in attn.hip; attn16.hip: the 16x16x32 form).
#pragma once
#include <stdlib.h>
#include <math.h>
#include <type_traits>
#include "common.hpp"

namespace pm {

struct AttnParams {
  const void* q;
  const void* k[2];
  const void* v[2];
  void* o;
  int64_t q_bs, q_rs, o_bs, o_rs;
  int64_t k_bs[2], k_rs[2];
  int Nk[2];
  float w[2];
  int nseg;
  int Nq, heads, nqt;
  float scale_log2e;
  int prescaled;  // attn_self_kernel: q already carries scale * log2(e) (scale_log2e == 1)
  // diagnostics build only (pm_debug_attn_stamps, include/pandora_mi355x_diag.h; nullptr otherwise): per workgroup
  // {d s_memtime, d s_memrealtime} over the kernel body - the clock the chip holds under this instruction stream
  unsigned long long* stamps;
};

int launch_attn_self16(const AttnParams& p, int dtype, dim3 grid, hipStream_t stream, int form = 0);  // attn16.hip

constexpr int KV_TILE = 64;
constexpr int KV_TILE_BYTES = KV_TILE * 128;  // 64 keys x 64 dims x 2 B

typedef __attribute__((address_space(3))) s16x4 lds_s16x4;
typedef __attribute__((address_space(3))) void lds_void;
typedef const __attribute__((address_space(1))) void glb_void;

// value held by lane ^ 32 (v_permlane32_swap: no LDS round trip)
__device__ __forceinline__ float other_half(float v) {
  const unsigned u = __float_as_uint(v);
  auto r = __builtin_amdgcn_permlane32_swap(u, u, false, false);
  return __uint_as_float((threadIdx.x & 32) ? r[0] : r[1]);
}

// 1-D grid, XCD-aware: blocks are dealt round-robin over the 8 XCDs, so give each XCD a contiguous
// run of ids = all query tiles of the same (frame, head) -> its K/V (re-read by every query tile)
// stays in that XCD's L2 instead of being fetched by all eight
struct AttnWork { int bh, qt, b, head; };  // (batch element, head) pair bh = b * heads + head, its query tile qt
__device__ __forceinline__ int xcd_workgroup() {
  const int wg = blockIdx.x, nwg = gridDim.x, qn = nwg >> 3, rn = nwg & 7, xcd = wg & 7;
  return ((xcd < rn) ? xcd * (qn + 1) : rn * (qn + 1) + (xcd - rn) * qn) + (wg >> 3);
}
__device__ __forceinline__ AttnWork attn_work(int wg, int nqt, int heads) {
  AttnWork w;
  w.bh = wg / nqt; w.qt = wg - w.bh * nqt;
  w.b = w.bh / heads; w.head = w.bh - w.b * heads;
  return w;
}

// a lane's query row: rows past the sequence load the last row and are not stored (valid = false)
__device__ __forceinline__ void clamp_qrow(int& row, bool& valid, int Nq) {
  valid = row < Nq;
  if (!valid) row = Nq - 1;
}

// AttnParams::prescaled == 0 (general callers): one extra 16-bit rounding of q * scale * log2(e)
template <typename T, int QB, int S> __device__ __forceinline__ void scale_q(Pack8<T> (&qf)[QB][S], float scale_log2e) {
#pragma unroll
  for (int qb = 0; qb < QB; ++qb)
#pragma unroll
    for (int s = 0; s < S; ++s)
#pragma unroll
      for (int e = 0; e < 8; ++e) qf[qb][s].e[e] = from_f32<T>(to_f32(qf[qb][s].e[e]) * scale_log2e);
}

template <typename T> __device__ __forceinline__ typename Vec<T>::v8 tr_pair(const char* base, int off0, int off1) {
  // two transposed 4x16 block reads -> 8 keys of one d column (the 32x32x16 A-operand fragment)
  union {
    struct { s16x4 lo, hi; } s;
    typename Vec<T>::v8 v;
  } u;
  u.s.lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(base + off0));
  u.s.hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(base + off1));
  return u.v;
}


// 32x32 accumulator layout (attn_cross.hpp, attn_self.hpp, attn_fp8.hpp): one query row's 64 outputs of the 32x32 layout, o[db][r] * inv <-> d = db*32 + (r&3) + 8*(r>>2) + 4*hh, to op[0 .. 63]
template <typename T> __device__ __forceinline__ void store_row32(T* op, const f32x16 (&o)[2], float inv, int hh) {
#pragma unroll
  for (int db = 0; db < 2; ++db)
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      Pack4<T> ov;
#pragma unroll
      for (int e = 0; e < 4; ++e) ov.e[e] = from_f32<T>(o[db][4 * g + e] * inv);
      *reinterpret_cast<u32x2*>(op + db * 32 + 8 * g + 4 * hh) = ov.u;
    }
}

}  // namespace pm
