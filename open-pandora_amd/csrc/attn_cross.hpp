// Flash-style attention for head dim 64 on gfx950 (spatial self-attention and the text+image
// cross-attention of the 3-D U-Net).  No score matrix ever reaches HBM.
//
// Workgroup = 4 waves, 128 query rows (32 per wave); K/V tiles of 64 keys are staged
// global -> VGPR -> LDS (two buffers, one barrier per tile).
//   S^T = K . Q^T      v_mfma_f32_32x32x16 with K as the A operand ("swapped QK^T"): every lane then
//                      owns ONE query row (col = lane & 31) and 32 of the tile's 64 scores, so the
//                      row max / row sum are in-lane reductions plus one exchange with lane ^ 32.
//   O^T += V^T . P^T   the S^T accumulator is re-used in place as the B operand (no LDS round trip,
//                      cdna guide §3 "accumulator tile as the next MFMA's operand"); V^T fragments
//                      come from the row-major V tile through ds_read_b64_tr_b16.
// Two key/value segments (text, image) are normalised independently and summed (attention.py:128-142).  (attn_kernel; included by attn.hip)
#pragma once
#include "attn_common.hpp"

namespace pm {
// QB = 32-row query blocks per wave.  QB = 1: 128 query rows per workgroup (short sequences, the
// two-segment cross-attention).  QB = 2: 256 rows per workgroup - every K / V^T fragment read from LDS
// feeds two MFMAs and the two blocks' MFMA and softmax chains are independent, so the scheduler can
// overlap one block's exp/max/convert VALU work with the other's matrix work (the kernel is
// VALU-issue-bound at head dim 64: ~13 VALU per 32x32x16 MFMA).
template <typename T, int QB, bool SEG2>
__global__ __launch_bounds__(256, 2) void attn_kernel(const AttnParams p) {
  __shared__ __attribute__((aligned(16))) char smem[4 * KV_TILE_BYTES];  // K[2], V[2]
  char* const Ks = smem;
  char* const Vs = smem + 2 * KV_TILE_BYTES;

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int ql = lane & 31, hh = lane >> 5;
  const AttnWork w = attn_work(xcd_workgroup(), p.nqt, p.heads);
  const int qt = w.qt, b = w.b, head = w.head;

  // Q^T fragments (B operand): element j of k-step s = Q[qrow][16 s + 8 hh + j]
  int qrow[QB];
  bool q_valid[QB];
  Pack8<T> qf[QB][4];
#pragma unroll
  for (int qb = 0; qb < QB; ++qb) {
    qrow[qb] = qt * (128 * QB) + wave * (32 * QB) + qb * 32 + ql;
    clamp_qrow(qrow[qb], q_valid[qb], p.Nq);
    const T* qp = reinterpret_cast<const T*>(p.q) + (int64_t)b * p.q_bs + (int64_t)qrow[qb] * p.q_rs +
                  head * 64 + 8 * hh;
#pragma unroll
    for (int s = 0; s < 4; ++s) qf[qb][s].u = ld_global16(qp + 16 * s);
  }

  // staging coordinates
  const int lc = tid & 7, lr = tid >> 3;  // chunk, row (+32)

  // two-segment (text + image) calls sum the independently normalised segment outputs here
  f32x16 out[SEG2 ? QB : 1][2];
  if constexpr (SEG2) {
#pragma unroll
    for (int qb = 0; qb < QB; ++qb)
#pragma unroll
      for (int d = 0; d < 2; ++d)
#pragma unroll
        for (int r = 0; r < 16; ++r) out[qb][d][r] = 0.f;
  }

  for (int seg = 0; seg < (SEG2 ? p.nseg : 1); ++seg) {
    const int Nk = p.Nk[seg];
    // wave-uniform bases (this block's batch element and head); lanes add 32-bit byte offsets, so the DMAs use
    // the "scalar base + 32-bit lane offset" address form (a per-lane 64-bit address costs the DMA about twice
    // the issue time: measured on the GEMM loaders, profiles/r01/ring_gemm_inkernel_stamps.txt)
    const char* const kbase = reinterpret_cast<const char*>(reinterpret_cast<const T*>(p.k[seg]) + (int64_t)b * p.k_bs[seg] + head * 64);
    const char* const vbase = reinterpret_cast<const char*>(reinterpret_cast<const T*>(p.v[seg]) + (int64_t)b * p.k_bs[seg] + head * 64);
    const uint32_t krs2 = (uint32_t)(p.k_rs[seg] * 2);  // row stride in bytes (Nk * row bytes < 4 GiB: checked by the launcher)
    const int nkt = (Nk + KV_TILE - 1) / KV_TILE;

    // K/V tiles go global -> LDS by DMA (1 KiB per wave-instruction, lane-linear image); the XOR
    // swizzles are applied on the source side: this lane fills physical slot tid & 7 of rows
    // lr + 32 j with logical chunk  slot ^ ((row >> 1) & 7)  (K: conflict-free ds_read_b128 for the
    // 32-row MFMA operand) resp.  slot ^ (((row >> 1) & 1) << 2)  (V: conflict-free transposed reads).
    const int kc = (tid & 7) ^ ((lr >> 1) & 7);
    const int vc = (tid & 7) ^ (((lr >> 1) & 1) << 2);
    auto load_kv = [&](int kt, int buf) {  // (kept per kernel: profiles/attn_split/README.md)
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        int key = kt * KV_TILE + lr + 32 * j;
        if (key > Nk - 1) key = Nk - 1;
        const int dst = buf * KV_TILE_BYTES + (32 * j + 8 * wave) * 128;
        const uint32_t row = (uint32_t)key * krs2;
        __builtin_amdgcn_global_load_lds((glb_void*)(kbase + (row + (uint32_t)kc * 16)), (lds_void*)(Ks + dst), 16, 0, 0);
        __builtin_amdgcn_global_load_lds((glb_void*)(vbase + (row + (uint32_t)vc * 16)), (lds_void*)(Vs + dst), 16, 0, 0);
      }
    };

    f32x16 oacc[QB][2];
    float m_run[QB], l_run[QB];
#pragma unroll
    for (int qb = 0; qb < QB; ++qb) {
      m_run[qb] = -INFINITY;
      l_run[qb] = 0.f;
#pragma unroll
      for (int d = 0; d < 2; ++d)
#pragma unroll
        for (int r = 0; r < 16; ++r) oacc[qb][d][r] = 0.f;
    }

    load_kv(0, 0);
    __syncthreads();  // drains the DMA (vmcnt) before the barrier

    for (int kt = 0; kt < nkt; ++kt) {
      const int buf = kt & 1;
      if (kt + 1 < nkt) load_kv(kt + 1, buf ^ 1);
      const char* ks = Ks + buf * KV_TILE_BYTES;
      const char* vs = Vs + buf * KV_TILE_BYTES;

      // ---- S^T = K . Q^T (raw scores, f32); each K fragment serves every query block ----
      f32x16 sacc[QB][2];
#pragma unroll
      for (int kb = 0; kb < 2; ++kb) {
#pragma unroll
        for (int qb = 0; qb < QB; ++qb)
#pragma unroll
          for (int r = 0; r < 16; ++r) sacc[qb][kb][r] = 0.f;
        const int row = kb * 32 + ql;
#pragma unroll
        for (int s = 0; s < 4; ++s) {
          Pack8<T> kf;
          const int chunk = 2 * s + hh;
          kf.u = *reinterpret_cast<const u32x4*>(ks + row * 128 + ((chunk ^ ((row >> 1) & 7)) << 4));
#pragma unroll
          for (int qb = 0; qb < QB; ++qb) sacc[qb][kb] = mfma32(kf.v, qf[qb][s].v, sacc[qb][kb]);
        }
      }
      // sacc[qb][kb][r] <-> key = kt*64 + kb*32 + (r&3) + 8*(r>>2) + 4*hh, query = ql of block qb
      if (kt * KV_TILE + KV_TILE > Nk) {  // (kept per kernel: profiles/attn_split/README.md)
#pragma unroll
        for (int qb = 0; qb < QB; ++qb)
#pragma unroll
          for (int kb = 0; kb < 2; ++kb)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
              const int key = kt * KV_TILE + kb * 32 + (r & 3) + 8 * (r >> 2) + 4 * hh;
              if (key >= Nk) sacc[qb][kb][r] = -INFINITY;
            }
      }
      // ---- online softmax (base-2 domain) ----
#pragma unroll
      for (int qb = 0; qb < QB; ++qb) {
        float mx = sacc[qb][0][0];
#pragma unroll
        for (int kb = 0; kb < 2; ++kb)
#pragma unroll
          for (int r = 0; r < 16; ++r) mx = fmaxf(mx, sacc[qb][kb][r]);
        mx = fmaxf(mx, other_half(mx));
        const float m_new = fmaxf(m_run[qb], mx * p.scale_log2e);
        // rescale only when some row's running max actually grew (alpha == 1 exactly otherwise)
        if (__builtin_amdgcn_ballot_w64(m_new > m_run[qb]) != 0) {
          const float alpha = __builtin_amdgcn_exp2f(m_run[qb] - m_new);
          l_run[qb] *= alpha;
#pragma unroll
          for (int d = 0; d < 2; ++d)
#pragma unroll
            for (int r = 0; r < 16; ++r) oacc[qb][d][r] *= alpha;
          m_run[qb] = m_new;
        }
        float psum = 0.f;
#pragma unroll
        for (int kb = 0; kb < 2; ++kb)
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            const float pv = __builtin_amdgcn_exp2f(sacc[qb][kb][r] * p.scale_log2e - m_run[qb]);
            sacc[qb][kb][r] = pv;
            psum += pv;
          }
        l_run[qb] += psum;
      }

      // ---- O^T += V^T . P^T; each V^T fragment serves every query block ----
      const int trow = (lane & 15) >> 2;                 // row inside the 4x16 block
      const int tcol8 = ((lane >> 4) & 1) * 2 + ((lane & 3) >> 1);  // 16-byte chunk inside the d-block
      const int tsub = (lane & 1) * 8;                   // byte inside the chunk
#pragma unroll
      for (int s4 = 0; s4 < 4; ++s4) {
        Pack8<T> pf[QB];
        const int kb = s4 >> 1, sp = s4 & 1;
#pragma unroll
        for (int qb = 0; qb < QB; ++qb)
#pragma unroll
          for (int j = 0; j < 8; ++j) pf[qb].e[j] = from_f32<T>(sacc[qb][kb][8 * sp + j]);
#pragma unroll
        for (int db = 0; db < 2; ++db) {
          const int r0 = 16 * s4 + 4 * hh + trow;
          const int r1 = r0 + 8;
          const int ch = db * 4 + tcol8;
          const int off0 = r0 * 128 + ((ch ^ (((r0 >> 1) & 1) << 2)) << 4) + tsub;
          const int off1 = r1 * 128 + ((ch ^ (((r1 >> 1) & 1) << 2)) << 4) + tsub;
          typename Vec<T>::v8 vf = tr_pair<T>(vs, off0, off1);
#pragma unroll
          for (int qb = 0; qb < QB; ++qb) oacc[qb][db] = mfma32(vf, pf[qb].v, oacc[qb][db]);
        }
      }
      __syncthreads();
    }
    // oacc[qb][db][r] <-> d = db*32 + (r&3) + 8*(r>>2) + 4*hh for query row ql of block qb
#pragma unroll
    for (int qb = 0; qb < QB; ++qb) {
      const float l_tot = l_run[qb] + other_half(l_run[qb]);
      const float inv = p.w[seg] / l_tot;
      if constexpr (SEG2) {
#pragma unroll
        for (int d = 0; d < 2; ++d)
#pragma unroll
          for (int r = 0; r < 16; ++r) out[qb][d][r] += oacc[qb][d][r] * inv;
        if (seg + 1 < p.nseg) continue;
      }
      if (q_valid[qb]) {
        T* op = reinterpret_cast<T*>(p.o) + (int64_t)b * p.o_bs + (int64_t)qrow[qb] * p.o_rs + head * 64;
        if constexpr (SEG2) store_row32(op, out[qb], 1.0f, hh);  // (already normalised, summed over the segments)
        else store_row32(op, oacc[qb], inv, hh);
      }
    }
  }
}

}  // namespace pm
