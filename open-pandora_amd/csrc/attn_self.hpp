// attn_self_kernel and its ceiling probes; included by attn.hip.
#pragma once
#include "attn_common.hpp"

namespace pm {
// Single-segment attention (the spatial self-attention: 19 % of a 576x1024 forward's FLOPs), VALU diet.
//
// At head dim 64 a 32-query x 64-key tile is 16 MFMAs (512 matrix cycles) against 2048 scores of softmax, so
// the kernel lives or dies by the vector instructions per score.  attn_kernel spends ~6.5 (max, scale-and-
// subtract FMA, exp, sum, convert, rescale bookkeeping); this one ~3:
//   * Q arrives pre-multiplied by scale*log2(e) (the host folds it into the to_q weights; otherwise the
//     fragments are scaled once here), so scores are already in the base-2 domain: no per-score multiply;
//   * the running maximum is subtracted BY THE MFMA: the S^T chain's initial accumulator is a register block
//     holding -m (nm[]), so the chain ends in s - m and p = exp2(S') needs no subtraction either.  m is the
//     "stale" maximum: it is only raised when a tile's scores exceed it by more than STALE_THR (p stays
//     <= 2^STALE_THR: harmless for f32 accumulation and for the 16-bit P operand, whose relative precision
//     does not depend on magnitude), which after the first tiles almost never happens, so the O/l rescale
//     and the rewrite of nm[] leave the steady state: per score there remain 1/2 v_max3 (the check), v_exp,
//     v_add (row sum) and 1/2 v_cvt_pk;
//   * the first tile and a ragged last tile run a "careful" variant (exact maximum, key masking): none of
//     that is in the hot loop;
//   * 64 query rows per wave as two 32-row blocks whose chains are issued block after block
//     (S'(0) | max(0) | S'(1) || exp(0) | max(1) | PV(0) || exp(1) | PV(1)), so one block's VALU work sits
//     beside the other block's MFMAs inside one wave, on top of the overlap between the two waves of a SIMD.
constexpr float STALE_THR = 6.0f;
constexpr float STALE_SUM = 1024.0f;

// PROBE > 0 (diagnosis builds of the production configuration, reached through pm_debug_attn_variant 11 / 12 / 13;
// their OUTPUT IS NOT AN ATTENTION RESULT): the same per-tile instruction stream with parts taken away, to measure what
// this chip sustains for the mix at the clock it holds (profiles/r03/attention_ceiling.txt):
//   1  no global traffic in the steady state: the first two K/V tiles stay in LDS and are re-read for every tile
//      (same 16 MFMAs, same 2048-score softmax stream, same LDS fragment reads, same barriers);
//   2  as 1 without the softmax's vector instructions (P = the low halves of S', no max / exp / sum / convert);
//   3  as 2 without the LDS fragment reads (K and V fragments stay in registers): the bare MFMA stream.
template <typename T, int QB, bool PIPE, bool POST, int RING, int PROBE = 0>
__global__ __launch_bounds__(256, (QB == 1 && RING == 2) ? 3 : 2) void attn_self_kernel(const AttnParams p) {
  __shared__ __attribute__((aligned(16))) char smem[2 * RING * KV_TILE_BYTES];  // K[RING], V[RING]
  char* const Ks = smem;
  char* const Vs = smem + RING * KV_TILE_BYTES;

  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int ql = lane & 31, hh = lane >> 5;
  const AttnWork w = attn_work(xcd_workgroup(), p.nqt, p.heads);
  const int qt = w.qt, b = w.b, head = w.head;

  unsigned long long t_clk0 = 0, t_real0 = 0;  // (kept per kernel: profiles/attn_split/README.md)
  if constexpr (PM_DIAG_BUILD) {
    if (p.stamps) {
      t_clk0 = __builtin_amdgcn_s_memtime();
      t_real0 = __builtin_amdgcn_s_memrealtime();
    }
  }

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
  if (p.prescaled == 0) scale_q(qf, p.scale_log2e);  // (uniform)

  const int lr = tid >> 3;
  const int Nk = p.Nk[0];
  const char* const kbase = reinterpret_cast<const char*>(reinterpret_cast<const T*>(p.k[0]) + (int64_t)b * p.k_bs[0] + head * 64);
  const char* const vbase = reinterpret_cast<const char*>(reinterpret_cast<const T*>(p.v[0]) + (int64_t)b * p.k_bs[0] + head * 64);
  const uint32_t krs2 = (uint32_t)(p.k_rs[0] * 2);
  const int nkt = (Nk + KV_TILE - 1) / KV_TILE;
  const int kc = (tid & 7) ^ ((lr >> 1) & 7);           // source-side swizzles: see attn_kernel (attn_cross.hpp)
  const int vc = (tid & 7) ^ (((lr >> 1) & 1) << 2);
  const int last_full = (Nk % KV_TILE == 0) ? nkt : nkt - 1;  // tiles [0, last_full) lie wholly inside the sequence
  // Those tiles are fetched with `buffer_load ... lds`: per-lane offset fixed for the whole kernel, the tile's position in
  // the SCALAR offset, the LDS stage in M0 - no vector instruction for addresses in the K loop (the global_load_lds form
  // recomputes clamped 64-bit per-lane addresses, ~20 VALU incl. two v_mul_lo_u32 per tile, on a loop bound by vector
  // issue).  (range = through the head slice of the last key row; no tile fetched this way reaches it)
  const uint32_t kv_range = (uint32_t)(Nk - 1) * krs2 + 128u;
  const __amdgpu_buffer_rsrc_t krsrc = __builtin_amdgcn_make_buffer_rsrc((void*)kbase, (short)0, (int)kv_range, 0x00020000);
  const __amdgpu_buffer_rsrc_t vrsrc = __builtin_amdgcn_make_buffer_rsrc((void*)vbase, (short)0, (int)kv_range, 0x00020000);
  const uint32_t kvoff = (uint32_t)lr * krs2 + (uint32_t)kc * 16, vvoff = (uint32_t)lr * krs2 + (uint32_t)vc * 16;
  auto load_kv = [&](int kt, int buf) {  // (both fetch forms kept per kernel: profiles/attn_split/README.md)
    if (kt < last_full) {
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        const uint32_t soff = (uint32_t)(kt * KV_TILE + 32 * j) * krs2;
        const int dst = buf * KV_TILE_BYTES + (32 * j + 8 * wave) * 128;
        __builtin_amdgcn_raw_ptr_buffer_load_lds(krsrc, (lds_void*)(Ks + dst), 16, kvoff, soff, 0, 0);
        __builtin_amdgcn_raw_ptr_buffer_load_lds(vrsrc, (lds_void*)(Vs + dst), 16, vvoff, soff, 0, 0);
      }
      return;
    }
#pragma unroll
    for (int j = 0; j < 2; ++j) {  // ragged last tile: rows clamped to the last key (masked by the careful tile)
      int key = kt * KV_TILE + lr + 32 * j;
      if (key > Nk - 1) key = Nk - 1;
      const int dst = buf * KV_TILE_BYTES + (32 * j + 8 * wave) * 128;
      const uint32_t row = (uint32_t)key * krs2;
      __builtin_amdgcn_global_load_lds((glb_void*)(kbase + (row + (uint32_t)kc * 16)), (lds_void*)(Ks + dst), 16, 0, 0);
      __builtin_amdgcn_global_load_lds((glb_void*)(vbase + (row + (uint32_t)vc * 16)), (lds_void*)(Vs + dst), 16, 0, 0);
    }
  };

  f32x16 oacc[QB][2], nm[QB];  // nm: every register = -m_run, the initial accumulator of the S^T chains
  float m_run[QB], l_run[QB];
#pragma unroll
  for (int qb = 0; qb < QB; ++qb) {
    m_run[qb] = 0.f;
    l_run[qb] = 0.f;
#pragma unroll
    for (int r = 0; r < 16; ++r) nm[qb][r] = 0.f;
    asm volatile("" : "+v"(nm[qb]));
#pragma unroll
    for (int d = 0; d < 2; ++d)
#pragma unroll
      for (int r = 0; r < 16; ++r) oacc[qb][d][r] = 0.f;
  }

  // transposed-read lane coordinates of the V^T fragments (see attn_kernel)
  const int trow = (lane & 15) >> 2;
  const int tcol8 = ((lane >> 4) & 1) * 2 + ((lane & 3) >> 1);
  const int tsub = (lane & 1) * 8;

  // raise the stale maximum of block qb by the row maximum of the pending tile (mx: this lane's half)
  auto raise = [&](int qb, f32x16 (&sacc)[2], float mx, bool first) {  // (kept per kernel: profiles/attn_split/README.md)
    float rmx = fmaxf(mx, other_half(mx));
    if (!first) {
      rmx = fmaxf(rmx, 0.f);  // never lower m: rows that did not outgrow it keep alpha == 1 exactly
      const float alpha = __builtin_amdgcn_exp2f(-rmx);
      l_run[qb] *= alpha;
#pragma unroll
      for (int d = 0; d < 2; ++d)
#pragma unroll
        for (int r = 0; r < 16; ++r) oacc[qb][d][r] *= alpha;
    }
    m_run[qb] += rmx;
#pragma unroll
    for (int r = 0; r < 16; ++r) nm[qb][r] = -m_run[qb];
    // opaque to the optimiser: knowing the 16 registers equal, hipcc re-broadcasts them from one scalar in
    // every tile (15 v_mov per block and tile - the very instructions this block exists to save)
    asm volatile("" : "+v"(nm[qb]));
#pragma unroll
    for (int kb = 0; kb < 2; ++kb)
#pragma unroll
      for (int r = 0; r < 16; ++r) sacc[kb][r] -= rmx;
  };

  // one K/V tile.  CAREFUL: exact maximum + key masking (first tile, ragged last tile).
  auto tile = [&](int kt, auto bufc, auto careful_c) {
    constexpr bool CAREFUL = decltype(careful_c)::value;
    const int buf = bufc;  // (an integral_constant in the fast loop: LDS offsets fold into the reads' immediates)
    const char* ks = Ks + buf * KV_TILE_BYTES;
    const char* vs = Vs + buf * KV_TILE_BYTES;
    Pack8<T> pf[QB][4];
    auto pv = [&](int qb) {  // O^T += V^T . P^T
#pragma unroll
      for (int s4 = 0; s4 < 4; ++s4) {
#pragma unroll
        for (int db = 0; db < 2; ++db) {
          const int r0 = 16 * s4 + 4 * hh + trow;
          const int r1 = r0 + 8;
          const int ch = db * 4 + tcol8;
          const int off0 = r0 * 128 + ((ch ^ (((r0 >> 1) & 1) << 2)) << 4) + tsub;
          const int off1 = r1 * 128 + ((ch ^ (((r1 >> 1) & 1) << 2)) << 4) + tsub;
          typename Vec<T>::v8 vf;
          if constexpr (PROBE >= 3) {
            vf = qf[qb][(s4 + db) & 3].v;  // (any resident register operand)
          } else {
            vf = tr_pair<T>(vs, off0, off1);
          }
          oacc[qb][db] = mfma32(vf, pf[qb][s4].v, oacc[qb][db]);
        }
      }
    };
#pragma unroll
    for (int qb = 0; qb < QB; ++qb) {
      // ---- S'^T = K . Q'^T - m : the chain starts from nm (K fragments are re-read per block: LDS reads are
      // cheap here, registers are not) ----
      f32x16 sacc[2];
#pragma unroll
      for (int kb = 0; kb < 2; ++kb) {
        const int row = kb * 32 + ql;
        Pack8<T> kf[4];
#pragma unroll
        for (int s = 0; s < 4; ++s) {
          const int chunk = 2 * s + hh;
          if constexpr (PROBE >= 3) {
            kf[s].u = qf[qb][(s + kb) & 3].u;
          } else {
            kf[s].u = *reinterpret_cast<const u32x4*>(ks + row * 128 + ((chunk ^ ((row >> 1) & 7)) << 4));
          }
        }
        sacc[kb] = mfma32(kf[0].v, qf[qb][0].v, nm[qb]);
#pragma unroll
        for (int s = 1; s < 4; ++s) sacc[kb] = mfma32(kf[s].v, qf[qb][s].v, sacc[kb]);
      }
      if constexpr (PIPE) {
        if (qb > 0) pv(qb - 1);  // the previous block's P.V sits between this block's S' chain and its softmax
      }
      if constexpr (CAREFUL) {
        if (kt * KV_TILE + KV_TILE > Nk) {  // (kept per kernel: profiles/attn_split/README.md)
#pragma unroll
          for (int kb = 0; kb < 2; ++kb)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
              const int key = kt * KV_TILE + kb * 32 + (r & 3) + 8 * (r >> 2) + 4 * hh;
              if (key >= Nk) sacc[kb][r] = -INFINITY;
            }
        }
      }
      // this lane's maximum over its 32 scores of the tile
      auto lane_max = [&]() -> float {
        float m0 = fmaxf(sacc[0][0], sacc[1][0]);
#pragma unroll
        for (int r = 1; r < 16; ++r) m0 = fmaxf(fmaxf(m0, sacc[0][r]), sacc[1][r]);
        return m0;
      };
      // p = 2^S', 16-bit P operand; returns this lane's sum of p
      auto softmax = [&]() -> float {
        float ps[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int kb = 0; kb < 2; ++kb)
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            const float pe = __builtin_amdgcn_exp2f(sacc[kb][r]);
            ps[r & 3] += pe;
            pf[qb][kb * 2 + (r >> 3)].e[r & 7] = from_f32<T>(pe);
          }
        return (ps[0] + ps[1]) + (ps[2] + ps[3]);
      };
      float psum;
      if constexpr (PROBE >= 2 && !CAREFUL) {
        // no softmax: the P operand is made of the S' registers as they stand (keeps the S' -> P.V dependence)
#pragma unroll
        for (int kb = 0; kb < 2; ++kb)
#pragma unroll
          for (int h2 = 0; h2 < 2; ++h2) {
            union { float f[4]; u32x4 u; } t;
#pragma unroll
            for (int e = 0; e < 4; ++e) t.f[e] = sacc[kb][8 * h2 + e];
            pf[qb][kb * 2 + h2].u = t.u;
          }
        psum = sacc[1][15];
      } else if constexpr (CAREFUL) {
        raise(qb, sacc, lane_max(), kt == 0);
        psum = softmax();
      } else if constexpr (POST) {
        // no maximum at all in the steady state: exponentiate against the stale m and look at the row sum that
        // is formed anyway - a score more than 10 above m (or an overflow: inf) shows as a lane sum > 2^10;
        // only then the exact maximum is taken, m raised and the tile's P redone (nothing of it has been
        // accumulated yet).  Below that bound every p <= 2^10: safe for f32 sums and the 16-bit operand.
        psum = softmax();
        if (__builtin_amdgcn_ballot_w64(!(psum <= STALE_SUM)) != 0) {
          raise(qb, sacc, lane_max(), false);
          psum = softmax();
        }
      } else {
        const float m0 = lane_max();
        if (__builtin_amdgcn_ballot_w64(m0 > STALE_THR) != 0) raise(qb, sacc, m0, false);
        psum = softmax();
      }
      l_run[qb] += psum;
      if constexpr (!PIPE) {
        pv(qb);
        __builtin_amdgcn_sched_barrier(0);  // keep the blocks apart: interleaved, their live ranges spill
      }
    }
    if constexpr (PIPE) pv(QB - 1);
  };

  // K/V ring: RING stages of 64 keys, the DMAs of the next RING-1 tiles in flight ACROSS the per-tile barrier
  // (counted s_waitcnt vmcnt + raw s_barrier; a __syncthreads() would drain them: with one tile of look-ahead
  // every tile paid the L2 / Infinity-Cache round trip, MFMA pipes 46 % busy at 2.0 GHz with the VALU diet).
  // Tile t lives in stage t % RING.  arrive(t): this wave's share of tile t has landed (each tile is 4 DMAs
  // per wave, younger tiles may stay in flight), then the barrier publishes everybody's share and proves that
  // every wave is done with tile t-1, whose stage the load issued right behind it (tile t+RING-1) overwrites.
  auto arrive = [&](int t) {
    if constexpr (RING == 2) {  // classic double buffer: 32 KiB of LDS, three workgroups per CU at 32 rows per wave
      __syncthreads();          // (drains this wave's DMAs, publishes tile t, frees tile t-1's stage)
      if (t + 1 < nkt && (PROBE == 0 || t == 0)) load_kv(t + 1, (t + 1) & 1);
    } else {
      const int ahead = (nkt - 1 - t < RING - 2) ? nkt - 1 - t : RING - 2;  // younger tiles already issued
      if (ahead >= 2)
        asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
      else if (ahead == 1)
        asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
      else
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      __builtin_amdgcn_s_barrier();
      if (t + RING - 1 < nkt) load_kv(t + RING - 1, (t + RING - 1) % RING);
    }
  };
  static_assert(RING == 4 || RING == 2, "the vmcnt ladder above is written for 3 tiles of look-ahead");
#pragma unroll
  for (int t = 0; t < RING - 1; ++t)
    if (t < nkt) load_kv(t, t);
  // three separate loops (careful first tile | fast tiles | careful ragged tile): with the two variants as the
  // arms of one loop body hipcc copied the 16-register accumulator tuples at every merge (~50 v_mov per tile)
  arrive(0);  // (tiles [1, last_full) need no masking; the walk is kept per kernel: profiles/attn_split/README.md)
  tile(0, std::integral_constant<int, 0>{}, std::true_type{});
  int kt = 1;
  for (; kt + 3 < last_full; kt += 4) {  // four tiles per trip: every tile's stage is a compile-time constant
    arrive(kt);
    tile(kt, std::integral_constant<int, 1>{}, std::false_type{});
    arrive(kt + 1);
    tile(kt + 1, std::integral_constant<int, 2 % RING>{}, std::false_type{});
    arrive(kt + 2);
    tile(kt + 2, std::integral_constant<int, 3 % RING>{}, std::false_type{});
    arrive(kt + 3);
    tile(kt + 3, std::integral_constant<int, 0 % RING>{}, std::false_type{});
  }
  for (; kt < last_full; ++kt) {
    arrive(kt);
    tile(kt, kt % RING, std::false_type{});
  }
  if (nkt > 1 && last_full < nkt) {
    arrive(nkt - 1);
    tile(nkt - 1, (nkt - 1) % RING, std::true_type{});
  }

#pragma unroll
  for (int qb = 0; qb < QB; ++qb) {
    const float l_tot = l_run[qb] + other_half(l_run[qb]);
    const float inv = 1.0f / l_tot;
    if (q_valid[qb]) {
      T* op = reinterpret_cast<T*>(p.o) + (int64_t)b * p.o_bs + (int64_t)qrow[qb] * p.o_rs + head * 64;
      store_row32(op, oacc[qb], inv, hh);
    }
  }
  if constexpr (PM_DIAG_BUILD) {
    if (p.stamps && tid == 0) {  // in-kernel clock = d(s_memtime) / d(s_memrealtime) x 100 MHz (diagnostics build only)
      unsigned long long* st = p.stamps + 2 * (size_t)blockIdx.x;
      st[0] = __builtin_amdgcn_s_memtime() - t_clk0;
      st[1] = __builtin_amdgcn_s_memrealtime() - t_real0;
    }
  }
}

}  // namespace pm
