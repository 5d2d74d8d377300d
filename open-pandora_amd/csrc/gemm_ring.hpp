// The two wave-specialised ring kernels of the GEMM family (128x128 and 256x128 tiles); included by gemm.hip.
#pragma once
#include "gemm_common.hpp"

namespace pm {

// In-kernel cycle stamps of one wave for tools/ring_prof.py: clock64 marks, three running sums of the intervals between them
// and a K-step count, written to prof[block][8 waves][4] (loader waves: vmcnt wait | barrier | issue | steps; consumer waves:
// barrier | compute | epilogue | steps).  In every other build the members are empty and the loops carry no code for them.
struct RingStamps {
#ifdef PM_RING_PROF
  long long s[4], t[4] = {0, 0, 0, 0};
  __device__ __forceinline__ void mark(int i) { s[i] = clock64(); }
  template <int... SLOT> __device__ __forceinline__ void laps() {  // the interval mark(i) .. mark(i + 1) goes to sum SLOT[i]
    int i = 0;
    ((t[SLOT] += s[i + 1] - s[i], ++i), ...);
  }
  __device__ __forceinline__ void step() { ++t[3]; }
  __device__ __forceinline__ void flush(const GemmParams& p, int wave, int lane) const {
    if (p.prof && lane == 0) {
      long long* d = p.prof + ((long long)blockIdx.x * 8 + wave) * 4;
      d[0] = t[0]; d[1] = t[1]; d[2] = t[2]; d[3] = t[3];
    }
  }
#else
  __device__ __forceinline__ void mark(int) {}
  template <int... SLOT> __device__ __forceinline__ void laps() {}
  __device__ __forceinline__ void step() {}
  __device__ __forceinline__ void flush(const GemmParams&, int, int) const {}
#endif
};

// ---------------------------------------------------------------------------------------------
// Ring-pipelined, wave-specialised persistent variant (16-bit operands, whole K-tiles: dense, fast 3x3
// and temporal modes).
//
// The 2-stage kernel above issues its DMAs from the waves that also issue the MFMAs: a wave's
// instructions issue in order, so whenever the CU's load path is backed up the MFMAs wait behind the
// stalled global_load_lds, and with one workgroup per CU (every grid of <= 256 tiles: the M = 2560 / 640
// levels) a K-step costs a full round trip (~1.3 us measured: 25 GB/s per CU against the ~68 GB/s a CU
// can ingest).  Here one 8-wave workgroup owns the CU:
//   * waves 4-7 only load: 4 LDS stages of 32 KiB form a ring with the DMA of three K-tiles (96 KiB) in
//     flight across the barrier (counted s_waitcnt vmcnt, never 0 in steady state);
//   * waves 0-3 only compute (ds_read_b128 + MFMA, 64x64 per wave) and run the epilogue;
//   * one raw s_barrier per K-step hands stage k to the consumers and stage k-1 back to the loaders;
//   * the workgroup is persistent: it walks its share of the (tile, split) list and the loader cursor
//     runs three K-steps ahead ACROSS tile boundaries, so the next tile streams in during the epilogue;
//   * the epilogue is wave-private and LDS-free (epilogue_regs): each consumer wave stores its own 64x64
//     quadrant straight from the accumulators while the loaders keep streaming.
// LDS: the 128 KiB ring only (the epilogue works from registers: epilogue_regs).
constexpr int RING_STAGES = 4;
constexpr int RING_LDS = RING_STAGES * 2 * TILE_BYTES;

template <typename T, int AMODE>
__global__ __launch_bounds__(512, 1) void gemm_ring_kernel(const GemmParams p) {
  static_assert(AMODE != A_CONV3X3, "K tails / nearest-x2 stay on gemm_kernel");
  constexpr int STAGE_BYTES = 2 * TILE_BYTES;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  char* const As = smem;
  char* const Bs = smem + TILE_BYTES;

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const int G = gridDim.x;
  const int nwork = p.mtiles * p.ntiles * p.splits;
  PM_WORK_WALK(blockIdx.x, G, nwork);  // work_id(round): the family's work walk (gemm_common.hpp)
  const int nk_all = p.K / BK;

  auto decode = [&](int w, int& mt, int& nt, int& split) { decode_work<AMODE, BM>(p, w, mt, nt, split); };  // (gemm_common.hpp)

  if (wave >= 4) {
    // ================= loader waves (see gemm_kernel for the source-side swizzle / scalarised K walk) =====
    const int lw = __builtin_amdgcn_readfirstlane(wave - 4);  // (scalar: the DMA's LDS base goes to M0 by SALU)
    const int r8 = lane >> 3;             // row inside an 8-row DMA piece; tile row = 32*j + 8*lw + r8
    const int lc = (lane & 7) ^ r8;       // logical 16-byte k-chunk this lane fetches ((row & 7) == r8)
    const char* const Ab = reinterpret_cast<const char*>(p.A);
    const char* const Wb = reinterpret_cast<const char*>(p.Wt);
    const char* const zero = reinterpret_cast<const char*>(p.zero);
    uint32_t b_off[4], a_off[4];
    int a_y[4], a_x[4];
    uint32_t inv[4] = {0u, 0u, 0u, 0u};  // conv modes: per row, the taps that are zero padding
    int tap_s = 0, ch_s = 0;
    int64_t nxt_a = 0, nxt_w = 0;  // fast conv: table entries of the K-step about to be issued
    int l_round = 0, l_kt = 0, l_kt1 = 0;
    auto loader_begin = [&]() -> bool {
      const int w = work_id(l_round);
      if (w < 0) return false;
      int mt, nt, split;
      decode(w, mt, nt, split);
      const int m0 = mt * BM, n0 = nt * BN;
      l_kt = split * p.ktps;
      l_kt1 = (l_kt + p.ktps < nk_all) ? l_kt + p.ktps : nk_all;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int pr = 32 * j + 8 * lw + r8;  // LDS row of the W tile -> output column (see epilogue_regs)
        int n = n0 + cperm(pr, p.act == PM_ACT_GEGLU || p.natural);
        if (n > p.N - 1) n = p.N - 1;
        b_off[j] = (uint32_t)(((int64_t)n * p.ldw + lc * 8) * 2);
        int m = m0 + 32 * j + 8 * lw + r8;
        if (m > p.M - 1) m = p.M - 1;
        if (AMODE == A_DENSE) {
          a_off[j] = (uint32_t)(((int64_t)m * p.lda + lc * 8) * 2);
          a_y[j] = a_x[j] = 0;
        } else if (AMODE == A_CONV3X3_FAST) {
          const int hw = p.Ho * p.Wo;
          const int f = m / hw;
          const int rem = m - f * hw;
          const int oy = rem / p.Wo, ox = rem - oy * p.Wo;
          a_y[j] = oy * p.stride + 1 - p.pad;
          a_x[j] = ox * p.stride + 1 - p.pad;
          a_off[j] = (uint32_t)((((int64_t)f * p.Hin + a_y[j]) * p.Win + a_x[j]) * p.lda * 2 + lc * 16);
          uint32_t bad = 0;  // bit t: tap t of this row is zero padding
#pragma unroll
          for (int t = 0; t < 9; ++t) {
            const int ty = t / 3, tx = t - ty * 3;
            const bool ok = (unsigned)(a_y[j] + ty - 1) < (unsigned)p.Hv && (unsigned)(a_x[j] + tx - 1) < (unsigned)p.Wv;
            bad |= ok ? 0u : (1u << t);
          }
          inv[j] = bad;
        } else {
          const int f = m / p.P;
          const int pix = m - f * p.P;
          a_off[j] = (uint32_t)((((int64_t)f * p.P + pix) * p.lda + lc * 8) * 2);
          const int fc = f % p.Fc;  // frame inside its clip (Fc == F unless clips are batched along the rows)
          a_y[j] = fc;
          a_x[j] = (int)(uint32_t)(((int64_t)pix * p.lda + lc * 8) * 2);  // byte offset inside a halo frame
          inv[j] = (fc == 0 ? 1u : 0u) | (fc == p.Fc - 1 ? 4u : 0u);  // taps reaching frame -1 / frame Fc of the clip
        }
      }
      if (AMODE == A_CONV3X3_FAST) {  // channel-chunk-major walk (see gemm_kernel's load_tile)
        const int chunk = l_kt / 9;
        tap_s = l_kt - chunk * 9;
        ch_s = chunk * BK;
        nxt_a = p.tap_a[tap_s];
        nxt_w = p.tap_w[tap_s];
      } else if (AMODE != A_DENSE) {  // temporal: chunk-major too (frames f-1, f, f+1 per 64-channel chunk), same table
        const int chunk = l_kt / 3;
        tap_s = l_kt - chunk * 3;
        ch_s = chunk * BK;
        nxt_a = p.tap_a[tap_s];
        nxt_w = p.tap_w[tap_s];
      }
      return true;
    };
    auto load_tile = [&](int kt, int buf) {
      const char* wb = Wb + (int64_t)((AMODE == A_DENSE && p.kwrap && kt * BK >= p.kwrap) ? kt * BK - p.kwrap : kt * BK) * 2;
      const char* ab = Ab;
      const char *hlo = nullptr, *hhi = nullptr;
      int dy = 0, dx = 0;
      if (AMODE == A_DENSE) {
        ab = Ab + (int64_t)kt * (BK * 2);
      } else if (AMODE == A_CONV3X3_FAST) {
        // per-tap A shift / W offset come from a host-filled table in the kernel arguments (scalar loads by a
        // uniform index, fetched one K-step ahead at the end of the previous call): the lone loader wave spent
        // ~150 cycles per K-step on the division by 3 and the 64-bit multiply chains that stood here
        wb = Wb + nxt_w + (int64_t)ch_s * 2;
        ab = Ab + nxt_a + (int64_t)ch_s * 2;
      } else {
        wb = Wb + nxt_w + (int64_t)ch_s * 2;
        ab = Ab + nxt_a + (int64_t)ch_s * 2;
        hlo = p.halo_lo ? reinterpret_cast<const char*>(p.halo_lo) + (int64_t)ch_s * 2 : nullptr;
        hhi = p.halo_hi ? reinterpret_cast<const char*>(p.halo_hi) + (int64_t)ch_s * 2 : nullptr;
      }
      // Conv modes without halo frames: the A tile goes through a buffer descriptor whose base carries the
      // (uniform) tap shift and channel offset; a lane's offset is its constant centre-tap offset, and a
      // padding lane gets offset ~0: out of range, for which `buffer_load ... lds` writes ZEROS into LDS
      // (tools/probes/buffer_lds_oob.hip).  2 VALU per DMA instead of the ~8 of a per-lane 64-bit pointer
      // select against a zero page (in-kernel stamps: loader issue 950 -> 560 cycles per K-step, which
      // had made the LOADER the bottleneck of the convs).
      const bool use_desc = (AMODE != A_DENSE) && p.halo_lo == nullptr && p.halo_hi == nullptr;
      if (use_desc) {
        const uint32_t nrec = (uint32_t)((Ab + p.a_bytes) - ab);
        __amdgpu_buffer_rsrc_t rsrc = __builtin_amdgcn_make_buffer_rsrc((void*)ab, (short)0, (int)nrec, 0x00020000);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const uint32_t voff = a_off[j] | (uint32_t)(-(int)((inv[j] >> tap_s) & 1u));
          const int dst = buf * STAGE_BYTES + (32 * j + 8 * lw) * 128;
          __builtin_amdgcn_raw_ptr_buffer_load_lds(rsrc, (lds_void*)(As + dst), 16, voff, 0, 0, 0);
          __builtin_amdgcn_global_load_lds((glb_void*)(wb + b_off[j]), (lds_void*)(Bs + dst), 16, 0, 0);
        }
      } else {
  #pragma unroll
        for (int j = 0; j < 4; ++j) {
          const char* src;
          if (AMODE == A_DENSE) {
            src = ab + a_off[j];
          } else if (AMODE == A_CONV3X3_FAST) {
            dy = tap_s / 3;
            dx = tap_s - dy * 3;
            const bool ok = (unsigned)(a_y[j] + dy - 1) < (unsigned)p.Hv && (unsigned)(a_x[j] + dx - 1) < (unsigned)p.Wv;
            src = ok ? ab + a_off[j] : zero;
          } else {
            // (per-row halo offsets are precomputed: the 64-bit multiplies that stood here made the loader the
            // bottleneck of the temporal conv: 1 250-1 450 issue cycles per K-step against 550 for dense)
            const int sf = a_y[j] + tap_s - 1;
            src = ab + a_off[j];
            if (sf < 0) src = hlo ? hlo + (uint32_t)a_x[j] : zero;
            if (sf >= p.Fc) src = hhi ? hhi + (uint32_t)a_x[j] : zero;
          }
          const int dst = buf * STAGE_BYTES + (32 * j + 8 * lw) * 128;
          __builtin_amdgcn_global_load_lds((glb_void*)src, (lds_void*)(As + dst), 16, 0, 0);
          __builtin_amdgcn_global_load_lds((glb_void*)(wb + b_off[j]), (lds_void*)(Bs + dst), 16, 0, 0);
        }
      }
      if (AMODE == A_CONV3X3_FAST) {
        if (++tap_s == 9) {
          tap_s = 0;
          ch_s += BK;
        }
        nxt_a = p.tap_a[tap_s];
        nxt_w = p.tap_w[tap_s];
      } else if (AMODE != A_DENSE) {
        if (++tap_s == 3) {
          tap_s = 0;
          ch_s += BK;
        }
        nxt_a = p.tap_a[tap_s];
        nxt_w = p.tap_w[tap_s];
      }
    };
    bool l_valid = loader_begin();
    int l_stage = 0, inflight = 0;
    auto issue = [&]() {
      if (!l_valid) return;
      load_tile(l_kt, l_stage);
      l_stage = (l_stage + 1) & (RING_STAGES - 1);
      ++inflight;
      if (++l_kt == l_kt1) {
        ++l_round;
        l_valid = loader_begin();
      }
    };
    issue();
    issue();
    issue();
    RingStamps st;  // -> vmcnt wait | barrier | issue
    // one iteration per K-step q of the consumers.  Barrier q publishes stages q AND q+1 (the consumers
    // pre-read the first fragments of step q+1 during step q), so everything but the youngest K-tile (8
    // DMAs per loader wave) must have landed; it also proves the consumers are done with stage q-1, which
    // the issue right behind it overwrites with step q+3.
    while (inflight > 0) {
      st.mark(0);
      if (inflight >= 3)
        asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
      else
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      st.mark(1);
      __builtin_amdgcn_s_barrier();
      st.mark(2);
      issue();
      --inflight;
      st.mark(3);
      st.laps<0, 1, 2>();
      st.step();
    }
    st.flush(p, wave, lane);
    return;
  }

  // ================= consumer waves =================
  const int wm = wave >> 1, wn = wave & 1;
  const int fr = lane & 15, fq = lane >> 4;
  const int a_frag = (wm * 64 + fr) * 128, b_frag = (wn * 64 + fr) * 128;
  const int slot0 = ((fq) ^ (fr & 7)) << 4, slot1 = ((4 + fq) ^ (fr & 7)) << 4;
  const bool partial = p.splits > 1;
  int c_stage = 0;
  RingStamps st;  // -> barrier | compute | epilogue

  // Fragment registers are double-buffered by k-substep: set 0 (k 0..31 of a stage) is read while the
  // MFMAs of the previous substep run - across the barrier for the first substep of the next stage - so
  // no MFMA ever waits for LDS latency (one consumer wave per SIMD: nobody else would hide it).
  Pack8<T> fa0[4], fb0[4], fa1[4], fb1[4];
  auto read_frags = [&](Pack8<T>* fa, Pack8<T>* fb, int stg, int slot) {
    const char* as = As + stg * STAGE_BYTES + a_frag + slot;
    const char* bs = Bs + stg * STAGE_BYTES + b_frag + slot;
#pragma unroll
    for (int i = 0; i < 4; ++i) fa[i].u = *reinterpret_cast<const u32x4*>(as + i * 2048);
#pragma unroll
    for (int j = 0; j < 4; ++j) fb[j].u = *reinterpret_cast<const u32x4*>(bs + j * 2048);
  };
  __builtin_amdgcn_s_barrier();  // barrier 0: stages 0 and 1 are in LDS
  read_frags(fa0, fb0, 0, slot0);

  for (int c_round = 0;; ++c_round) {
    const int w = work_id(c_round);
    if (w < 0) break;
    const bool last_tile = (work_id(c_round + 1) < 0);
    int mt, nt, split;
    decode(w, mt, nt, split);
    const int m0 = mt * BM, n0 = nt * BN;
    const int kt0 = split * p.ktps;
    const int kt1 = (kt0 + p.ktps < nk_all) ? kt0 + p.ktps : nk_all;
    float bv[4][4];  // requested now, needed in the epilogue
    load_bias_regs(p, bv, n0, wn, fq);

    f32x4 acc[4][4];
    const bool res_done = residual_into_acc<T>(p, acc, m0, n0, wm, wn, fr, fq);
    if (!res_done) {
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
    }

    for (int kt = kt0; kt < kt1; ++kt) {
      st.mark(0);
      const bool more = (kt + 1 < kt1) || !last_tile;  // does a next step exist (possibly the next tile's)?
      const int nstage = (c_stage + 1) & (RING_STAGES - 1);
      // Issue pattern pinned per substep: one ds_read_b128 behind each of the first 8 MFMAs (an MFMA holds
      // the SIMD's issue for 8 of its 16 cycles: the read rides in the gap), then 8 bare MFMAs that cover
      // the last read's latency.  Left alone, hipcc sinks each read group down to its first use (the MFMAs
      // then wait out the LDS latency); read groups issued en bloc between the MFMA groups cost ~100
      // issue cycles each (in-kernel stamps: 726 cycles per K-step against 512 of MFMA).
      __builtin_amdgcn_sched_barrier(0);
      read_frags(fa1, fb1, c_stage, slot1);
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = mfma16(fb0[j].v, fa0[i].v, acc[i][j]);
#pragma unroll
      for (int t = 0; t < 8; ++t) {
        __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);  // 1 MFMA
        __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);  // 1 DS read
      }
      __builtin_amdgcn_sched_group_barrier(0x008, 8, 0);
      __builtin_amdgcn_sched_barrier(0);
      // next step's first fragments: that stage was published by the previous step's barrier.  Read
      // unconditionally (after the very last step the values are simply unused): a branch here would make
      // hipcc merge the LDS wait counts of both paths and stall the MFMAs on these reads
      read_frags(fa0, fb0, nstage, slot0);
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = mfma16(fb1[j].v, fa1[i].v, acc[i][j]);
#pragma unroll
      for (int t = 0; t < 8; ++t) {
        __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
        __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
      }
      __builtin_amdgcn_sched_group_barrier(0x008, 8, 0);
      __builtin_amdgcn_sched_barrier(0);
      st.mark(1);
      // all reads of stage c_stage have returned (their MFMAs are issued): hand it back, get stage + 2
      if (more) __builtin_amdgcn_s_barrier();
      c_stage = nstage;
      st.mark(2);
      st.laps<1, 0>();
      st.step();
    }
    st.mark(0);

    // ---------------- epilogue of this wave's 64x64 quadrant (the loaders keep streaming the next tile) ----
    if (piece_dead(p, m0 + wm * 64, n0 + wn * 64)) {
    } else if (AMODE == A_DENSE && !res_done && epilogue_lean16_ok(p, m0 + wm * 64, n0 + wn * 64))
      epilogue_lean16<T>(p, acc, bv, m0 + wm * 64, n0 + wn * 64, fr, fq);  // (r06: see gemm_kernel)
    else if (epilogue_lean32_ok(p, m0 + wm * 64, n0 + wn * 64, res_done))
      epilogue_lean32<T>(p, acc, bv, m0 + wm * 64, n0 + wn * 64, fr, fq, mt * 2 + wm, split);
    else
      epilogue_regs<T>(p, acc, bv, m0, n0, wm, wn, fr, fq, mt * 2 + wm, split, res_done);
    st.mark(1);
    st.laps<2>();
  }
  st.flush(p, wave, lane);
}

// Entry `i` (wave-uniform, 0..8) of a per-tap table in the kernel arguments, by a select chain over constant offsets: indexed
// dynamically, hipcc demoted the WHOLE by-value GemmParams of gemm_ringw_kernel's 3x3 instantiation to scratch memory (every
// p.field became a scratch load - 1403 of them, the loader's DMA issue path included: 3-4x slower than the 128x128 ring).
__device__ __forceinline__ int64_t tap_entry(const int64_t (&t)[9], int i) {
  int64_t r = t[0];
#pragma unroll
  for (int k = 1; k < 9; ++k) r = (i == k) ? t[k] : r;
  return r;
}

// gemm_ringw: the ring kernel on a 256(M) x 128(N) tile (PANDORA_GEMM_RINGW).  Why: in-kernel stamps of the ring kernel on long
// K loops (tools/ring_prof.py, 8192^3): the four loader waves spend 645 clocks per K-step ISSUING its 32 DMAs and the consumers
// wait for them (563 clocks of compute, 207 at the barrier) - and eight loader waves change nothing
// (profiles/r03/negative_result_ring8_*): the CU's vector-memory path takes ~50 B/clk, a 128x128x64 K-step needs 64 B per
// MFMA clock.  A 256x128 tile needs 48: four consumer waves of 128x64 (two 64-row accumulator halves, 64 MFMAs and 24
// ds_read_b128 per K-step), the same four loaders (8 + 4 pieces each), three 48-KiB stages; barrier q publishes stage q.
template <typename T, int AMODE>
__global__ __launch_bounds__(512, 1) void gemm_ringw_kernel(const GemmParams p) {
  static_assert(AMODE != A_CONV3X3, "K tails / nearest-x2 stay on gemm_kernel");
  constexpr int BMW = 256;                        // tile rows
  constexpr int STAGE_BYTES = 3 * TILE_BYTES;     // A tile 256 x 64 (32 KiB) | W tile 128 x 64 (16 KiB)
  constexpr int NSTAGE = 3;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  char* const As = smem;
  char* const Bs = smem + 2 * TILE_BYTES;

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int G = gridDim.x;
  const int nwork = p.mtiles * p.ntiles * p.splits;
  // (the loader waves below - loader_begin, load_tile, issue - are still one copy per ring kernel: sharing them has not been
  // tried against the adoption rule of profiles/gemm_walk/README.md yet)
  PM_WORK_WALK(blockIdx.x, G, nwork);  // work_id(round): the family's work walk (gemm_common.hpp)
  const int nk_all = p.K / BK;

  auto decode = [&](int w, int& mt, int& nt, int& split) { decode_work<AMODE, BMW>(p, w, mt, nt, split); };  // (gemm_common.hpp)

  if (wave >= 4) {
    // ================= loader waves (see gemm_kernel for the source-side swizzle / scalarised K walk) =====
    const int lw = __builtin_amdgcn_readfirstlane(wave - 4);  // (scalar: the DMA's LDS base goes to M0 by SALU)
    const int r8 = lane >> 3;             // row inside an 8-row DMA piece; tile row = 32*j + 8*lw + r8
    const int lc = (lane & 7) ^ r8;       // logical 16-byte k-chunk this lane fetches ((row & 7) == r8)
    const char* const Ab = reinterpret_cast<const char*>(p.A);
    const char* const Wb = reinterpret_cast<const char*>(p.Wt);
    const char* const zero = reinterpret_cast<const char*>(p.zero);
    uint32_t b_off[4], a_off[8];
    int a_y[8], a_x[8];
    uint32_t inv[8] = {0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u};  // conv modes: per row, the taps that are zero padding
    int tap_s = 0, ch_s = 0;
    int64_t nxt_a = 0, nxt_w = 0;  // fast conv: table entries of the K-step about to be issued
    int l_round = 0, l_kt = 0, l_kt1 = 0;
    // (always_inline: left to the inliner, the 3x3 instantiation kept loader_begin - 8 rows x 9 taps - as a real function:
    // its by-reference captures, the kernel's GemmParams among them, then live in scratch memory)
    auto loader_begin = [&]() __attribute__((always_inline)) -> bool {
      const int w = work_id(l_round);
      if (w < 0) return false;
      int mt, nt, split;
      decode(w, mt, nt, split);
      const int m0 = mt * BMW, n0 = nt * BN;
      l_kt = split * p.ktps;
      l_kt1 = (l_kt + p.ktps < nk_all) ? l_kt + p.ktps : nk_all;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int pr = 32 * j + 8 * lw + r8;  // LDS row of the W tile -> output column (see epilogue_regs)
        int n = n0 + cperm(pr, p.act == PM_ACT_GEGLU || p.natural);
        if (n > p.N - 1) n = p.N - 1;
        b_off[j] = (uint32_t)(((int64_t)n * p.ldw + lc * 8) * 2);
      }
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        int m = m0 + 32 * j + 8 * lw + r8;
        if (m > p.M - 1) m = p.M - 1;
        if (AMODE == A_DENSE) {
          a_off[j] = (uint32_t)(((int64_t)m * p.lda + lc * 8) * 2);
          a_y[j] = a_x[j] = 0;
        } else if (AMODE == A_CONV3X3_FAST) {
          const int hw = p.Ho * p.Wo;
          const int f = m / hw;
          const int rem = m - f * hw;
          const int oy = rem / p.Wo, ox = rem - oy * p.Wo;
          a_y[j] = oy * p.stride + 1 - p.pad;
          a_x[j] = ox * p.stride + 1 - p.pad;
          a_off[j] = (uint32_t)((((int64_t)f * p.Hin + a_y[j]) * p.Win + a_x[j]) * p.lda * 2 + lc * 16);
          uint32_t bad = 0;  // bit t: tap t of this row is zero padding
#pragma unroll
          for (int t = 0; t < 9; ++t) {
            const int ty = t / 3, tx = t - ty * 3;
            const bool ok = (unsigned)(a_y[j] + ty - 1) < (unsigned)p.Hv && (unsigned)(a_x[j] + tx - 1) < (unsigned)p.Wv;
            bad |= ok ? 0u : (1u << t);
          }
          inv[j] = bad;
        } else {
          const int f = m / p.P;
          const int pix = m - f * p.P;
          a_off[j] = (uint32_t)((((int64_t)f * p.P + pix) * p.lda + lc * 8) * 2);
          const int fc = f % p.Fc;  // frame inside its clip (Fc == F unless clips are batched along the rows)
          a_y[j] = fc;
          a_x[j] = (int)(uint32_t)(((int64_t)pix * p.lda + lc * 8) * 2);  // byte offset inside a halo frame
          inv[j] = (fc == 0 ? 1u : 0u) | (fc == p.Fc - 1 ? 4u : 0u);  // taps reaching frame -1 / frame Fc of the clip
        }
      }
      if (AMODE == A_CONV3X3_FAST) {  // channel-chunk-major walk (see gemm_kernel's load_tile)
        const int chunk = l_kt / 9;
        tap_s = l_kt - chunk * 9;
        ch_s = chunk * BK;
        nxt_a = tap_entry(p.tap_a, tap_s);
        nxt_w = tap_entry(p.tap_w, tap_s);
      } else if (AMODE != A_DENSE) {  // temporal: chunk-major too (frames f-1, f, f+1 per 64-channel chunk), same table
        const int chunk = l_kt / 3;
        tap_s = l_kt - chunk * 3;
        ch_s = chunk * BK;
        nxt_a = tap_entry(p.tap_a, tap_s);
        nxt_w = tap_entry(p.tap_w, tap_s);
      }
      return true;
    };
    auto load_tile = [&](int kt, int buf) __attribute__((always_inline)) {
      const char* wb = Wb + (int64_t)((AMODE == A_DENSE && p.kwrap && kt * BK >= p.kwrap) ? kt * BK - p.kwrap : kt * BK) * 2;
      const char* ab = Ab;
      const char *hlo = nullptr, *hhi = nullptr;
      int dy = 0, dx = 0;
      if (AMODE == A_DENSE) {
        ab = Ab + (int64_t)kt * (BK * 2);
      } else if (AMODE == A_CONV3X3_FAST) {
        // per-tap A shift / W offset come from a host-filled table in the kernel arguments (scalar loads by a
        // uniform index, fetched one K-step ahead at the end of the previous call): the lone loader wave spent
        // ~150 cycles per K-step on the division by 3 and the 64-bit multiply chains that stood here
        wb = Wb + nxt_w + (int64_t)ch_s * 2;
        ab = Ab + nxt_a + (int64_t)ch_s * 2;
      } else {
        wb = Wb + nxt_w + (int64_t)ch_s * 2;
        ab = Ab + nxt_a + (int64_t)ch_s * 2;
        hlo = p.halo_lo ? reinterpret_cast<const char*>(p.halo_lo) + (int64_t)ch_s * 2 : nullptr;
        hhi = p.halo_hi ? reinterpret_cast<const char*>(p.halo_hi) + (int64_t)ch_s * 2 : nullptr;
      }
      // Conv modes without halo frames: the A tile goes through a buffer descriptor whose base carries the
      // (uniform) tap shift and channel offset; a lane's offset is its constant centre-tap offset, and a
      // padding lane gets offset ~0: out of range, for which `buffer_load ... lds` writes ZEROS into LDS
      // (tools/probes/buffer_lds_oob.hip).  2 VALU per DMA instead of the ~8 of a per-lane 64-bit pointer
      // select against a zero page (in-kernel stamps: loader issue 950 -> 560 cycles per K-step, which
      // had made the LOADER the bottleneck of the convs).
      const bool use_desc = (AMODE != A_DENSE) && p.halo_lo == nullptr && p.halo_hi == nullptr;
      if (use_desc) {
        const uint32_t nrec = (uint32_t)((Ab + p.a_bytes) - ab);
        __amdgpu_buffer_rsrc_t rsrc = __builtin_amdgcn_make_buffer_rsrc((void*)ab, (short)0, (int)nrec, 0x00020000);
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const uint32_t voff = a_off[j] | (uint32_t)(-(int)((inv[j] >> tap_s) & 1u));
          const int dst = buf * STAGE_BYTES + (32 * j + 8 * lw) * 128;
          __builtin_amdgcn_raw_ptr_buffer_load_lds(rsrc, (lds_void*)(As + dst), 16, voff, 0, 0, 0);
          if (j < 4) __builtin_amdgcn_global_load_lds((glb_void*)(wb + b_off[j]), (lds_void*)(Bs + dst), 16, 0, 0);
        }
      } else {
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const char* src;
          if (AMODE == A_DENSE) {
            src = ab + a_off[j];
          } else if (AMODE == A_CONV3X3_FAST) {
            dy = tap_s / 3;
            dx = tap_s - dy * 3;
            const bool ok = (unsigned)(a_y[j] + dy - 1) < (unsigned)p.Hv && (unsigned)(a_x[j] + dx - 1) < (unsigned)p.Wv;
            src = ok ? ab + a_off[j] : zero;
          } else {
            const int sf = a_y[j] + tap_s - 1;
            src = ab + a_off[j];
            if (sf < 0) src = hlo ? hlo + (uint32_t)a_x[j] : zero;
            if (sf >= p.Fc) src = hhi ? hhi + (uint32_t)a_x[j] : zero;
          }
          const int dst = buf * STAGE_BYTES + (32 * j + 8 * lw) * 128;
          __builtin_amdgcn_global_load_lds((glb_void*)src, (lds_void*)(As + dst), 16, 0, 0);
          if (j < 4) __builtin_amdgcn_global_load_lds((glb_void*)(wb + b_off[j]), (lds_void*)(Bs + dst), 16, 0, 0);
        }
      }
      if (AMODE == A_CONV3X3_FAST) {
        if (++tap_s == 9) {
          tap_s = 0;
          ch_s += BK;
        }
        nxt_a = tap_entry(p.tap_a, tap_s);
        nxt_w = tap_entry(p.tap_w, tap_s);
      } else if (AMODE != A_DENSE) {
        if (++tap_s == 3) {
          tap_s = 0;
          ch_s += BK;
        }
        nxt_a = tap_entry(p.tap_a, tap_s);
        nxt_w = tap_entry(p.tap_w, tap_s);
      }
    };
    bool l_valid = loader_begin();
    int l_stage = 0, inflight = 0;
    auto issue = [&]() __attribute__((always_inline)) {
      if (!l_valid) return;
      load_tile(l_kt, l_stage);
      l_stage = (l_stage + 1 == NSTAGE) ? 0 : l_stage + 1;
      ++inflight;
      if (++l_kt == l_kt1) {
        ++l_round;
        l_valid = loader_begin();
      }
    };
    issue();
    issue();
    RingStamps st;  // -> vmcnt wait | barrier | issue
    // one iteration per K-step q of the consumers.  Barrier q publishes stage q (no pre-read across the barrier here: with
    // three 48-KiB stages the stage after next is the one the consumers have just left), so everything but the youngest
    // K-tile (12 DMAs per loader wave) must have landed; it also proves the consumers are done with stage q-1, which the
    // issue right behind it overwrites with step q+2.
    while (inflight > 0) {
      st.mark(0);
      if (inflight >= 2)
        asm volatile("s_waitcnt vmcnt(12)" ::: "memory");
      else
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      st.mark(1);
      __builtin_amdgcn_s_barrier();
      st.mark(2);
      issue();
      --inflight;
      st.mark(3);
      st.laps<0, 1, 2>();
      st.step();
    }
    st.flush(p, wave, lane);
    return;
  }

  // ================= consumer waves: wave (wm, wn) owns rows wm*128 .. +128 (two 64-row halves), columns wn*64 .. +64 ==========
  const int wm = wave >> 1, wn = wave & 1;
  const int fr = lane & 15, fq = lane >> 4;
  const int a_frag = (wm * 128 + fr) * 128, b_frag = (wn * 64 + fr) * 128;
  const int slot0 = ((fq) ^ (fr & 7)) << 4, slot1 = ((4 + fq) ^ (fr & 7)) << 4;
  int c_stage = 0;
  RingStamps st;  // -> barrier | compute | epilogue

  // fragments of one k-substep: 8 A blocks (two row halves) + 4 W blocks; double-buffered by substep INSIDE a K-step
  Pack8<T> fa0[8], fb0[4], fa1[8], fb1[4];
  auto read_frags = [&](Pack8<T>* fa, Pack8<T>* fb, int stg, int slot) {
    const char* as = As + stg * STAGE_BYTES + a_frag + slot;
    const char* bs = Bs + stg * STAGE_BYTES + b_frag + slot;
    // in the order the MFMAs need them (row block i of both halves against all four column blocks, i = 0 first): the first
    // MFMA waits for three reads, not nine
    fb[0].u = *reinterpret_cast<const u32x4*>(bs);
    fa[0].u = *reinterpret_cast<const u32x4*>(as);
    fa[4].u = *reinterpret_cast<const u32x4*>(as + 4 * 2048);
#pragma unroll
    for (int j = 1; j < 4; ++j) fb[j].u = *reinterpret_cast<const u32x4*>(bs + j * 2048);
#pragma unroll
    for (int i = 1; i < 4; ++i) {
      fa[i].u = *reinterpret_cast<const u32x4*>(as + i * 2048);
      fa[4 + i].u = *reinterpret_cast<const u32x4*>(as + (4 + i) * 2048);
    }
  };

  for (int c_round = 0;; ++c_round) {
    const int w = work_id(c_round);
    if (w < 0) break;
    int mt, nt, split;
    decode(w, mt, nt, split);
    const int m0 = mt * BMW, n0 = nt * BN;
    const int kt0 = split * p.ktps;
    const int kt1 = (kt0 + p.ktps < nk_all) ? kt0 + p.ktps : nk_all;
    float bv[4][4];
    // dense: requested now, needed in the epilogue.  Conv modes (long K loops, a loader with far more scalar state): requested
    // in front of the epilogue - 16 registers less through the K loop is what keeps their loaders' state out of scratch
    if constexpr (AMODE == A_DENSE) load_bias_regs(p, bv, n0, wn, fq);

    f32x4 acc0[4][4], acc1[4][4];  // rows m0 + wm*128 + {0, 64} ..
    // (dead pieces, gemm_common.hpp piece_dead: skipped in the conv modes only - with the two extra branches the DENSE instance of
    //  this kernel goes from 21 to 74 spilled registers under hipcc and loses 1 % of a step; the conv instances go from 17 to 0)
    constexpr bool SKIP_DEAD = AMODE != A_DENSE;
    const bool res_done = residual_into_acc<T, SKIP_DEAD>(p, acc0, m0 + wm * 128, n0, 0, wn, fr, fq);
    if (res_done) {
      (void)residual_into_acc<T, SKIP_DEAD>(p, acc1, m0 + wm * 128 + 64, n0, 0, wn, fr, fq);
    } else {
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc0[i][j] = acc1[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
    }

    for (int kt = kt0; kt < kt1; ++kt) {
      st.mark(0);
      __builtin_amdgcn_s_barrier();  // stage c_stage is in LDS (and the loaders may overwrite the stage we left)
      st.mark(1);
      __builtin_amdgcn_sched_barrier(0);
      read_frags(fa0, fb0, c_stage, slot0);  // (exposed: three stages leave no landed stage to pre-read across the barrier)
      __builtin_amdgcn_sched_barrier(0);
      // second k-substep's 12 reads ride behind the first 12 MFMAs of the first (an MFMA holds the SIMD's issue for 8 of
      // its 16 cycles: the read goes in the gap), the other 20 cover the last read's latency - the ring kernel's pattern
      read_frags(fa1, fb1, c_stage, slot1);
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          acc0[i][j] = mfma16(fb0[j].v, fa0[i].v, acc0[i][j]);
          acc1[i][j] = mfma16(fb0[j].v, fa0[4 + i].v, acc1[i][j]);
        }
#pragma unroll
      for (int t = 0; t < 12; ++t) {
        __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);  // 1 MFMA
        __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);  // 1 DS read
      }
      __builtin_amdgcn_sched_group_barrier(0x008, 20, 0);
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          acc0[i][j] = mfma16(fb1[j].v, fa1[i].v, acc0[i][j]);
          acc1[i][j] = mfma16(fb1[j].v, fa1[4 + i].v, acc1[i][j]);
        }
      __builtin_amdgcn_sched_barrier(0);
      c_stage = (c_stage + 1 == NSTAGE) ? 0 : c_stage + 1;
      st.mark(2);
      st.laps<0, 1>();
      st.step();
    }
    st.mark(0);

    // ---------------- epilogue of this wave's 128x64 block, one 64-row half at a time (the loaders keep streaming) ----
    {
      if constexpr (AMODE != A_DENSE) load_bias_regs(p, bv, n0, wn, fq);
      const int m_eff = m0 + wm * 128;
      if (SKIP_DEAD && piece_dead(p, m_eff, n0 + wn * 64)) {
      } else if (AMODE == A_DENSE && !res_done && epilogue_lean16_ok(p, m_eff, n0 + wn * 64) && m_eff + 128 <= p.M) {
        epilogue_lean16<T>(p, acc0, bv, m_eff, n0 + wn * 64, fr, fq);  // (r06: see gemm_kernel)
        epilogue_lean16<T>(p, acc1, bv, m_eff + 64, n0 + wn * 64, fr, fq);
      } else if (epilogue_lean32_ok(p, m_eff, n0 + wn * 64, res_done) && m_eff + 128 <= p.M) {
        epilogue_lean32<T>(p, acc0, bv, m_eff, n0 + wn * 64, fr, fq, m_eff >> 6, split);
        epilogue_lean32<T>(p, acc1, bv, m_eff + 64, n0 + wn * 64, fr, fq, (m_eff + 64) >> 6, split);
      } else {
        epilogue_regs<T>(p, acc0, bv, m_eff, n0, 0, wn, fr, fq, m_eff >> 6, split, res_done);
        epilogue_regs<T>(p, acc1, bv, m_eff + 64, n0, 0, wn, fr, fq, (m_eff + 64) >> 6, split, res_done);
      }
    }
    st.mark(1);
    st.laps<2>();
  }
  st.flush(p, wave, lane);
}

}  // namespace pm
