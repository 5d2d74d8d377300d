// MFMA GEMM core for gfx950 with three A-operand loaders (dense rows, 3x3 im2col on channels-last
// frames, 3-tap temporal im2col) and a fused epilogue (bias, SiLU / GEGLU, residual).
//
//   C[M, N] = epi(A[M, K] . W[N, K]^T),  f32 accumulate on v_mfma_f32_16x16x32_{f16,bf16}.
//
// Tiling: 128x128 output tile per 256-thread workgroup (4 waves as 2x2, 64x64 per wave = 4x4 MFMA
// blocks), BK = 64, two LDS buffers, one barrier per K-tile.  16-bit A and W tiles go global -> LDS by
// DMA (global_load_lds_dwordx4: no VGPR round trip, no ds_write; the im2col gather and the padding
// are per-lane SOURCE addresses); an f32 A operand (residual stream) is staged through registers and
// rounded on the way.  LDS rows are 128 B with the 16-byte chunk index XOR-ed by (row & 7) - applied
// on the source side - so the ds_read_b128 fragment reads spread over the banks.  The epilogue works from
// registers (operands swapped in the MFMA, W rows interleaved by the loader: epilogue_regs), 16 bytes per lane.
#pragma once
#include "gemm_common.hpp"

namespace pm {

// 128x128 tile, 4 waves, 2 LDS stages, 2 workgroups per CU (any shape, split-K, f32 A).
template <typename T, int AMODE, bool A32>
__global__ __launch_bounds__(256, 2) void gemm_kernel(const GemmParams p) {
  typedef typename std::conditional<A32, float, T>::type TA;  // storage type of the A operand
  constexpr int ES = sizeof(TA);
  // Persistent walk (16-bit operands): a workgroup takes work items w, w + G, ...; the next item's first K-tile is
  // issued in the last K-step of this item and its barrier is deferred to BEHIND the epilogue (the epilogue is
  // LDS-free), so that DMA round trip and the next tile's residual / bias loads fly during the stores instead of
  // at the head of a fresh workgroup.  (The f32-operand instantiations stay one item per workgroup: the extra live
  // state pushed them past 256 VGPRs.)
  constexpr bool PERSIST = !A32;
  constexpr int NT = 256;                    // threads
  constexpr int WMW = 2;                     // waves along M (2 along N)
  constexpr int BMT = WMW * 64;              // tile rows
  constexpr int RSTEP = NT / 8;              // rows staged per loader pass
  constexpr int BP = BN / RSTEP;             // loader passes over the W tile (A tile: always 4)
  constexpr int A_BYTES = BMT * BK * 2, B_BYTES = BN * BK * 2;
  constexpr int STAGE_BYTES = A_BYTES + B_BYTES;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  // stage s: A tile at s*STAGE_BYTES, W tile right behind it
  char* const As = smem;
  char* const Bs = smem + A_BYTES;

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;
  const int fr = lane & 15, fq = lane >> 4;

  const int G = gridDim.x;
  const int nwork = p.mtiles * p.ntiles * p.splits;
  const int nk_all = (p.K + BK - 1) / BK;
  auto decode = [&](int w, int& mt, int& nt, int& split) { decode_work<AMODE, BMT>(p, w, mt, nt, split); };

  const char* const Ab = reinterpret_cast<const char*>(p.A);
  const char* const Wb = reinterpret_cast<const char*>(p.Wt);
  const char* const zero = reinterpret_cast<const char*>(p.zero);

  // ---- loader state.  This thread stages rows lr + 32*j, filling the PHYSICAL 16-byte slot tid & 7
  // of each 128-byte LDS row.  The XOR swizzle is applied on the SOURCE side: the lane fetches logical
  // k-chunk lc = slot ^ (row & 7) (row & 7 == lr & 7 for all four rows), so that the LDS image is
  // lane-linear, which is what a direct global->LDS DMA (global_load_lds_dwordx4) writes.
  // Addresses are kept as (wave-uniform 64-bit base that walks K) + (constant 32-bit lane offset) so the
  // main loop spends SALU, not VALU, on them: the kernel is otherwise VALU-issue-bound next to the MFMAs.
  const int lr = tid >> 3;
  const int lc = (tid & 7) ^ (lr & 7);
  uint32_t b_off[BP], a_off[4];
  int a_y[4], a_x[4];
  uint32_t inv[4] = {0u, 0u, 0u, 0u};  // fast conv modes: per row, the taps that are zero padding (see load_tile)
  // (tap, channel) position of the K walk.  Fast modes: one tap per K-tile (Cin % 64 == 0), tracked as
  // wave-uniform scalars.  General conv (stem Cin = 8, nearest-x2 upsample): per-lane.
  int tap_s = 0, ch_s = 0;       // uniform: tap and first channel of the current K-tile
  int tap_l = 0, ch_l = lc * 8;  // per-lane (A_CONV3X3 only)
  // point the loader at work item w; returns its first K-tile
  auto loader_begin = [&](int w) -> int {
    int mt, nt, split;
    decode(w, mt, nt, split);
    const int m0 = mt * BMT, n0 = nt * BN;
    const int kt0 = split * p.ktps;
#pragma unroll
    for (int j = 0; j < BP; ++j) {
      int n = n0 + cperm(lr + RSTEP * j, p.act == PM_ACT_GEGLU || p.natural);  // LDS row -> output column (epilogue_regs)
      if (n > p.N - 1) n = p.N - 1;
      b_off[j] = (uint32_t)(((int64_t)n * p.ldw + lc * 8) * 2);
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      int m = m0 + lr + RSTEP * j;
      if (m > p.M - 1) m = p.M - 1;
      if (AMODE == A_DENSE) {
        a_off[j] = (uint32_t)(((int64_t)m * p.lda + lc * 8) * ES);
        a_y[j] = a_x[j] = 0;
      } else if (AMODE == A_CONV3X3 || AMODE == A_CONV3X3_FAST) {
        const int hw = p.Ho * p.Wo;
        const int f = m / hw;
        const int rem = m - f * hw;
        const int oy = rem / p.Wo, ox = rem - oy * p.Wo;
        a_y[j] = oy * p.stride + 1 - p.pad;  // tap (dy, dx) reads virtual pixel (a_y + dy - 1, a_x + dx - 1)
        a_x[j] = ox * p.stride + 1 - p.pad;
        if (AMODE == A_CONV3X3_FAST) {  // no upsample: offset of the centre tap, the tap shift is uniform
          a_off[j] = (uint32_t)((((int64_t)f * p.Hin + a_y[j]) * p.Win + a_x[j]) * p.lda * ES + lc * 8 * ES);
          uint32_t bad = 0;
#pragma unroll
          for (int t = 0; t < 9; ++t) {
            const int ty = t / 3, tx = t - ty * 3;
            const bool ok = (unsigned)(a_y[j] + ty - 1) < (unsigned)p.Hv && (unsigned)(a_x[j] + tx - 1) < (unsigned)p.Wv;
            bad |= ok ? 0u : (1u << t);
          }
          inv[j] = bad;
        } else
          a_off[j] = (uint32_t)((int64_t)f * p.Hin * p.Win * p.lda * ES);
      } else {
        const int f = m / p.P;
        const int pix = m - f * p.P;
        a_off[j] = (uint32_t)((((int64_t)f * p.P + pix) * p.lda + lc * 8) * ES);
        const int fc = f % p.Fc;  // frame inside its clip (Fc == F unless clips are batched along the rows)
        a_y[j] = fc;
        a_x[j] = (int)(uint32_t)(((int64_t)pix * p.lda + lc * 8) * ES);  // byte offset of this row inside a halo frame
        inv[j] = (fc == 0 ? 1u : 0u) | (fc == p.Fc - 1 ? 4u : 0u);  // taps reaching frame -1 / frame Fc of the clip
      }
    }
    if (AMODE == A_CONV3X3_FAST) {  // channel-chunk-major walk: K-tile s = (chunk s / 9, tap s % 9), see load_tile
      const int chunk = kt0 / 9;
      tap_s = kt0 - chunk * 9;
      ch_s = chunk * BK;
    } else if (AMODE != A_DENSE) {
      tap_s = (kt0 * BK) / p.Cin;
      ch_s = kt0 * BK - tap_s * p.Cin;
      const int k_l = kt0 * BK + lc * 8;
      tap_l = k_l / p.Cin;
      ch_l = k_l - tap_l * p.Cin;
    }
    return kt0;
  };

  u32x4 ra[4], ra_hi[4], rb[BP];  // register staging (A32 only); ra_hi: second half of an f32 chunk
  // issue the loads of K-tile kt (tiles are requested in increasing order) into LDS buffer `buf`
  auto load_tile = [&](int kt, int buf) {
    const int kb = kt * BK;
    const bool kin_l = kb + lc * 8 < p.K;  // only the general conv mode can have a K tail
    const char* wb = Wb + (int64_t)((AMODE == A_DENSE && p.kwrap && kb >= p.kwrap) ? kb - p.kwrap : kb) * 2;
    const char* ab = Ab;
    const char *hlo = nullptr, *hhi = nullptr;  // temporal mode: halo frames at this K-tile's channel (uniform)
    int dy = 0, dx = 0;
    if (AMODE == A_DENSE) {
      ab = Ab + (int64_t)kb * ES;
    } else if (AMODE == A_CONV3X3_FAST) {
      // The fast 3x3 mode walks K channel-chunk-major: all 9 taps of a 64-channel chunk back to back (the
      // packed weights stay tap-major, only the order of summation changes).  The 9 taps re-read the same
      // input rows; tap-major put a whole pass over all channels (more than an XCD's L2 holds, with 32-64
      // tiles in flight) between two reads of a line and the fabric saw 2-2.7x the algorithmic bytes.
      dy = tap_s / 3;
      dx = tap_s - dy * 3;
      wb = Wb + ((int64_t)tap_s * p.Cin + ch_s) * 2;
      ab = Ab + ((int64_t)((dy - 1) * p.Win + (dx - 1)) * p.lda + ch_s) * ES;
    } else if (AMODE == A_CONVT3) {
      ab = Ab + ((int64_t)(tap_s - 1) * p.P * p.lda + ch_s) * ES;
      hlo = p.halo_lo ? reinterpret_cast<const char*>(p.halo_lo) + (int64_t)ch_s * ES : nullptr;
      hhi = p.halo_hi ? reinterpret_cast<const char*>(p.halo_hi) + (int64_t)ch_s * ES : nullptr;
    } else {
      dy = tap_l / 3;
      dx = tap_l - dy * 3;
    }
    // Fast conv modes without halo frames, 16-bit operands: the A tile goes through a buffer descriptor whose
    // base carries the uniform tap shift; a padding lane gets offset ~0 = out of range, for which
    // `buffer_load ... lds` writes zeros (see gemm_ring_kernel): 2-3 VALU per DMA instead of ~8.
    const bool use_desc = !A32 && (AMODE == A_CONV3X3_FAST || AMODE == A_CONVT3) && p.halo_lo == nullptr && p.halo_hi == nullptr;
    if constexpr (!A32) {
      if (use_desc) {
        const uint32_t nrec = (uint32_t)((Ab + p.a_bytes) - ab);
        __amdgpu_buffer_rsrc_t rsrc = __builtin_amdgcn_make_buffer_rsrc((void*)ab, (short)0, (int)nrec, 0x00020000);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const uint32_t voff = a_off[j] | (uint32_t)(-(int)((inv[j] >> tap_s) & 1u));
          const int dst = buf * STAGE_BYTES + (RSTEP * j + 8 * wave) * 128;
          __builtin_amdgcn_raw_ptr_buffer_load_lds(rsrc, (lds_void*)(As + dst), 16, voff, 0, 0, 0);
        }
      }
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (use_desc) break;
      const char* src;
      if (AMODE == A_DENSE) {
        src = ab + a_off[j];
      } else if (AMODE == A_CONV3X3_FAST) {
        const bool ok = (unsigned)(a_y[j] + dy - 1) < (unsigned)p.Hv && (unsigned)(a_x[j] + dx - 1) < (unsigned)p.Wv;
        src = ok ? ab + a_off[j] : zero;
      } else if (AMODE == A_CONVT3) {
        // (per-row halo offsets are precomputed: the 64-bit multiplies that stood here made the loader the
        // bottleneck of the temporal conv: 1 250-1 450 issue cycles per K-step against 550 for dense)
        const int sf = a_y[j] + tap_s - 1;
        src = ab + a_off[j];
        if (sf < 0) src = hlo ? hlo + (uint32_t)a_x[j] : zero;
        if (sf >= p.Fc) src = hhi ? hhi + (uint32_t)a_x[j] : zero;
      } else {
        int iy = a_y[j] + dy - 1, ix = a_x[j] + dx - 1;
        const bool ok = kin_l && (unsigned)iy < (unsigned)p.Hv && (unsigned)ix < (unsigned)p.Wv;
        if (p.ups) {
          iy >>= 1;
          ix >>= 1;
        }
        src = ok ? Ab + a_off[j] + (((int64_t)iy * p.Win + ix) * p.lda + ch_l) * ES : zero;
      }
      if constexpr (A32) {  // f32 stream operand: through registers (needs the f32 -> 16-bit rounding)
        ra[j] = ld_global16(src);
        ra_hi[j] = ld_global16(src + 16);
      } else {  // 16-bit operands: DMA straight into the tile, 1 KiB per wave-instruction
        const int dst = buf * STAGE_BYTES + (RSTEP * j + 8 * wave) * 128;
        __builtin_amdgcn_global_load_lds((glb_void*)src, (lds_void*)(As + dst), 16, 0, 0);
      }
    }
#pragma unroll
    for (int j = 0; j < BP; ++j) {
      const char* wsrc = (AMODE == A_CONV3X3 && !kin_l) ? zero : wb + b_off[j];
      if constexpr (A32) {
        rb[j] = ld_global16(wsrc);
      } else {
        const int dst = buf * STAGE_BYTES + (RSTEP * j + 8 * wave) * 128;
        __builtin_amdgcn_global_load_lds((glb_void*)wsrc, (lds_void*)(Bs + dst), 16, 0, 0);
      }
    }
    if (AMODE == A_CONV3X3_FAST) {  // next tap of this channel chunk, then the next chunk
      if (++tap_s == 9) {
        tap_s = 0;
        ch_s += BK;
      }
    } else if (AMODE != A_DENSE) {  // advance the (tap, channel) walk to the next K-tile
      ch_s += BK;
      if (ch_s >= p.Cin) {
        ch_s -= p.Cin;
        ++tap_s;
      }
      if (AMODE == A_CONV3X3) {
        ch_l += BK;
        while (ch_l >= p.Cin) {
          ch_l -= p.Cin;
          ++tap_l;
        }
      }
    }
  };
  auto store_tile = [&](int buf) {
    if constexpr (!A32) return;  // DMA path: the tile is already in flight to LDS
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int off = buf * STAGE_BYTES + (lr + RSTEP * j) * 128 + ((tid & 7) << 4);
      union { u32x4 u; float f[4]; } lo, hi;
      lo.u = ra[j];
      hi.u = ra_hi[j];
      Pack8<T> cv;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        cv.e[e] = from_f32<T>(lo.f[e]);
        cv.e[e + 4] = from_f32<T>(hi.f[e]);
      }
      if (p.a_lo) {  // (uniform) second pass of a split-operand call: what the first pass rounded away
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          cv.e[e] = from_f32<T>(lo.f[e] - to_f32(cv.e[e]));
          cv.e[e + 4] = from_f32<T>(hi.f[e] - to_f32(cv.e[e + 4]));
        }
      }
      *reinterpret_cast<u32x4*>(As + off) = cv.u;
      *reinterpret_cast<u32x4*>(Bs + off) = rb[j];
    }
  };

  // fragment read offsets: row & 7 == fr & 7 for every MFMA block of this wave, so the swizzled slot
  // depends on the k-step only; the block index becomes an immediate offset of the ds_read_b128
  const int a_frag = (wm * 64 + fr) * 128, b_frag = (wn * 64 + fr) * 128;
  const int slot0 = ((fq) ^ (fr & 7)) << 4, slot1 = ((4 + fq) ^ (fr & 7)) << 4;

  int w = xcd_remap(blockIdx.x, G);  // (G <= nwork: every workgroup has a first item)
  int buf = 0;
  load_tile(loader_begin(w), 0);
  // The residual (accumulator start values) and the bias of the FIRST tile are requested right behind its first
  // K-tile's DMA and before the barrier that waits for it: their round trips overlap.  They used to be issued after
  // that barrier and waited for on their own - two memory latencies in a row at the head of every workgroup, as
  // long as the whole K loop of a K = 320 GEMM.
  f32x4 acc[4][4];
  float bv[4][4];
  bool res_done;
  {
    int mt, nt, split;
    decode(w, mt, nt, split);
    res_done = residual_into_acc<T>(p, acc, mt * BMT, nt * BN, wm, wn, fr, fq);
    load_bias_regs(p, bv, nt * BN, wn, fq);
  }
  store_tile(0);
  __syncthreads();  // (hipcc drains vmcnt before the barrier, so the DMA'd tile is visible)

  for (bool first_item = true;; first_item = false) {
    int mt, nt, split;
    decode(w, mt, nt, split);
    const int m0 = mt * BMT, n0 = nt * BN;
    const int kt0 = split * p.ktps;
    const int kt1 = (kt0 + p.ktps < nk_all) ? kt0 + p.ktps : nk_all;
    const bool has_next = PERSIST && (w + G < nwork);

    if (!first_item) {
      res_done = residual_into_acc<T>(p, acc, m0, n0, wm, wn, fr, fq);
      load_bias_regs(p, bv, n0, wn, fq);  // requested now, needed in the epilogue
    }
    if (!res_done) {
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
    }

    for (int kt = kt0; kt < kt1; ++kt) {
      const bool more = (kt + 1 < kt1) || has_next;
      if (kt + 1 < kt1)
        load_tile(kt + 1, buf ^ 1);
      else if (has_next)  // first K-tile of the next work item: in flight during this item's epilogue
        load_tile(loader_begin(w + G), buf ^ 1);
      const char* as = As + buf * STAGE_BYTES + a_frag;
      const char* bs = Bs + buf * STAGE_BYTES + b_frag;
      // all 16 fragment reads of the K-tile are issued first (64 VGPRs), so the MFMAs of k-step 0 start
      // as soon as ITS operands land and the reads of k-step 1 are hidden behind them; written per
      // k-step the compiler serialises read -> lgkmcnt(0) -> MFMA four times per tile
      Pack8<T> a[2][4], b[2][4];
#pragma unroll
      for (int ks = 0; ks < 2; ++ks) {
        const int slot = ks ? slot1 : slot0;
#pragma unroll
        for (int i = 0; i < 4; ++i) a[ks][i].u = *reinterpret_cast<const u32x4*>(as + i * 2048 + slot);
#pragma unroll
        for (int j = 0; j < 4; ++j) b[ks][j].u = *reinterpret_cast<const u32x4*>(bs + j * 2048 + slot);
      }
#pragma unroll
      for (int ks = 0; ks < 2; ++ks) {
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
          for (int j = 0; j < 4; ++j) acc[i][j] = mfma16(b[ks][j].v, a[ks][i].v, acc[i][j]);  // C^T: see epilogue_regs
      }
      if (more) store_tile(buf ^ 1);
      if (kt + 1 < kt1 || !has_next) __syncthreads();  // (last step before a prefetched item: barrier after the epilogue)
      buf ^= 1;
    }
    // ---------------- epilogue: registers -> global (no LDS staging, no barrier) ----------------
    // split-K slices store raw f32 partials into their slab; bias/act/residual run in the reduce pass
    // (r06: the 16-bit projection flavours - q|k|v with its column scale, plain / bias - on the lean epilogue where the wave's
    // 64 x 64 piece lies inside the matrix: gemm_common.hpp epilogue_lean16)
    if (piece_dead(p, m0 + wm * 64, n0 + wn * 64)) {
      // (nothing of this wave's piece is inside the matrix)
    } else if (AMODE == A_DENSE && !res_done && epilogue_lean16_ok(p, m0 + wm * 64, n0 + wn * 64))
      epilogue_lean16<T>(p, acc, bv, m0 + wm * 64, n0 + wn * 64, fr, fq);
    else if (epilogue_lean32_ok(p, m0 + wm * 64, n0 + wn * 64, res_done))  // (the all-f32 flavours of every A mode)
      epilogue_lean32<T>(p, acc, bv, m0 + wm * 64, n0 + wn * 64, fr, fq, mt * WMW + wm, split);
    else
      epilogue_regs<T>(p, acc, bv, m0, n0, wm, wn, fr, fq, mt * WMW + wm, split, res_done);
    if (!has_next) break;
    w += G;
    __syncthreads();  // the prefetched first K-tile of item w has landed (vmcnt drained here, behind the stores)
  }
}

}  // namespace pm
