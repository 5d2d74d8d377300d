// MXFP8 (OCP e4m3fn elements, one E8M0 power-of-two scale per 32 consecutive elements along K) for the projections of the
// U-Net's transformer blocks: the quantiser pm_quant_mx8 (plain, or LayerNorm-fused on the f32 residual stream) and the
// block-scaled GEMM pm_gemm_mx8 on v_mfma_scale_f32_16x16x128_f8f6f4 (K = 128 per instruction at twice the bf16 rate, the
// scales applied inside the instruction).  Quantisation rule: include/pandora_mi355x.h, "MXFP8".
#include "gemm_common.hpp"
#include "mx8_common.hpp"

namespace pm {
namespace {

typedef __attribute__((ext_vector_type(8))) int i32x8;

// ---- the quantisation rule: mx8_exp / mx8_inv_scale / e4m3_rne / mx8_block of mx8_common.hpp -----------------------------
template <typename TI>
__device__ __forceinline__ void load8(const TI* p, float (&v)[8]) {
  Pack8<TI> t;
  t.u = ld_global16(p);
#pragma unroll
  for (int e = 0; e < 8; ++e) v[e] = to_f32(t.e[e]);
}
__device__ __forceinline__ void load8(const float* p, float (&v)[8]) {
  const f32x4 a = *reinterpret_cast<const f32x4*>(p), b = *reinterpret_cast<const f32x4*>(p + 4);
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    v[e] = a[e];
    v[4 + e] = b[e];
  }
}

// ---- pm_quant_mx8: one wave per row, 8 consecutive elements per lane, a block = 4 adjacent lanes --------------------------
constexpr int QMAX_IT = 8;  // LayerNorm mode keeps the row in registers: K <= 8 * 512 = 4096

template <typename TI, bool LN>
__global__ __launch_bounds__(256) void mx8_quant_kernel(const TI* __restrict__ x, int64_t ldx, const float* __restrict__ gamma,
                                                        const float* __restrict__ beta, float eps, uint8_t* __restrict__ q,
                                                        int64_t ldq, uint8_t* __restrict__ s, int64_t lds, int M, int K) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= M) return;
  const TI* xr = x + (int64_t)row * ldx;
  uint8_t* qr = q + (int64_t)row * ldq;
  uint8_t* sr = s + (int64_t)row * lds;
  const int nit = (K + 511) >> 9;
  if constexpr (!LN) {
    for (int it = 0; it < nit; ++it) {
      const int col = (it * 64 + lane) * 8;
      float v[8];
      if (col < K) {
        load8(xr + col, v);
      } else {
#pragma unroll
        for (int e = 0; e < 8; ++e) v[e] = 0.f;
      }
      uint32_t w0, w1;
      const uint32_t code = mx8_block<1, 2>(v, w0, w1);  // (K % 32 == 0: the 4 lanes of a block share one fate)
      if (col < K) {
        *reinterpret_cast<u32x2*>(qr + col) = u32x2{w0, w1};
        if ((lane & 3) == 0) sr[col >> 5] = (uint8_t)code;
      }
    }
  } else {
    // LayerNorm as pm_layernorm computes it (mean, then the centred sum of squares, rsqrt(var + eps), * gamma + beta in f32),
    // quantised from the f32 value: the 16-bit LayerNorm output never exists
    float v[QMAX_IT][8];
    float sum = 0.f;
#pragma unroll
    for (int it = 0; it < QMAX_IT; ++it) {
      const int col = (it * 64 + lane) * 8;
      if (it < nit && col < K) {
        load8(xr + col, v[it]);
      } else {
#pragma unroll
        for (int e = 0; e < 8; ++e) v[it][e] = 0.f;
      }
#pragma unroll
      for (int e = 0; e < 8; ++e) sum += v[it][e];
    }
    const float mean = wave_sum(sum) / (float)K;
    float ss = 0.f;
#pragma unroll
    for (int it = 0; it < QMAX_IT; ++it) {
      const int col = (it * 64 + lane) * 8;
      if (it < nit && col < K) {
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          const float d = v[it][e] - mean;
          ss = fmaf(d, d, ss);
        }
      }
    }
    const float rstd = rsqrtf(wave_sum(ss) / (float)K + eps);
#pragma unroll
    for (int it = 0; it < QMAX_IT; ++it) {
      if (it >= nit) break;
      const int col = (it * 64 + lane) * 8;
      float y[8];
      if (col < K) {
        float g[8], b[8];
        load8(gamma + col, g);
        load8(beta + col, b);
#pragma unroll
        for (int e = 0; e < 8; ++e) y[e] = (v[it][e] - mean) * rstd * g[e] + b[e];
      } else {
#pragma unroll
        for (int e = 0; e < 8; ++e) y[e] = 0.f;
      }
      uint32_t w0, w1;
      const uint32_t code = mx8_block<1, 2>(y, w0, w1);
      if (col < K) {
        *reinterpret_cast<u32x2*>(qr + col) = u32x2{w0, w1};
        if ((lane & 3) == 0) sr[col >> 5] = (uint8_t)code;
      }
    }
  }
}

// ---- pm_gemm_mx8 ------------------------------------------------------------------------------------------------------------
// 128 x 128 output tile, 4 waves of 64 x 64 (acc[4][4] of 16x16 blocks), BK = 128 fp8 = the bytes of the bf16 kernels' BK = 64.
// Both operands are staged through registers (one K-step ahead) into two LDS buffers of 128 rows x 128 bytes each, the 16-byte
// chunks of a row XOR-swizzled by (row & 7); the zero-filled second half of the last K-step (K % 128 == 64) comes for free.
// Operand map of v_mfma_scale_f32_16x16x128_f8f6f4 (tools/probes/mfma_scale16_layout.hip, exact integers with a different
// scale per lane): lane l holds row l & 15 in two K = 64 halves - bytes 0..15 are k = 16 (l >> 4) + 0..15, bytes 16..31 are
// k = 64 + 16 (l >> 4) + 0..15 - while its scale operand scales the 32-block k = 32 (l >> 4) .. +31 of that row (whose bytes
// other lanes hold).  So a lane reads 16-byte chunks l >> 4 and 4 + (l >> 4) of its row and passes the scale of block l >> 4.  As in the bf16 kernels the MFMA computes C^T (W fragment as the instruction's A), so
// lane (fr = l & 15, fq = l >> 4) accumulates row m = 16 i + fr, columns n = 16 j + 4 fq + r (r = 0..3) of block (i, j).
constexpr int MX_BM = 128, MX_BN = 128, MX_BK = 128;
constexpr int MX_TILE = MX_BM * MX_BK;  // bytes per operand and buffer

enum { MX_EPI_16 = 0, MX_EPI_F32 = 1, MX_EPI_GEGLU = 2, MX_EPI_GEGLU_MX = 3, MX_EPI_QKV8 = 4 };
// A-loader modes.  MX_LD_DENSE: A is [M, K].  MX_LD_C3 / MX_LD_T3 (pm_conv2d_3x3_mx8 / pm_conv_temporal_k3_mx8): A is the MXFP8
// activation [rows, Cin] and K index k is channel k % Cin of tap k / Cin, read from the tap's neighbour row (3x3: pixel
// (y + tap / 3 - 1, x + tap % 3 - 1) of the same frame; temporal: the same pixel of frame f + tap - 1 of the same clip).  With
// Cin % 32 == 0 a 16-byte chunk and a 32-block lie inside one tap, a 128-byte K-step does not (Cin = 320: 2.5 steps per tap,
// Cin = 64: two taps per step): the tap is looked up per chunk and per scale block.  A tap outside the frame / clip is padding:
// zero elements with scale 2^0, exactly what a zero-filled im2col operand would hold - the K walk is pm_gemm_mx8's.
enum { MX_LD_DENSE = 0, MX_LD_C3 = 1, MX_LD_T3 = 2 };

struct Mx8Params {
  const uint8_t* A;
  int64_t lda;
  const uint8_t* As;
  int64_t ldas;
  const uint8_t* W;
  int64_t ldw;
  const uint8_t* Ws;
  int64_t ldws;
  const float* bias;
  const void* R;
  int64_t ldr;
  void* C;
  int64_t ldc;
  uint8_t* Cs;
  int64_t ldcs;
  int M, N, K;
  int bias_mul;  // PM_FLAG_BIAS_IS_SCALE
  int res32;     // residual is f32
  int mtiles, ntiles;
  // MX_EPI_QKV8 only (appended: the other flavours' argument offsets stay where they were)
  uint8_t* q8;
  uint8_t* k8;
  uint8_t* v8t;
  int heads, P;  // tokens per batch item (P % 64 == 0, M = B * P)
  float qmul;    // extra factor on the q columns (1 when the prescale arrives as the column scale)
  // MX_LD_C3 / MX_LD_T3 only (appended likewise)
  int cin;       // channels per tap (K = taps * cin)
  int fh, fw;    // 3x3: frame height and width (row m = (f * fh + y) * fw + x)
  int px, clip;  // temporal: pixels per frame (row m = f * px + pixel) and frames per clip
};

__device__ __forceinline__ int swz(int row, int chunk) { return row * MX_BK + ((chunk ^ (row & 7)) << 4); }

// conv loaders: bit t of the mask = tap t of row m reads a real row (else padding); tap_rows = how many rows further it lies
template <int LD>
__device__ __forceinline__ int tap_mask(const Mx8Params& p, int m) {
  if constexpr (LD == MX_LD_C3) {
    const int rem = m % (p.fh * p.fw), y = rem / p.fw, x = rem - y * p.fw;
    const int xm = (x > 0 ? 1 : 0) | 2 | (x < p.fw - 1 ? 4 : 0);
    return (y > 0 ? xm : 0) | (xm << 3) | (y < p.fh - 1 ? xm << 6 : 0);
  } else {
    const int fi = (m / p.px) % p.clip;
    return (fi > 0 ? 1 : 0) | 2 | (fi < p.clip - 1 ? 4 : 0);
  }
}
template <int LD>
__device__ __forceinline__ int tap_rows(const Mx8Params& p, int tap) {
  if constexpr (LD == MX_LD_C3) {
    const int dy = tap / 3;
    return (dy - 1) * p.fw + (tap - 3 * dy - 1);
  } else {
    return (tap - 1) * p.px;
  }
}

template <typename T, int EPI, int LD = MX_LD_DENSE>
__global__ __launch_bounds__(256, 2) void gemm_mx8_kernel(Mx8Params p) {
  __shared__ __attribute__((aligned(16))) uint8_t lds[2][2][MX_TILE];  // [buffer][A, W]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1, fr = lane & 15, fq = lane >> 4;
  const int nwg = p.mtiles * p.ntiles;
  const int bid = xcd_remap(blockIdx.x, nwg);
  const int mt = bid / p.ntiles, nt = bid - mt * p.ntiles;
  const int m0 = mt * MX_BM, n0 = nt * MX_BN;
  const int nk = (p.K + MX_BK - 1) / MX_BK;
  const int kblocks = p.K >> 5;

  // staging: chunk c = tid + 256 q (q = 0..3) of a tile is row c >> 3, 16-byte chunk c & 7
  const uint8_t* ga[4];
  const uint8_t* gw[4];
  int lo[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int c = tid + 256 * q, row = c >> 3, ch = c & 7;
    const int am = min(m0 + row, p.M - 1), wr = min(n0 + row, p.N - 1);  // (clamped rows: loaded, never stored)
    ga[q] = p.A + (int64_t)am * p.lda + ch * 16;
    gw[q] = p.W + (int64_t)wr * p.ldw + ch * 16;
    lo[q] = swz(row, ch);
  }
  int qmask[4], smask[4];  // conv loaders: tap masks of the staged rows and of the fragments' scale rows
  if constexpr (LD != MX_LD_DENSE) {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      qmask[q] = tap_mask<LD>(p, min(m0 + ((tid + 256 * q) >> 3), p.M - 1));
      smask[q] = tap_mask<LD>(p, min(m0 + wm * 64 + q * 16 + fr, p.M - 1));
    }
  }
  // scale rows of this lane's fragments
  const uint8_t* sa[4];
  const uint8_t* sw[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    sa[i] = p.As + (int64_t)min(m0 + wm * 64 + i * 16 + fr, p.M - 1) * p.ldas;
    sw[i] = p.Ws + (int64_t)min(n0 + wn * 64 + i * 16 + fr, p.N - 1) * p.ldws;
  }

  u32x4 ra[4], rw[4];
  int xa[4], xw[4];
  auto fetch = [&](int kt) {
    const int k0 = kt * MX_BK;
    const int kb = kt * 4 + fq;  // past K (zero-filled half step): any finite scale, 2^0
    if constexpr (LD == MX_LD_DENSE) {
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int ch = (tid + 256 * q) & 7;
        const bool in = k0 + ch * 16 < p.K;
        ra[q] = in ? ld_global16(ga[q] + k0) : u32x4{0u, 0u, 0u, 0u};
        rw[q] = in ? ld_global16(gw[q] + k0) : u32x4{0u, 0u, 0u, 0u};
      }
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        xa[i] = kb < kblocks ? (int)sa[i][kb] : 127;
        xw[i] = kb < kblocks ? (int)sw[i][kb] : 127;
      }
    } else {
      // this thread's chunk (the same column of all four staged rows): tap and channel of its first element
      const int k = k0 + (tid & 7) * 16;
      const bool in = k < p.K;
      const int tap = in ? k / p.cin : 0;
      const int64_t aoff = (int64_t)tap_rows<LD>(p, tap) * p.lda + (k - tap * p.cin) - (tid & 7) * 16;  // (ga holds ch * 16)
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        ra[q] = in && ((qmask[q] >> tap) & 1) ? ld_global16(ga[q] + aoff) : u32x4{0u, 0u, 0u, 0u};
        rw[q] = in ? ld_global16(gw[q] + k0) : u32x4{0u, 0u, 0u, 0u};
      }
      // this lane's scale block 4 kt + fq: block (k % Cin) / 32 of the tap's neighbour row
      const bool ins = kb < kblocks;
      const int ks = kb * 32, stap = ins ? ks / p.cin : 0;
      const int64_t soff = (int64_t)tap_rows<LD>(p, stap) * p.ldas + ((ks - stap * p.cin) >> 5);
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        xa[i] = ins && ((smask[i] >> stap) & 1) ? (int)sa[i][soff] : 127;
        xw[i] = ins ? (int)sw[i][kb] : 127;
      }
    }
  };
  auto stage = [&](int buf) {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      *reinterpret_cast<u32x4*>(&lds[buf][0][lo[q]]) = ra[q];
      *reinterpret_cast<u32x4*>(&lds[buf][1][lo[q]]) = rw[q];
    }
  };

  f32x4 acc[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  fetch(0);
  stage(0);
  __syncthreads();
  for (int kt = 0; kt < nk; ++kt) {
    const int buf = kt & 1;
    int ca[4], cw[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      ca[i] = xa[i];
      cw[i] = xw[i];
    }
    if (kt + 1 < nk) fetch(kt + 1);
    i32x8 fa[4], fw[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int ra_ = wm * 64 + i * 16 + fr, rw_ = wn * 64 + i * 16 + fr;
      const u32x4 a0 = *reinterpret_cast<const u32x4*>(&lds[buf][0][swz(ra_, fq)]);
      const u32x4 a1 = *reinterpret_cast<const u32x4*>(&lds[buf][0][swz(ra_, 4 + fq)]);
      const u32x4 w0 = *reinterpret_cast<const u32x4*>(&lds[buf][1][swz(rw_, fq)]);
      const u32x4 w1 = *reinterpret_cast<const u32x4*>(&lds[buf][1][swz(rw_, 4 + fq)]);
      fa[i] = i32x8{(int)a0[0], (int)a0[1], (int)a0[2], (int)a0[3], (int)a1[0], (int)a1[1], (int)a1[2], (int)a1[3]};
      fw[i] = i32x8{(int)w0[0], (int)w0[1], (int)w0[2], (int)w0[3], (int)w1[0], (int)w1[1], (int)w1[2], (int)w1[3]};
    }
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j)
        acc[i][j] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(fw[j], fa[i], acc[i][j], 0, 0, 0, cw[j], 0, ca[i]);
    if (kt + 1 < nk) stage(buf ^ 1);
    __syncthreads();
  }

  // ---- epilogue: bias (or column scale) -> GEGLU -> residual -> store, from the registers --------------------------------
  const int nw0 = n0 + wn * 64;
  if (nw0 >= p.N) return;  // (ragged last column tile: this wave's piece lies outside)
  float bv[4][4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int n = nw0 + j * 16 + 4 * fq;
    const bool ok = p.bias != nullptr && n < p.N;
    const f32x4 t = ok ? *reinterpret_cast<const f32x4*>(p.bias + n) : f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int r = 0; r < 4; ++r) bv[j][r] = ok ? t[r] : (p.bias_mul ? 1.f : 0.f);
  }
  if constexpr (EPI == MX_EPI_QKV8) {
    // q|k|v as the packed e4m3 operands of pm_attention_fp8_packed (layout: include/pandora_mi355x.h).  A wave's 64 x 64 piece is
    // ONE (batch item, part, head, 64-token tile): P % 64 == 0 keeps its rows inside a batch item and on a tile boundary, and
    // inner = heads * 64 keeps its columns inside one head of one part - whatever the 128-column tile straddles.  The codes go
    // through the wave's own slice of the staging LDS (idle after the K loop; the loop's last barrier has retired every read of
    // it), so that they leave as 16-byte stores: Q / K tiles are 4 KiB contiguous, V^T tiles 64 rows of 64 bytes.
    const int mw0 = m0 + wm * 64;
    if (mw0 >= p.M) return;  // (M % 128 == 64: the lower half of the last tile lies outside; M % 64 == 0)
    const int inner = p.heads * 64;
    const int part = nw0 / inner, head = (nw0 - part * inner) >> 6;
    const int b = mw0 / p.P, t0 = mw0 - b * p.P;
    const int64_t bh = (int64_t)b * p.heads + head;
    uint8_t* const wl = &lds[0][0][0] + wave * 4096;
    const float mul = part == 0 ? p.qmul : 1.0f;
    uint32_t code[4][4];  // [i][j]: row 16 i + fr, bytes = columns 16 j + 4 fq + 0..3
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        uint32_t w = 0;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          float y = p.bias_mul ? acc[i][j][r] * bv[j][r] : acc[i][j][r] + bv[j][r];
          if (part == 0) y *= mul;
          w |= e4m3_sat(y) << (8 * r);
        }
        code[i][j] = w;
      }
    if (part < 2) {
      // rows of 64 bytes, the 16-byte chunk XOR-ed with (row >> 2) & 3: dword writes and 16-byte reads without bank conflicts
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int row = 16 * i + fr;
#pragma unroll
        for (int j = 0; j < 4; ++j) *reinterpret_cast<uint32_t*>(wl + row * 64 + ((j ^ ((row >> 2) & 3)) << 4) + 4 * fq) = code[i][j];
      }
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
      uint8_t* dst = (part == 0 ? p.q8 : p.k8) + (bh * p.P + t0) * 64;
#pragma unroll
      for (int it = 0; it < 4; ++it) {
        const int row = 16 * it + (lane >> 2), ch = lane & 3;
        const u32x4 t = *reinterpret_cast<const u32x4*>(wl + row * 64 + ((ch ^ ((row >> 2) & 3)) << 4));
        st_global16(dst + row * 64 + ch * 16, t);
      }
    } else {
      // V^T: byte (key, d) -> row d, byte pos(key) = 32 ((key >> 2) & 1) + 4 (key >> 3) + (key & 3) of the 64-key tile
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int key = 16 * i + fr;
        const int pos = 32 * ((key >> 2) & 1) + 4 * (key >> 3) + (key & 3);
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
          for (int r = 0; r < 4; ++r) wl[(16 * j + 4 * fq + r) * 64 + pos] = (uint8_t)(code[i][j] >> (8 * r));
      }
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
      uint8_t* dst = p.v8t + bh * 64 * p.P + t0;
#pragma unroll
      for (int it = 0; it < 4; ++it) {
        const int d = 16 * it + (lane >> 2), ch = lane & 3;
        const u32x4 t = *reinterpret_cast<const u32x4*>(wl + d * 64 + ch * 16);
        st_global16(dst + (int64_t)d * p.P + ch * 16, t);
      }
    }
  } else if constexpr (EPI == MX_EPI_GEGLU || EPI == MX_EPI_GEGLU_MX) {
    // value block 2jj, gate block 2jj + 1 (weights packed [16 value | 16 gate]); the wave's 32 output columns are ONE MX block
    const int nc = (nw0 >> 1) + 4 * fq;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int m = m0 + wm * 64 + i * 16 + fr;
      float v[8];
#pragma unroll
      for (int jj = 0; jj < 2; ++jj)
#pragma unroll
        for (int r = 0; r < 4; ++r)
          v[4 * jj + r] = (acc[i][2 * jj][r] + bv[2 * jj][r]) * gelu_erf_f(acc[i][2 * jj + 1][r] + bv[2 * jj + 1][r]);
      if constexpr (EPI == MX_EPI_GEGLU_MX) {
        uint32_t w0, w1;
        const uint32_t code = mx8_block<16, 32>(v, w0, w1);  // (wave-wide shuffles: before the row mask)
        if (m < p.M) {
          uint8_t* cr = reinterpret_cast<uint8_t*>(p.C) + (int64_t)m * p.ldc + nc;
          *reinterpret_cast<uint32_t*>(cr) = w0;
          *reinterpret_cast<uint32_t*>(cr + 16) = w1;
          if (fq == 0) p.Cs[(int64_t)m * p.ldcs + (nw0 >> 6)] = (uint8_t)code;
        }
      } else if (m < p.M) {
        T* cr = reinterpret_cast<T*>(p.C) + (int64_t)m * p.ldc + nc;
#pragma unroll
        for (int jj = 0; jj < 2; ++jj) {
          Pack4<T> o;
#pragma unroll
          for (int r = 0; r < 4; ++r) o.e[r] = from_f32<T>(v[4 * jj + r]);
          *reinterpret_cast<u32x2*>(cr + 16 * jj) = o.u;
        }
      }
    }
  } else {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int m = m0 + wm * 64 + i * 16 + fr;
      if (m >= p.M) continue;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int n = nw0 + j * 16 + 4 * fq;
        if (n >= p.N) continue;
        float v[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) v[r] = p.bias_mul ? acc[i][j][r] * bv[j][r] : acc[i][j][r] + bv[j][r];
        if (p.R != nullptr) {
          if (p.res32) {
            const f32x4 t = *reinterpret_cast<const f32x4*>(reinterpret_cast<const float*>(p.R) + (int64_t)m * p.ldr + n);
#pragma unroll
            for (int r = 0; r < 4; ++r) v[r] += t[r];
          } else {
            Pack4<T> t;
            t.u = *reinterpret_cast<const u32x2*>(reinterpret_cast<const T*>(p.R) + (int64_t)m * p.ldr + n);
#pragma unroll
            for (int r = 0; r < 4; ++r) v[r] += to_f32(t.e[r]);
          }
        }
        if constexpr (EPI == MX_EPI_F32) {
          *reinterpret_cast<f32x4*>(reinterpret_cast<float*>(p.C) + (int64_t)m * p.ldc + n) = f32x4{v[0], v[1], v[2], v[3]};
        } else {
          Pack4<T> o;
#pragma unroll
          for (int r = 0; r < 4; ++r) o.e[r] = from_f32<T>(v[r]);
          *reinterpret_cast<u32x2*>(reinterpret_cast<T*>(p.C) + (int64_t)m * p.ldc + n) = o.u;
        }
      }
    }
  }
}

inline bool aligned(const void* ptr, uintptr_t a) { return (reinterpret_cast<uintptr_t>(ptr) & (a - 1)) == 0; }

}  // namespace
}  // namespace pm

using namespace pm;

extern "C" int pm_quant_mx8(const void* x, int64_t ldx, const float* gamma, const float* beta, float eps, void* q, int64_t ldq,
                            void* scales, int64_t lds, int64_t M, int64_t K, int in_dtype, void* stream) {
  if (!x || !q || !scales || ((gamma == nullptr) != (beta == nullptr))) return PM_E_NULL;
  const bool ln = gamma != nullptr;
  if (in_dtype != PM_F16 && in_dtype != PM_BF16 && in_dtype != PM_F32) return PM_E_DTYPE;
  const int64_t amask = in_dtype == PM_F32 ? 3 : 7;
  if (M < 1 || K < 32 || (K & 31) || K > (1 << 24) || ldx < K || (ldx & amask) || ldq < K || (ldq & 7) || lds < K / 32 ||
      !aligned(x, 16) || !aligned(q, 8) || M > (int64_t)1 << 30)
    return PM_E_SHAPE;
  if (ln && (in_dtype != PM_F32 || K > QMAX_IT * 512 || !aligned(gamma, 16) || !aligned(beta, 16))) return PM_E_SHAPE;
  const dim3 grid((unsigned)((M + 3) / 4));
  const hipStream_t st = (hipStream_t)stream;
  uint8_t* qo = static_cast<uint8_t*>(q);
  uint8_t* so = static_cast<uint8_t*>(scales);
  if (ln) {
    hipLaunchKernelGGL((mx8_quant_kernel<float, true>), grid, dim3(256), 0, st, (const float*)x, ldx, gamma, beta, eps, qo, ldq,
                       so, lds, (int)M, (int)K);
  } else if (in_dtype == PM_F32) {
    hipLaunchKernelGGL((mx8_quant_kernel<float, false>), grid, dim3(256), 0, st, (const float*)x, ldx, nullptr, nullptr, 0.f,
                       qo, ldq, so, lds, (int)M, (int)K);
  } else if (in_dtype == PM_F16) {
    hipLaunchKernelGGL((mx8_quant_kernel<f16, false>), grid, dim3(256), 0, st, (const f16*)x, ldx, nullptr, nullptr, 0.f, qo,
                       ldq, so, lds, (int)M, (int)K);
  } else {
    hipLaunchKernelGGL((mx8_quant_kernel<bf16, false>), grid, dim3(256), 0, st, (const bf16*)x, ldx, nullptr, nullptr, 0.f, qo,
                       ldq, so, lds, (int)M, (int)K);
  }
  return check_launch();
}

extern "C" int pm_gemm_mx8(const void* Aq, int64_t lda, const void* As, int64_t ldas, const void* Wq, int64_t ldw, const void* Ws,
                           int64_t ldws, const float* bias, const void* residual, int64_t ldr, void* C, int64_t ldc, void* Cs,
                           int64_t ldcs, int64_t M, int64_t N, int64_t K, int act, int flags, int dtype, void* stream) {
  if (!Aq || !As || !Wq || !Ws || !C) return PM_E_NULL;
  const bool mx_out = (dtype & PM_OUT_MX8) != 0;
  const int dt = dtype & ~PM_OUT_MX8;
  if (dt & ~0xff) return PM_E_SHAPE;  // (PM_OUT_HILO and any other output mode)
  if (dt != PM_F16 && dt != PM_BF16) return PM_E_DTYPE;
  const int known = PM_FLAG_OUT_F32 | PM_FLAG_RES_F32 | PM_FLAG_BIAS_IS_SCALE;
  if (flags & ~known) return PM_E_SHAPE;  // A_F32, A_LO, W_WRAP, STATS_I64 (and its instance count) are not served
  const bool out32 = flags & PM_FLAG_OUT_F32, res32 = flags & PM_FLAG_RES_F32, bmul = flags & PM_FLAG_BIAS_IS_SCALE;
  const bool geglu = act == PM_ACT_GEGLU;
  if (act != PM_ACT_NONE && !geglu) return PM_E_SHAPE;
  if (M < 1 || M > (int64_t)1 << 30 || N < 32 || (N & 31) || N > (1 << 24) || K < 64 || (K & 63) || K > (1 << 24))
    return PM_E_SHAPE;
  if (lda < K || ldw < K || (lda & 15) || (ldw & 15) || ldas < K / 32 || ldws < K / 32 || !aligned(Aq, 16) || !aligned(Wq, 16))
    return PM_E_SHAPE;
  if (bmul && (bias == nullptr || geglu)) return PM_E_SHAPE;
  if (mx_out && (!geglu || Cs == nullptr)) return mx_out && Cs == nullptr ? PM_E_NULL : PM_E_SHAPE;
  if (geglu && ((N & 63) || out32 || res32 || residual != nullptr)) return PM_E_SHAPE;
  if (out32 && res32) return PM_E_SHAPE;
  if (res32 && residual == nullptr) return PM_E_SHAPE;
  const int64_t nout = geglu ? N / 2 : N;
  if (ldc < nout || (ldc & 3) || (bias != nullptr && !aligned(bias, 16))) return PM_E_SHAPE;
  if (mx_out && (ldcs < nout / 32 || !aligned(C, 4))) return PM_E_SHAPE;
  if (!mx_out && !aligned(C, out32 ? 16 : 8)) return PM_E_SHAPE;
  if (residual != nullptr && (ldr < N || (ldr & 3) || !aligned(residual, (out32 || res32) ? 16 : 8))) return PM_E_SHAPE;
  Mx8Params p;
  p.A = static_cast<const uint8_t*>(Aq);
  p.lda = lda;
  p.As = static_cast<const uint8_t*>(As);
  p.ldas = ldas;
  p.W = static_cast<const uint8_t*>(Wq);
  p.ldw = ldw;
  p.Ws = static_cast<const uint8_t*>(Ws);
  p.ldws = ldws;
  p.bias = bias;
  p.R = residual;
  p.ldr = ldr;
  p.C = C;
  p.ldc = ldc;
  p.Cs = static_cast<uint8_t*>(Cs);
  p.ldcs = ldcs;
  p.M = (int)M;
  p.N = (int)N;
  p.K = (int)K;
  p.bias_mul = bmul;
  p.res32 = out32 || res32;
  p.mtiles = (int)((M + MX_BM - 1) / MX_BM);
  p.ntiles = (int)((N + MX_BN - 1) / MX_BN);
  if ((int64_t)p.mtiles * p.ntiles > 0x7fffffff) return PM_E_SHAPE;
  const dim3 grid((unsigned)(p.mtiles * p.ntiles));
  const hipStream_t st = (hipStream_t)stream;
  PM_DISPATCH_DTYPE(dt, T, {
    if (mx_out)
      hipLaunchKernelGGL((gemm_mx8_kernel<T, MX_EPI_GEGLU_MX>), grid, dim3(256), 0, st, p);
    else if (geglu)
      hipLaunchKernelGGL((gemm_mx8_kernel<T, MX_EPI_GEGLU>), grid, dim3(256), 0, st, p);
    else if (out32)
      hipLaunchKernelGGL((gemm_mx8_kernel<T, MX_EPI_F32>), grid, dim3(256), 0, st, p);
    else
      hipLaunchKernelGGL((gemm_mx8_kernel<T, MX_EPI_16>), grid, dim3(256), 0, st, p);
  });
  return check_launch();
}

extern "C" int pm_gemm_mx8_qkv_fp8(const void* Aq, int64_t lda, const void* As, int64_t ldas, const void* Wq, int64_t ldw,
                                   const void* Ws, int64_t ldws, const float* bias, void* q8, void* k8, void* v8t, int64_t M,
                                   int64_t K, int64_t heads, int64_t P, float qmul, int flags, void* stream) {
  if (!Aq || !As || !Wq || !Ws || !q8 || !k8 || !v8t) return PM_E_NULL;
  if (flags & ~PM_FLAG_BIAS_IS_SCALE) return PM_E_SHAPE;
  const bool bmul = flags & PM_FLAG_BIAS_IS_SCALE;
  if (bmul && bias == nullptr) return PM_E_SHAPE;
  if (heads < 1 || heads > 4096 || P < 64 || (P & 63) || M < P || M % P || M > (int64_t)1 << 30 || K < 64 || (K & 63) ||
      K > (1 << 24))
    return PM_E_SHAPE;
  const int64_t N = 3 * heads * 64;
  if (lda < K || ldw < K || (lda & 15) || (ldw & 15) || ldas < K / 32 || ldws < K / 32 || !aligned(Aq, 16) || !aligned(Wq, 16))
    return PM_E_SHAPE;
  if (!aligned(q8, 16) || !aligned(k8, 16) || !aligned(v8t, 16) || (bias != nullptr && !aligned(bias, 16))) return PM_E_SHAPE;
  Mx8Params p{};
  p.A = static_cast<const uint8_t*>(Aq);
  p.lda = lda;
  p.As = static_cast<const uint8_t*>(As);
  p.ldas = ldas;
  p.W = static_cast<const uint8_t*>(Wq);
  p.ldw = ldw;
  p.Ws = static_cast<const uint8_t*>(Ws);
  p.ldws = ldws;
  p.bias = bias;
  p.M = (int)M;
  p.N = (int)N;
  p.K = (int)K;
  p.bias_mul = bmul;
  p.mtiles = (int)((M + MX_BM - 1) / MX_BM);
  p.ntiles = (int)((N + MX_BN - 1) / MX_BN);
  p.q8 = static_cast<uint8_t*>(q8);
  p.k8 = static_cast<uint8_t*>(k8);
  p.v8t = static_cast<uint8_t*>(v8t);
  p.heads = (int)heads;
  p.P = (int)P;
  p.qmul = qmul;
  if ((int64_t)p.mtiles * p.ntiles > 0x7fffffff) return PM_E_SHAPE;
  hipLaunchKernelGGL((gemm_mx8_kernel<f16, MX_EPI_QKV8>), dim3((unsigned)(p.mtiles * p.ntiles)), dim3(256), 0, (hipStream_t)stream,
                     p);  // (the element type parameter is unused by this flavour)
  return check_launch();
}

// ---- pm_conv2d_3x3_mx8 / pm_conv_temporal_k3_mx8: the conv A-loader modes of gemm_mx8_kernel, MX_EPI_F32 epilogue only --------
// (the element type parameter is unused by that flavour with an f32 residual: one instance per loader)
template <int LD>
static int conv_mx8(Mx8Params& p, const void* Aq, int64_t lda, const void* As, int64_t ldas, const void* Wq, const void* Ws,
                    const float* bias, const void* residual, int64_t ldr, void* C, int64_t ldc, int64_t M, int64_t taps,
                    int64_t Cin, int64_t Cout, int act, int flags, int dtype, void* stream) {
  if (!Aq || !As || !Wq || !Ws || !C) return PM_E_NULL;
  if (dtype & ~0xff) return PM_E_SHAPE;  // (PM_OUT_HILO, PM_OUT_MX8 and any other output mode)
  if (dtype != PM_F16 && dtype != PM_BF16) return PM_E_DTYPE;
  // f32 output onto an optional f32 residual and nothing else: 16-bit output, a column scale, statistics flags (and their instance
  // count), f32 / [hi | lo] A operands are not served
  if (flags != PM_FLAG_OUT_F32 || act != PM_ACT_NONE) return PM_E_SHAPE;
  const int64_t K = taps * Cin;
  if (M < 1 || M > (int64_t)1 << 30 || Cout < 32 || (Cout & 31) || Cout > (1 << 24) || Cin < 32 || (Cin & 31) || K > (1 << 24))
    return PM_E_SHAPE;
  if (lda < Cin || (lda & 15) || ldas < Cin / 32 || !aligned(Aq, 16) || !aligned(Wq, 16)) return PM_E_SHAPE;
  if (ldc < Cout || (ldc & 3) || !aligned(C, 16) || (bias != nullptr && !aligned(bias, 16))) return PM_E_SHAPE;
  if (residual != nullptr && (ldr < Cout || (ldr & 3) || !aligned(residual, 16))) return PM_E_SHAPE;
  p.A = static_cast<const uint8_t*>(Aq);
  p.lda = lda;
  p.As = static_cast<const uint8_t*>(As);
  p.ldas = ldas;
  p.W = static_cast<const uint8_t*>(Wq);  // packed [Cout, taps * Cin], tap-major, contiguous; scales [Cout, taps * Cin / 32]
  p.ldw = K;
  p.Ws = static_cast<const uint8_t*>(Ws);
  p.ldws = K / 32;
  p.bias = bias;
  p.R = residual;
  p.ldr = ldr;
  p.C = C;
  p.ldc = ldc;
  p.M = (int)M;
  p.N = (int)Cout;
  p.K = (int)K;
  p.res32 = 1;
  p.cin = (int)Cin;
  p.mtiles = (int)((M + MX_BM - 1) / MX_BM);
  p.ntiles = (int)((Cout + MX_BN - 1) / MX_BN);
  if ((int64_t)p.mtiles * p.ntiles > 0x7fffffff) return PM_E_SHAPE;
  hipLaunchKernelGGL((gemm_mx8_kernel<f16, MX_EPI_F32, LD>), dim3((unsigned)(p.mtiles * p.ntiles)), dim3(256), 0,
                     (hipStream_t)stream, p);
  return check_launch();
}

extern "C" int pm_conv2d_3x3_mx8(const void* Aq, int64_t lda, const void* As, int64_t ldas, const void* Wq, const void* Ws,
                                 const float* bias, const void* residual, int64_t ldr, void* C, int64_t ldc, int64_t F, int64_t H,
                                 int64_t W, int64_t Cin, int64_t Cout, int stride, int upsample2x, int pad_lo, int act, int flags,
                                 int dtype, void* stream) {
  if (stride != 1 || upsample2x || pad_lo != 1) return PM_E_SHAPE;  // the fast mode of pm_conv2d_3x3 only
  if (F < 1 || H < 1 || W < 1 || H > (1 << 30) || W > (1 << 30) || F > (1 << 30) || H * W > (int64_t)1 << 30) return PM_E_SHAPE;
  Mx8Params p{};
  p.fh = (int)H;
  p.fw = (int)W;
  return conv_mx8<MX_LD_C3>(p, Aq, lda, As, ldas, Wq, Ws, bias, residual, ldr, C, ldc, F * H * W, 9, Cin, Cout, act, flags, dtype,
                            stream);
}

extern "C" int pm_conv_temporal_k3_mx8(const void* Aq, int64_t lda, const void* As, int64_t ldas, const void* Wq, const void* Ws,
                                       const float* bias, const void* residual, int64_t ldr, void* C, int64_t ldc, int64_t F,
                                       int64_t clip_frames, int64_t P, int64_t Cin, int64_t Cout, int act, int flags, int dtype,
                                       void* stream) {
  if (F < 1 || P < 1 || F > (1 << 30) || P > (1 << 30) || clip_frames < 1 || F % clip_frames) return PM_E_SHAPE;
  Mx8Params p{};
  p.px = (int)P;
  p.clip = (int)clip_frames;
  return conv_mx8<MX_LD_T3>(p, Aq, lda, As, ldas, Wq, Ws, bias, residual, ldr, C, ldc, F * P, 3, Cin, Cout, act, flags, dtype,
                            stream);
}
