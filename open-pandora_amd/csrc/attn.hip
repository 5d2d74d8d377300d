// Host side of the attention kernels: the diagnostics variant override, the extern "C" entry points and the launchers.
// The kernels live in the headers below (one translation unit); attn_self16_kernel is its own unit, attn16.hip.
#include "attn_cross.hpp"
#include "attn_self.hpp"
#include "attn_fp8.hpp"
#include "attn_temporal.hpp"
#include "attn_small.hpp"
using namespace pm;

// Kernel selection override for A/B measurements (tools/attn_bench.py) - ONLY in the -DPM_DIAG build
// (libpandora_mi355x_diag.so, include/pandora_mi355x_diag.h): the shipped library always runs the production kernels,
// holds no mutable global and instantiates none of the older variants / ceiling probes.
#ifdef PM_DIAG
static int g_attn_variant = -1;
static int attn_variant() {
  if (g_attn_variant < 0) {
    const char* e = diag_env("PANDORA_ATTN_VARIANT");
    g_attn_variant = e ? atoi(e) : 0;
  }
  return g_attn_variant;
}
extern "C" void pm_debug_attn_variant(int v) { g_attn_variant = v < 0 ? 0 : v; }
static unsigned long long* g_attn_stamps = nullptr;
extern "C" void pm_debug_attn_stamps(void* buf) { g_attn_stamps = reinterpret_cast<unsigned long long*>(buf); }
#else
static constexpr int attn_variant() { return 0; }
#endif

constexpr float LOG2E = 1.4426950408889634f;  // scores are kept in the base-2 domain: exp2(s * scale * log2(e))

// attn_self_kernel<T, QB, PIPE, POST, RING, PROBE> for the call's element type
template <int QB, bool PIPE, bool POST, int RING, int PROBE = 0>
static int launch_attn_self(const AttnParams& p, int dtype, dim3 grid, hipStream_t stream) {
  PM_DISPATCH_DTYPE(dtype, T, hipLaunchKernelGGL((attn_self_kernel<T, QB, PIPE, POST, RING, PROBE>), grid, dim3(256), 0, stream, p);
                    return check_launch());
}

extern "C" int pm_attention(const void* q, int64_t q_bs, int64_t q_rs, const void* k1,
                            const void* v1, int64_t k1_bs, int64_t k1_rs, int64_t Nk1,
                            const void* k2, const void* v2, int64_t k2_bs, int64_t k2_rs,
                            int64_t Nk2, float w2, void* o, int64_t o_bs, int64_t o_rs, int64_t B,
                            int64_t heads, int64_t Nq, float scale, int dtype, void* stream) {
  if (!q || !k1 || !v1 || !o) return PM_E_NULL;
  if (k2 && !v2) return PM_E_NULL;
  if (B < 1 || heads < 1 || Nq < 1 || Nk1 < 1 || (k2 && Nk2 < 1)) return PM_E_SHAPE;
  if ((q_bs | q_rs | k1_bs | k1_rs | o_bs | o_rs) & 7) return PM_E_SHAPE;
  if (k2 && ((k2_bs | k2_rs) & 7)) return PM_E_SHAPE;
  if (Nk1 * k1_rs * 2 >= (1ll << 32) || (k2 && Nk2 * k2_rs * 2 >= (1ll << 32))) return PM_E_SHAPE;  // 32-bit lane byte offsets
  if (B * heads * ((Nq + 127) / 128) > (1ll << 30)) return PM_E_SHAPE;
  AttnParams p{};
  p.q = q; p.o = o; p.q_bs = q_bs; p.q_rs = q_rs; p.o_bs = o_bs; p.o_rs = o_rs;
  p.k[0] = k1; p.v[0] = v1; p.k_bs[0] = k1_bs; p.k_rs[0] = k1_rs; p.Nk[0] = (int)Nk1; p.w[0] = 1.f;
  p.k[1] = k2; p.v[1] = v2; p.k_bs[1] = k2_bs; p.k_rs[1] = k2_rs; p.Nk[1] = (int)Nk2; p.w[1] = w2;
  p.nseg = k2 ? 2 : 1;
  p.Nq = (int)Nq; p.heads = (int)heads;
  p.scale_log2e = scale * LOG2E;
  p.prescaled = fabsf(p.scale_log2e - 1.0f) < 1e-6f ? 1 : 0;
  if (k2) {
    p.nqt = (int)((Nq + 127) / 128);
    dim3 grid((unsigned)(p.nqt * B * heads));
    PM_DISPATCH_DTYPE(dtype, T,
                      hipLaunchKernelGGL((attn_kernel<T, 1, true>), grid, dim3(256), 0, (hipStream_t)stream, p);
                      return check_launch());
  }
  // single segment: 32 query rows per wave (128 per workgroup), double-buffered K/V, three workgroups per CU.
  // Measured on the U-Net's shapes (tools/attn_bench.py, interleaved A/B in one process, random data): this is
  // the fastest at every N (1020-1035 TF/s at N = 9216).  The 64-rows-per-wave forms (variants 3 / 5: half the
  // LDS fragment reads per MFMA, a 4-stage K/V ring, 2.0 GHz instead of 1.75) lose 1-3 % there and more on
  // short sequences; kept for A/B runs.
  const int variant = attn_variant();
#ifdef PM_DIAG
  p.stamps = g_attn_stamps;
#endif
  const bool qb2 = variant == 3 || variant == 5;
  const int rows = qb2 ? 256 : 128;
  p.nqt = (int)((Nq + rows - 1) / rows);
  dim3 grid((unsigned)(p.nqt * B * heads));
#ifdef PM_DIAG
  // 16 forces the 16x16x32-MFMA form (attn16.hip); 17 / 18 / 19: its forms 1 / 2 / 3 (per-lane K/V addresses, row sums on the
  // vector pipe, hipcc's own PV issue order)
  if (variant >= 16 && variant <= 19) return launch_attn_self16(p, dtype, grid, (hipStream_t)stream, variant - 16);
  if (variant == 9)  // (kept for A/B runs: the round-1 kernel)
    PM_DISPATCH_DTYPE(dtype, T,
                      hipLaunchKernelGGL((attn_kernel<T, 1, false>), grid, dim3(256), 0, (hipStream_t)stream, p);
                      return check_launch());
  if (variant == 3) return launch_attn_self<2, true, false, 4>(p, dtype, grid, (hipStream_t)stream);
  if (variant == 5) return launch_attn_self<2, true, true, 4>(p, dtype, grid, (hipStream_t)stream);
  // ceiling probes (diagnosis: the output is not an attention result)
  if (variant == 11) return launch_attn_self<1, false, false, 2, 1>(p, dtype, grid, (hipStream_t)stream);
  if (variant == 12) return launch_attn_self<1, false, false, 2, 2>(p, dtype, grid, (hipStream_t)stream);
  if (variant == 13) return launch_attn_self<1, false, false, 2, 3>(p, dtype, grid, (hipStream_t)stream);
  if (variant == 1) return launch_attn_self<1, false, false, 2>(p, dtype, grid, (hipStream_t)stream);  // force the 32x32x16 form
#endif
  // long sequences: the 16x16x32-MFMA form (csrc/attn16.hip: +1-2 % by wall at N = 9216, +-1 % around 2304-2560 - the chip holds a ~11 % higher clock
  // under that shape, profiles/r04/attention_shapes.txt); shorter ones: the 32x32x16 form (fewer, longer MFMAs per tile)
  if (Nq >= 4096 && Nk1 >= 4096) return launch_attn_self16(p, dtype, grid, (hipStream_t)stream);
  return launch_attn_self<1, false, false, 2>(p, dtype, grid, (hipStream_t)stream);
}

static int64_t pad64(int64_t n) { return (n + 63) / 64 * 64; }

extern "C" size_t pm_attention_fp8_workspace_bytes(int64_t B, int64_t heads, int64_t Nq, int64_t Nk) {
  return (size_t)(B * heads * 64 * (pad64(Nq) + 2 * pad64(Nk)));
}

// the packed operands [B*heads][pad64(N)][64] (v8t: [B*heads][64][pad64(Nk)]) and the output of one call
// (o_bs / o_rs in elements for a 16-bit output, in bytes for the MXFP8 output, whose caller adds the scale fields)
static AttnFp8Params fp8_params(const void* q8, const void* k8, const void* v8t, void* o, int64_t o_bs, int64_t o_rs,
                                int64_t heads, int64_t Nq, int64_t Nk) {
  AttnFp8Params p{};
  p.q8 = static_cast<const unsigned char*>(q8); p.k8 = static_cast<const unsigned char*>(k8);
  p.v8t = static_cast<const unsigned char*>(v8t); p.o = o; p.o_bs = o_bs; p.o_rs = o_rs;
  p.Nq = (int)Nq; p.Nk = (int)Nk; p.Nq_pad = (int)pad64(Nq); p.Nk_pad = (int)pad64(Nk); p.heads = (int)heads;
  return p;
}

// attn_fp8_kernel on packed operands (p.q8 / k8 / v8t / o / os and the sizes filled in); dtype may carry PM_OUT_MX8
static int launch_attn_fp8(AttnFp8Params p, int64_t B, int dtype, hipStream_t stream) {
#ifdef PM_DIAG
  const bool qb2 = attn_variant() == 2 && !(dtype & PM_OUT_MX8);  // (32 rows per wave measured faster at every N: tools/attn_bench.py 101 / 102)
#else
  constexpr bool qb2 = false;
#endif
  const int rows = qb2 ? 256 : 128;
  p.nqt = (int)((p.Nq + rows - 1) / rows);
  dim3 grid((unsigned)(p.nqt * B * p.heads));
  if (dtype & PM_OUT_MX8) {
    hipLaunchKernelGGL((attn_fp8_kernel<f16, 1, true>), grid, dim3(256), 0, stream, p);  // (the element type is unused)
    return check_launch();
  }
  PM_DISPATCH_DTYPE(dtype, T,
                    if constexpr (PM_DIAG_BUILD) {
                      if (qb2) {
                        hipLaunchKernelGGL((attn_fp8_kernel<T, PM_DIAG_BUILD ? 2 : 1>), grid, dim3(256), 0, stream, p);
                        return check_launch();
                      }
                    }
                    hipLaunchKernelGGL((attn_fp8_kernel<T, 1>), grid, dim3(256), 0, stream, p);
                    return check_launch());
}

extern "C" int pm_attention_fp8_packed(const void* q8, const void* k8, const void* v8t, int64_t Nq, int64_t Nk, void* o,
                                       int64_t o_bs, int64_t o_rs, void* os, int64_t os_bs, int64_t os_rs, int64_t B,
                                       int64_t heads, int dtype, void* stream) {
  if (!q8 || !k8 || !v8t || !o) return PM_E_NULL;
  const bool mx_out = (dtype & PM_OUT_MX8) != 0;
  const int dt = dtype & ~PM_OUT_MX8;
  if (dt & ~0xff) return PM_E_SHAPE;
  if (dt != PM_F16 && dt != PM_BF16) return PM_E_DTYPE;
  if (mx_out && !os) return PM_E_NULL;
  if (B < 1 || heads < 1 || Nq < 1 || Nk < 1) return PM_E_SHAPE;
  if (mx_out ? (((o_bs | o_rs) & 3) || o_rs < heads * 64 || os_rs < heads * 2 || (reinterpret_cast<uintptr_t>(o) & 3))
             : (((o_bs | o_rs) & 7) != 0))
    return PM_E_SHAPE;
  if ((reinterpret_cast<uintptr_t>(q8) | reinterpret_cast<uintptr_t>(k8) | reinterpret_cast<uintptr_t>(v8t)) & 15) return PM_E_SHAPE;
  if (pad64(Nk) * 64 >= (1ll << 31) || pad64(Nq) * 64 >= (1ll << 31) || B * heads > 65535) return PM_E_SHAPE;
  AttnFp8Params p = fp8_params(q8, k8, v8t, o, o_bs, o_rs, heads, Nq, Nk);
  p.os = static_cast<unsigned char*>(os); p.os_bs = os_bs; p.os_rs = os_rs;
  return launch_attn_fp8(p, B, dtype, (hipStream_t)stream);
}

extern "C" int pm_attention_fp8(const void* q, int64_t q_bs, int64_t q_rs, const void* k, const void* v,
                                int64_t k_bs, int64_t k_rs, int64_t Nk, void* o, int64_t o_bs, int64_t o_rs,
                                int64_t B, int64_t heads, int64_t Nq, float scale, int dtype, void* workspace,
                                size_t workspace_bytes, void* stream) {
  if (!q || !k || !v || !o || !workspace) return PM_E_NULL;
  if (B < 1 || heads < 1 || Nq < 1 || Nk < 1) return PM_E_SHAPE;
  if ((q_bs | q_rs | k_bs | k_rs | o_bs | o_rs) & 7) return PM_E_SHAPE;
  if (workspace_bytes < pm_attention_fp8_workspace_bytes(B, heads, Nq, Nk)) return PM_E_WORKSPACE;
  const int64_t nq = pad64(Nq), nk = pad64(Nk);
  if (nk * 64 >= (1ll << 31) || B * heads > 65535) return PM_E_SHAPE;
  if (dtype != PM_F16 && dtype != PM_BF16) return PM_E_DTYPE;
  unsigned char* ws = reinterpret_cast<unsigned char*>(workspace);
  AttnFp8PackParams pp{};
  pp.q = q; pp.k = k; pp.v = v; pp.q_bs = q_bs; pp.q_rs = q_rs; pp.k_bs = k_bs; pp.k_rs = k_rs;
  pp.q8 = ws; pp.k8 = ws + B * heads * nq * 64; pp.v8t = pp.k8 + B * heads * nk * 64;
  pp.Nq = (int)Nq; pp.Nk = (int)Nk; pp.Nq_pad = (int)nq; pp.Nk_pad = (int)nk; pp.heads = (int)heads;
  pp.ntq = (int)(nq / 64);
  pp.qscale = scale * LOG2E;  // scores in the base-2 domain
  dim3 pgrid((unsigned)(nq / 64 + nk / 64), (unsigned)(B * heads));
  const AttnFp8Params p = fp8_params(pp.q8, pp.k8, pp.v8t, o, o_bs, o_rs, heads, Nq, Nk);
  // pack + the packed-operand kernel (what pm_attention_fp8_packed launches)
  PM_DISPATCH_DTYPE(dtype, T,
                    hipLaunchKernelGGL((attn_fp8_pack_kernel<T>), pgrid, dim3(256), 0, (hipStream_t)stream, pp));
  return launch_attn_fp8(p, B, dtype, (hipStream_t)stream);
}

// pm_attention_generic and pm_attention_causal: one parameter block, one grid, the kernel's CAUSAL flag apart
static int launch_attn_small(const void* q, int64_t q_bs, int64_t q_rs, const void* k, const void* v, int64_t k_bs,
                             int64_t k_rs, int64_t Nk, void* o, int64_t o_bs, int64_t o_rs, int64_t B, int64_t heads,
                             int64_t Nq, int64_t D, float scale, int dtype, bool causal, int64_t q_pos0, void* stream) {
  if (!q || !k || !v || !o) return PM_E_NULL;
  if (B < 1 || heads < 1 || Nq < 1 || Nk < 1 || Nk > 1024 || D < 8 || D > 128 || (D & 7)) return PM_E_SHAPE;
  if ((q_bs | q_rs | k_bs | k_rs | o_bs | o_rs) & 7) return PM_E_SHAPE;
  if (B * heads > 65535) return PM_E_SHAPE;
  if (causal && (q_pos0 < 0 || q_pos0 > Nk - Nq)) return PM_E_SHAPE;
  AttnSmallParams p{};
  p.q = q; p.k = k; p.v = v; p.o = o; p.q_bs = q_bs; p.q_rs = q_rs; p.k_bs = k_bs; p.k_rs = k_rs;
  p.o_bs = o_bs; p.o_rs = o_rs; p.Nq = (int)Nq; p.Nk = (int)Nk; p.heads = (int)heads; p.D = (int)D; p.scale = scale;
  p.q_pos0 = (int)q_pos0;
  dim3 grid((unsigned)((Nq + 3) / 4), (unsigned)(B * heads));
  if (causal) {
    PM_DISPATCH_DTYPE(dtype, T,
                      hipLaunchKernelGGL((attn_small_kernel<T, true>), grid, dim3(256), 0, (hipStream_t)stream, p);
                      return check_launch());
  }
  PM_DISPATCH_DTYPE(dtype, T,
                    hipLaunchKernelGGL((attn_small_kernel<T, false>), grid, dim3(256), 0, (hipStream_t)stream, p);
                    return check_launch());
}

extern "C" int pm_attention_generic(const void* q, int64_t q_bs, int64_t q_rs, const void* k, const void* v,
                                    int64_t k_bs, int64_t k_rs, int64_t Nk, void* o, int64_t o_bs, int64_t o_rs,
                                    int64_t B, int64_t heads, int64_t Nq, int64_t D, float scale, int dtype,
                                    void* stream) {
  return launch_attn_small(q, q_bs, q_rs, k, v, k_bs, k_rs, Nk, o, o_bs, o_rs, B, heads, Nq, D, scale, dtype, false, 0, stream);
}

extern "C" int pm_attention_causal(const void* q, int64_t q_bs, int64_t q_rs, const void* k, const void* v,
                                   int64_t k_bs, int64_t k_rs, int64_t Nk, void* o, int64_t o_bs, int64_t o_rs,
                                   int64_t B, int64_t heads, int64_t Nq, int64_t D, float scale, int dtype,
                                   int64_t q_pos0, void* stream) {
  return launch_attn_small(q, q_bs, q_rs, k, v, k_bs, k_rs, Nk, o, o_bs, o_rs, B, heads, Nq, D, scale, dtype, true, q_pos0, stream);
}

extern "C" int pm_attention_temporal(const void* q, int64_t ldq, const void* k, const void* v,
                                     int64_t ldk, void* o, int64_t ldo, int64_t Fq, int64_t Fk,
                                     int64_t P, int64_t heads, float scale, int dtype,
                                     void* stream) {
  if (!q || !k || !v || !o) return PM_E_NULL;
  if (Fq < 1 || Fk < 1 || Fk > 16 || P < 1 || heads < 1) return PM_E_SHAPE;
  if ((ldq | ldk | ldo) & 7) return PM_E_SHAPE;
  TAttnParams p{};
  p.q = q; p.k = k; p.v = v; p.o = o; p.ldq = ldq; p.ldk = ldk; p.ldo = ldo;
  p.Fq = (int)Fq; p.Fk = (int)Fk; p.P = (int)P; p.heads = (int)heads;
  p.scale_log2e = scale * LOG2E;
  if (Fq > 16 || P * heads > (1ll << 30)) return PM_E_SHAPE;
  p.nprob = (int)(P * heads);
  int64_t nb = (p.nprob + 3) / 4;  // 4 waves per block; cap the grid and loop (8 waves/SIMD resident)
  if (nb > 256 * 8) nb = 256 * 8;
  dim3 grid((unsigned)nb);
  PM_DISPATCH_DTYPE(dtype, T,
                    hipLaunchKernelGGL((tattn_kernel<T>), grid, dim3(256), 0, (hipStream_t)stream, p);
                    return check_launch());
}
