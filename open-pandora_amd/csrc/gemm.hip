// Host side of the MFMA GEMM family for gfx950: process state, the split-K plan, the ONE kernel choice (choose_kernel),
// the launchers and the C entry points pm_gemm / pm_conv2d_3x3 / pm_conv_temporal_k3*.  The kernels of this translation
// unit live in gemm_2stage.hpp (128x128, two LDS stages: any shape), gemm_ring.hpp (128x128 and 256x128 ring kernels)
// and gemm_splitk_reduce.hpp; gemm_wide.hip and gemm_wide_stream.hip are units of their own.
#include "gemm_common.hpp"
#include "gemm_2stage.hpp"
#include "gemm_ring.hpp"
#include "gemm_splitk_reduce.hpp"

namespace pm {

// Process-level state of this file, all of it write-once: the environment overrides read by init_once() before
// their first use (from EVERY entry point that depends on them, so a sizing query and the launch it sizes agree).
// The per-device caches (CU count, dynamic LDS limit) are common.hpp's num_cus() / raise_dynamic_lds().
static int g_ring = 1;  // PANDORA_GEMM_RING: 0 = never, 1 = by prefer_ring(), 2 = always
static int g_ringw = 1;  // PANDORA_GEMM_RINGW: 0 = never, 1 = by prefer_ringw(), 2 (with PANDORA_GEMM_RING=2) = every unsplit 16-bit call
static int g_natural = 1;          // PANDORA_GEMM_NATURAL (diagnostics build): 0 = interleaved W rows for the f32 flavours too (A/B)
static int g_split_min_nk = 24;     // PANDORA_SPLITK_MIN_NK: shortest K loop (in 64-wide tiles) that is split
static int g_split_max_tiles = 384; // PANDORA_SPLITK_MAX_TILES: grids of at least this many tiles never split
static int g_split_force = 0;       // PANDORA_SPLITK_FORCE = s > 0: every splittable call takes (up to) s slices (sweeps that fit the model)

#ifdef PM_RING_PROF
static long long* g_ring_prof = nullptr;  // RingStamps' destination (tools/ring_prof.py)
extern "C" void pm_debug_ring_prof(void* buf) { g_ring_prof = reinterpret_cast<long long*>(buf); }
#endif

static void init_once() {
  static const bool init = [] {
    const char* m = diag_env("PANDORA_SPLITK_MIN_NK");
    if (m) g_split_min_nk = atoi(m);
    const char* mt = diag_env("PANDORA_SPLITK_MAX_TILES");
    if (mt) g_split_max_tiles = atoi(mt);
    const char* rwe = diag_env("PANDORA_GEMM_RINGW");
    if (rwe) g_ringw = atoi(rwe);
    const char* r = diag_env("PANDORA_GEMM_RING");
    if (r) g_ring = atoi(r);
    const char* sf = diag_env("PANDORA_SPLITK_FORCE");
    if (sf) g_split_force = atoi(sf);
    const char* nl = diag_env("PANDORA_GEMM_NATURAL");
    if (nl) g_natural = atoi(nl);
    return true;
  }();
  (void)init;
}

// Split-K plan of a call shape.  Few-tile grids (the deep U-Net levels) can cut their K loop over several
// workgroups, but the slabs cost a second pass: s partial [M, N] f32 slabs written by the main kernel, read by
// the reduce launch.  The old rule (aim at 512 work items) split 200-tile grids three ways - 600 items run in
// three rounds of one workgroup per CU, no shorter than the unsplit round, plus the reduce: the temporal convs at
// M = 2560 ran 64 us against 42 unsplit - and cut 50-tile grids 11 ways where 5 fill the chip once.  Now: the s
// that minimises  rounds(s) x (K-steps per slice x t_step + t_fixed) + reduce(s)  with the ring kernel's measured
// step (0.55 us per 64-wide K-step per workgroup, ~2 us of prologue + epilogue per round) and the slabs' HBM time.
static int choose_splits(int64_t M, int64_t N, int64_t K, int act, int* ktps, bool two_stage = false) {
  init_once();
  const int64_t tiles = ((M + BM - 1) / BM) * ((N + BN - 1) / BN);
  const int nk = (int)((K + BK - 1) / BK);
  *ktps = nk;
  if (act == PM_ACT_GEGLU || tiles >= g_split_max_tiles || nk < g_split_min_nk) return 1;
  if (g_split_force > 0) {
    int s = g_split_force;
    if (s > nk / 4) s = nk / 4;
    if (s < 2) return 1;
    *ktps = (nk + s - 1) / s;
    return (nk + *ktps - 1) / *ktps;
  }
  // Work items run in rounds of one workgroup per CU on the ring kernel (0.55 us per K-step), of two per CU on the
  // 2-stage kernel, the only one the general 3x3 mode (nearest-x2 upsample) has (1.1 us per K-step per workgroup).
  // A slab is written and read once, mostly out of the 256 MiB Infinity Cache: ~9 TB/s.  Constants and the two
  // exceptions checked against a sweep of forced slice counts (PANDORA_SPLITK_FORCE = 1..10, both resolutions:
  // profiles/r02/splitk_forced_sweep.txt): the model's pick is within 3 % of the best forced count on every shape.
  const double slots = two_stage ? 512.0 : 256.0, t_step = two_stage ? 1.1 : 0.55, t_fixed = two_stage ? 3.0 : 2.0;
  const double slab_us = (double)M * (double)N * 8.0 / 9.0e6;
  int best_s = 1, best_ktps = nk;
  double best = 0.0;
  for (int s = 1; s <= 32 && s <= nk / 4; ++s) {
    const int kt = (nk + s - 1) / s, splits = (nk + kt - 1) / kt;
    if (s > 1 && splits != s) continue;  // (the same plan as a smaller s)
    const double rounds = (double)((tiles * splits + (int64_t)slots - 1) / (int64_t)slots);
    double cost = rounds * (kt * t_step + t_fixed) + (splits > 1 ? 2.5 + splits * slab_us : 0.0);
    if (splits == 1 && nk >= 256) cost *= 1.1;  // (very long unsplit loops measured ~10 % over the model: L2 window)
    if (s == 1 || cost < best * 0.97) {
      best = cost;
      best_s = splits;
      best_ktps = kt;
    }
  }
  *ktps = best_ktps;
  return best_s;
}

static void plan_split(GemmParams& p, void* workspace, size_t workspace_bytes, bool two_stage = false) {
  init_once();
  int ktps;
  // (a call with fused statistics keeps the plan pm_gemm_colstats_rows answers for: its colstats are sized by it)
  int s = choose_splits(p.M, p.N, p.K, p.act, &ktps, two_stage && p.colstats == nullptr);
  // fused statistics: from the main kernel's epilogue when the call runs unsplit (64-row blocks), from the
  // reduce pass when it splits (16-row blocks, pm_gemm_colstats_rows); the reduce variant needs 4-column vectors
  if (p.colstats != nullptr && s > 1 && ((p.N & 3) || p.act == PM_ACT_GEGLU)) {  // (pm_gemm_colstats_rows says 64 too)
    s = 1;
    ktps = (p.K + BK - 1) / BK;
  }
  if (s > 1 && (workspace == nullptr || workspace_bytes < (size_t)s * p.M * p.N * sizeof(float))) {
    s = 1;  // no (or too small a) workspace: run unsplit
    ktps = (p.K + BK - 1) / BK;
  }
  p.splits = s;
  p.ktps = ktps;
  p.ws = reinterpret_cast<float*>(workspace);
  // all-f32 epilogue (f32 output - its residual, if any, is f32 too - or split-K slabs) on the fast flavour's
  // preconditions: W rows staged in natural column order, 64 contiguous bytes per row and store / residual-load
  // instruction (gemm_common.hpp cperm)
  const int64_t ldc = s > 1 ? p.N : p.ldc;
  p.natural = (g_natural && p.act != PM_ACT_GEGLU && (p.out32 || s > 1) && (p.N & 31) == 0 && (ldc & 7) == 0 &&
               (p.R == nullptr || (p.ldr & 7) == 0)) ? 1 : 0;
}

template <typename T> static void launch_reduce(const GemmParams& p, hipStream_t stream) {
  // (the 16-row x 256-column block mapping is also the faster plain reduce whenever 4-column vectors apply)
  if (p.colstats != nullptr || ((p.N & 3) == 0 && (p.ldc & 3) == 0 && (p.R == nullptr || (p.ldr & 3) == 0))) {
    dim3 grid((unsigned)((p.M + 15) / 16), (unsigned)((p.N + 255) / 256));
    hipLaunchKernelGGL((splitk_reduce_stats_kernel<T>), grid, dim3(256), 0, stream, p);
    return;
  }
  const int64_t work = (int64_t)p.M * ((p.N + 3) / 4);
  int64_t nb = (work + 255) / 256;
  if (nb > 4096) nb = 4096;
  hipLaunchKernelGGL((splitk_reduce_kernel<T>), dim3((unsigned)nb), dim3(256), 0, stream, p);
}

template <typename T, int AMODE, bool A32> static int launch1(const GemmParams& p, hipStream_t stream) {
  constexpr int lds = 4 * TILE_BYTES;
  GemmParams q = p;
  q.mtiles = (p.M + BM - 1) / BM;
  const int64_t nwork = (int64_t)q.mtiles * p.ntiles * p.splits;
  // one work item per workgroup (persistent 2-stage workgroups measured: 2 per CU = no gain, 1 or 3 per CU 5 % slower)
  const int grid = (int)nwork;
  raise_dynamic_lds(reinterpret_cast<const void*>(gemm_kernel<T, AMODE, A32>), lds);
  hipLaunchKernelGGL((gemm_kernel<T, AMODE, A32>), dim3(grid), dim3(256), lds, stream, q);
  if (p.splits > 1) launch_reduce<T>(p, stream);
  return check_launch();
}

constexpr int RINGW_LDS = 3 * 3 * TILE_BYTES;  // three stages of (A 256 x 64 | W 128 x 64)
// 256-row tiles halve the tile count: only where that does not cost whole-round efficiency (measured per shape in the model:
// profiles/r03/ringw_ab.txt), unsplit, 16-bit operands, the dense / fast 3x3 / temporal loaders
static bool prefer_ringw(int amode, const GemmParams& p) {
  if (p.splits != 1 || p.K < 8 * BK) return false;  // (K = 320 .. 448: the 256x256 kernel / the 128x128 kernels measure better)
  const int64_t cu = num_cus();
  const int64_t n256 = (int64_t)((p.M + 255) / 256) * p.ntiles, n128 = (int64_t)((p.M + BM - 1) / BM) * p.ntiles;
  const double e256 = (double)n256 / (double)(((n256 + cu - 1) / cu) * cu) * ((double)p.M / (double)(((p.M + 255) / 256) * 256));
  const double e128 = (double)n128 / (double)(((n128 + cu - 1) / cu) * cu) * ((double)p.M / (double)(((p.M + BM - 1) / BM) * BM));
  return n256 >= cu * 3 / 4 && e256 >= e128 - 0.06;
}
template <typename T, int AMODE> static int launch_ringw(const GemmParams& p, hipStream_t stream) {
  GemmParams q = p;
#ifdef PM_RING_PROF
  q.prof = g_ring_prof;
#endif
  q.mtiles = (p.M + 255) / 256;
  const int64_t nwork = (int64_t)q.mtiles * p.ntiles;
  const int grid = (int)(nwork < num_cus() ? nwork : num_cus());
  raise_dynamic_lds(reinterpret_cast<const void*>(gemm_ringw_kernel<T, AMODE>), RINGW_LDS);
  hipLaunchKernelGGL((gemm_ringw_kernel<T, AMODE>), dim3(grid), dim3(512), RINGW_LDS, stream, q);
  return check_launch();
}

template <typename T, int AMODE> static int launch_ring(const GemmParams& p, hipStream_t stream) {
  GemmParams q = p;
#ifdef PM_RING_PROF
  q.prof = g_ring_prof;
#endif
  q.mtiles = (p.M + BM - 1) / BM;
  const int64_t nwork = (int64_t)q.mtiles * p.ntiles * p.splits;
  const int grid = (int)(nwork < num_cus() ? nwork : num_cus());
  raise_dynamic_lds(reinterpret_cast<const void*>(gemm_ring_kernel<T, AMODE>), RING_LDS);
  hipLaunchKernelGGL((gemm_ring_kernel<T, AMODE>), dim3(grid), dim3(512), RING_LDS, stream, q);
  if (p.splits > 1) launch_reduce<T>(p, stream);
  return check_launch();
}

// Which kernel for a 16-bit-operand call (measured per shape in the model, tools/shape_profile.py with
// PANDORA_GEMM_RING=0 / 2).  The ring kernel has the faster steady state (~700 vs ~950 cycles per K-step per
// CU) and hides the load round trip, but owns the CU alone: it pays for every epilogue with idle MFMA time and
// quantises the grid in rounds of 1 workgroup per CU, where the 2-stage kernel runs rounds of 2.
static bool prefer_ring(int amode, const GemmParams& p) {
  if (p.act == PM_ACT_GEGLU) return false;  // (in the model the 2-stage kernel is 6-10% faster on the GEGLU GEMMs)
  const int64_t nwork = (int64_t)((p.M + BM - 1) / BM) * p.ntiles * p.splits;
  const int64_t cu = num_cus();
  const double eff_ring = (double)nwork / (double)(((nwork + cu - 1) / cu) * cu);
  const double eff_two = (double)nwork / (double)(((nwork + 2 * cu - 1) / (2 * cu)) * 2 * cu);
  // (temporal convs: ties go to the ring kernel - 2-8 % faster at M = 10240 .. 147456, tools/shape_profile.py with
  // PANDORA_GEMM_RING=0/2, profiles/r02/kernel_choice_ab.txt)
  if (amode == A_CONVT3) return eff_ring + 0.05 >= eff_two || (nwork <= cu && nwork >= cu / 2);
  if (nwork <= cu) return true;  // one tile per CU: the 2-stage kernel would be round-trip-bound
  if (amode == A_CONV3X3_FAST) return eff_ring >= eff_two;  // long K loops: ties go to the faster steady state
  return (p.M <= 2560 && p.splits == 1) || eff_ring > eff_two + 0.05;
}

// The kernel families of pm_gemm / the convs.  The values are what pm_gemm_kernel_choice returns (bench.py, ops_hip.py and the tests
// compare against them).
// (2 was the retired 256x256 8-phase kernel: reserved, never returned)
enum KernelChoice { K_TWO_STAGE = 0, K_RING = 1, K_RINGW = 3, K_WIDE = 4, K_WIDE_STREAM = 5 };

// THE dispatch rule: which kernel runs a planned call (p after plan_split) with loader `amode`.  The launches and the
// pm_gemm_kernel_choice query both go through here.
static KernelChoice choose_kernel(const GemmParams& p, int flags, int amode) {
  init_once();
  if (flags & PM_FLAG_A_F32) return K_TWO_STAGE;  // f32 A is staged through registers: the 2-stage kernel alone
  const bool dense = amode == A_DENSE;            // (the conv loaders exist in the 2-stage and the two ring kernels only)
  // the 16-bit projection flavours on whole 256 x 256 tiles: the assembly kernel with the K stream continuous across tiles
  if (dense && gemm_wide_stream_wanted(p, flags, num_cus())) return K_WIDE_STREAM;
  // wide / long-K shapes whose grid keeps whole rounds of 256 x 256 tiles: four waves of 128 x 128, assembly main loop (gemm_wide.hip)
  if (dense && gemm_wide_wanted(p, flags, num_cus())) return K_WIDE;
  if (amode == A_CONV3X3) return K_TWO_STAGE;  // (general 3x3 mode: K tails / nearest-x2 stay on gemm_kernel)
  const bool force_ringw = g_ringw == 2 && g_ring == 2;  // every unsplit 16-bit call on the 256x128 ring kernel (tools/ring_prof.py --ringw)
  if (p.splits == 1 && (force_ringw || (g_ringw == 1 && g_ring != 0 && prefer_ringw(amode, p)))) return K_RINGW;
  return (g_ring == 2 || (g_ring == 1 && prefer_ring(amode, p))) ? K_RING : K_TWO_STAGE;
}

template <typename T, int AMODE> static int launch(const GemmParams& p, int flags, hipStream_t stream) {
  switch (choose_kernel(p, flags, AMODE)) {
    case K_WIDE_STREAM:
      if constexpr (AMODE == A_DENSE) return launch_gemm_wide_stream<T>(p, num_cus(), stream);
      break;
    case K_WIDE:
      if constexpr (AMODE == A_DENSE) return launch_gemm_wide<T>(p, num_cus(), stream);
      break;
    case K_RINGW:
      if constexpr (AMODE != A_CONV3X3) return launch_ringw<T, AMODE>(p, stream);
      break;
    case K_RING:
      if constexpr (AMODE != A_CONV3X3) return launch_ring<T, AMODE>(p, stream);
      break;
    case K_TWO_STAGE:
      return (flags & PM_FLAG_A_F32) ? launch1<T, AMODE, true>(p, stream) : launch1<T, AMODE, false>(p, stream);
  }
  return PM_E_SHAPE;  // (unreachable: choose_kernel gives a loader mode only kernels that have it)
}

// the loaders address an operand as (64-bit uniform base) + (32-bit lane byte offset)
static bool fits_u32(int64_t elements, int flags) {
  return elements * ((flags & PM_FLAG_A_F32) ? 4 : 2) < (1ll << 32) - (1ll << 24);  // (margin: a conv's descriptor base sits up to a tap shift before A)
}

static int check_common(const void* A, const void* W, void* C, int64_t M, int64_t N, int64_t K,
                        int act) {
  if (!A || !W || !C) return PM_E_NULL;
  if (M < 1 || N < 1 || K < 8 || (K & 7)) return PM_E_SHAPE;
  if (M > (1ll << 30) || N > (1ll << 30) || K > (1ll << 30)) return PM_E_SHAPE;
  if (act == PM_ACT_GEGLU && (N % 32) != 0) return PM_E_SHAPE;
  if (act < PM_ACT_NONE || act > PM_ACT_GELU) return PM_E_SHAPE;
  return PM_OK;
}

// What the three entry points share of the call parameters (p.M, p.N set): the epilogue's output / residual types, the
// statistics mode with its shape checks, the column tile count.
static int fill_epilogue(GemmParams& p, int flags, float* colstats) {
  p.out32 = (flags & PM_FLAG_OUT_F32) ? 1 : 0;
  p.res32 = (flags & (PM_FLAG_OUT_F32 | PM_FLAG_RES_F32)) ? 1 : 0;
  p.colstats = colstats;
  if (colstats != nullptr && (flags & PM_FLAG_STATS_I64)) {  // r06: int64 group totals [NI][32][4] instead of column sums
    p.gs_ni = (flags >> 8) & 0xff;
    if (p.gs_ni < 1 || (p.M % p.gs_ni) || (p.N & 31)) return PM_E_SHAPE;
    p.gs_rows = p.M / p.gs_ni;
  }
  p.ntiles = (p.N + BN - 1) / BN;
  return PM_OK;
}

// plan_split and what the plan must satisfy
static int plan_checked(GemmParams& p, void* workspace, size_t workspace_bytes, bool two_stage = false) {
  plan_split(p, workspace, workspace_bytes, two_stage);
  if (!GS_EPILOGUE && p.gs_ni > 0 && p.splits <= 1) return PM_E_SHAPE;  // (integer totals from an unsplit call: diagnostics build only)
  if (p.colstats != nullptr && p.splits > 1 && ((p.ldc & 3) || (p.R != nullptr && (p.ldr & 3)))) return PM_E_SHAPE;
  return PM_OK;
}

}  // namespace pm

using namespace pm;

extern "C" int pm_gemm(const void* A, int64_t lda, const void* W, int64_t ldw, const float* bias,
                       const void* residual, int64_t ldr, void* C, int64_t ldc, int64_t M,
                       int64_t N, int64_t K, int act, int flags, int dtype, void* workspace,
                       size_t workspace_bytes, float* colstats, void* stream) {
  int rc = check_common(A, W, C, M, N, K, act);
  if (rc) return rc;
  const int64_t Kw = (flags & PM_FLAG_W_WRAP) ? K / 2 : K;  // columns of W
  if ((flags & PM_FLAG_W_WRAP) && ((K % (2 * BK)) || (flags & PM_FLAG_A_F32))) return PM_E_SHAPE;
  if ((lda & ((flags & PM_FLAG_A_F32) ? 3 : 7)) || (ldw & 7) || lda < K || ldw < Kw) return PM_E_SHAPE;
  if (!fits_u32(M * lda, flags) || N * ldw * 2 >= (1ll << 32)) return PM_E_SHAPE;  // 32-bit lane offsets
  if ((flags & PM_FLAG_OUT_F32) && act == PM_ACT_GEGLU) return PM_E_SHAPE;
  if ((flags & PM_FLAG_BIAS_IS_SCALE) && (bias == nullptr || act == PM_ACT_GEGLU)) return PM_E_SHAPE;
  if ((flags & PM_FLAG_A_LO) && !(flags & PM_FLAG_A_F32)) return PM_E_SHAPE;
  GemmParams p{};
  p.A = A; p.lda = lda; p.Wt = W; p.ldw = ldw; p.bias = bias; p.R = residual; p.ldr = ldr;
  p.C = C; p.ldc = ldc; p.M = (int)M; p.N = (int)N; p.K = (int)K; p.act = act;
  p.bias_mul = (flags & PM_FLAG_BIAS_IS_SCALE) ? 1 : 0;
  p.a_lo = (flags & PM_FLAG_A_LO) ? 1 : 0;
  p.kwrap = (flags & PM_FLAG_W_WRAP) ? (int)Kw : 0;
  if ((rc = fill_epilogue(p, flags, colstats)) != PM_OK) return rc;
  p.zero = A;  // dense K tails never occur (K % 8 == 0 and whole chunks only); see kin below
  // A dense K tail (K % 64 != 0) reads chunk-wise: chunks with k >= K take `zero`; any 16 readable
  // bytes would poison the accumulator, so require a real zero source only when a tail exists.
  if (K % BK) return PM_E_SHAPE;  // all Linear layers on the path have K % 64 == 0
  if ((rc = plan_checked(p, workspace, workspace_bytes)) != PM_OK) return rc;
  PM_DISPATCH_DTYPE(dtype, T, return (launch<T, A_DENSE>(p, flags, (hipStream_t)stream)));
}

namespace pm {

// The planned call of pm_conv2d_3x3: argument checks, GemmParams, the split plan and the loader mode (`amode`: A_CONV3X3_FAST
// or A_CONV3X3).  The ONE place a 3x3 conv's parameters are built: the entry point launches what this returns and the
// diagnostics build's pm_debug_conv_kernel_choice asks choose_kernel about the same thing.
static int plan_conv3x3(GemmParams& p, int& amode, const void* x, int64_t ldx, const void* Wp, const float* bias,
                        const void* residual, int64_t ldr, void* y, int64_t ldy, int64_t F, int64_t H, int64_t W, int64_t Cin,
                        int64_t Cout, int stride, int upsample2x, int pad_lo, const void* zero_page, int flags, void* workspace,
                        size_t workspace_bytes, float* colstats) {
  if (!zero_page) return PM_E_NULL;
  if (stride != 1 && stride != 2) return PM_E_SHAPE;
  if (upsample2x && stride != 1) return PM_E_SHAPE;
  if (pad_lo != 0 && pad_lo != 1) return PM_E_SHAPE;
  if ((Cin & 7) || (ldx & ((flags & PM_FLAG_A_F32) ? 3 : 7)) || ldx < Cin) return PM_E_SHAPE;
  if (!fits_u32(F * H * W * ldx, flags)) return PM_E_SHAPE;  // 32-bit lane offsets: chunk the frames
  const int64_t Hv = upsample2x ? 2 * H : H, Wv = upsample2x ? 2 * W : W;
  // zero padding: pad_lo rows/cols before, 1 after (pad_lo = 0: the first-stage encoder's (0,1,0,1) pad)
  const int64_t Ho = (Hv + pad_lo - 2) / stride + 1, Wo = (Wv + pad_lo - 2) / stride + 1;
  const int64_t M = F * Ho * Wo, K = 9 * Cin;
  int rc = check_common(x, Wp, y, M, Cout, K, PM_ACT_NONE);
  if (rc) return rc;
  p = GemmParams{};
  p.A = x; p.lda = ldx; p.Wt = Wp; p.ldw = K; p.bias = bias; p.R = residual; p.ldr = ldr;
  p.C = y; p.ldc = ldy; p.M = (int)M; p.N = (int)Cout; p.K = (int)K; p.act = PM_ACT_NONE;
  if ((rc = fill_epilogue(p, flags, colstats)) != PM_OK) return rc;
  p.Hin = (int)H; p.Win = (int)W; p.Hv = (int)Hv; p.Wv = (int)Wv; p.Cin = (int)Cin;
  p.Ho = (int)Ho; p.Wo = (int)Wo; p.stride = stride; p.ups = upsample2x ? 1 : 0; p.pad = pad_lo;
  p.zero = zero_page;
  p.a_bytes = ((F * H * W - 1) * ldx + Cin) * ((flags & PM_FLAG_A_F32) ? 4 : 2);
  for (int t = 0; t < 9; ++t) {
    p.tap_a[t] = ((int64_t)(t / 3 - 1) * W + (t % 3 - 1)) * ldx * 2;
    p.tap_w[t] = (int64_t)t * Cin * 2;
  }
  amode = (!upsample2x && (Cin % BK) == 0) ? A_CONV3X3_FAST : A_CONV3X3;
  return plan_checked(p, workspace, workspace_bytes, /*two_stage=*/amode == A_CONV3X3);
}

// The same for pm_conv_temporal_k3_clips (loader mode A_CONVT3).
static int plan_conv_temporal(GemmParams& p, const void* x, int64_t ldx, const void* halo_lo, const void* halo_hi, const void* Wp,
                              const float* bias, const void* residual, int64_t ldr, void* y, int64_t ldy, int64_t F,
                              int64_t clip_frames, int64_t P, int64_t Cin, int64_t Cout, const void* zero_page, int flags,
                              void* workspace, size_t workspace_bytes, float* colstats) {
  if (!zero_page) return PM_E_NULL;
  if (clip_frames < 1 || F % clip_frames) return PM_E_SHAPE;
  if (clip_frames != F && (halo_lo || halo_hi)) return PM_E_SHAPE;  // (halo frames belong to ONE clip's ends)
  if ((Cin & 7) || (ldx & ((flags & PM_FLAG_A_F32) ? 3 : 7)) || ldx < Cin) return PM_E_SHAPE;
  if (Cin % BK) return PM_E_SHAPE;  // one tap per K-tile
  if (!fits_u32(F * P * ldx, flags)) return PM_E_SHAPE;
  const int64_t M = F * P, K = 3 * Cin;
  int rc = check_common(x, Wp, y, M, Cout, K, PM_ACT_NONE);
  if (rc) return rc;
  p = GemmParams{};
  p.A = x; p.lda = ldx; p.Wt = Wp; p.ldw = K; p.bias = bias; p.R = residual; p.ldr = ldr;
  p.C = y; p.ldc = ldy; p.M = (int)M; p.N = (int)Cout; p.K = (int)K; p.act = PM_ACT_NONE;
  if ((rc = fill_epilogue(p, flags, colstats)) != PM_OK) return rc;
  p.Cin = (int)Cin; p.F = (int)F; p.Fc = (int)clip_frames; p.P = (int)P; p.halo_lo = halo_lo; p.halo_hi = halo_hi;
  p.zero = zero_page;
  p.a_bytes = ((F * P - 1) * ldx + Cin) * ((flags & PM_FLAG_A_F32) ? 4 : 2);
  for (int t = 0; t < 3; ++t) {
    p.tap_a[t] = (int64_t)(t - 1) * P * ldx * 2;
    p.tap_w[t] = (int64_t)t * Cin * 2;
  }
  return plan_checked(p, workspace, workspace_bytes);
}

}  // namespace pm

extern "C" int pm_conv2d_3x3(const void* x, int64_t ldx, const void* Wp, const float* bias,
                             const void* residual, int64_t ldr, void* y, int64_t ldy, int64_t F,
                             int64_t H, int64_t W, int64_t Cin, int64_t Cout, int stride,
                             int upsample2x, int pad_lo, const void* zero_page, int flags, int dtype,
                             void* workspace, size_t workspace_bytes, float* colstats, void* stream) {
  GemmParams p;
  int amode = A_CONV3X3;
  const int rc = plan_conv3x3(p, amode, x, ldx, Wp, bias, residual, ldr, y, ldy, F, H, W, Cin, Cout, stride, upsample2x, pad_lo,
                              zero_page, flags, workspace, workspace_bytes, colstats);
  if (rc != PM_OK) return rc;
  if (amode == A_CONV3X3_FAST)
    PM_DISPATCH_DTYPE(dtype, T, return (launch<T, A_CONV3X3_FAST>(p, flags, (hipStream_t)stream)));
  PM_DISPATCH_DTYPE(dtype, T, return (launch<T, A_CONV3X3>(p, flags, (hipStream_t)stream)));
}

extern "C" int pm_conv_temporal_k3(const void* x, int64_t ldx, const void* halo_lo,
                                   const void* halo_hi, const void* Wp, const float* bias,
                                   const void* residual, int64_t ldr, void* y, int64_t ldy,
                                   int64_t F, int64_t P, int64_t Cin, int64_t Cout,
                                   const void* zero_page, int flags, int dtype, void* workspace,
                                   size_t workspace_bytes, float* colstats, void* stream) {
  return pm_conv_temporal_k3_clips(x, ldx, halo_lo, halo_hi, Wp, bias, residual, ldr, y, ldy, F, F, P, Cin, Cout, zero_page,
                                   flags, dtype, workspace, workspace_bytes, colstats, stream);
}

extern "C" int pm_conv_temporal_k3_clips(const void* x, int64_t ldx, const void* halo_lo,
                                         const void* halo_hi, const void* Wp, const float* bias,
                                         const void* residual, int64_t ldr, void* y, int64_t ldy,
                                         int64_t F, int64_t clip_frames, int64_t P, int64_t Cin, int64_t Cout,
                                         const void* zero_page, int flags, int dtype, void* workspace,
                                         size_t workspace_bytes, float* colstats, void* stream) {
  GemmParams p;
  const int rc = plan_conv_temporal(p, x, ldx, halo_lo, halo_hi, Wp, bias, residual, ldr, y, ldy, F, clip_frames, P, Cin, Cout,
                                    zero_page, flags, workspace, workspace_bytes, colstats);
  if (rc != PM_OK) return rc;
  PM_DISPATCH_DTYPE(dtype, T, return (launch<T, A_CONVT3>(p, flags, (hipStream_t)stream)));
}

#ifdef PM_DIAG
// Diagnostics build: the ring-family switches as a setter (the environment is read once per process) and the conv entry points'
// own kernel decision as a query (include/pandora_mi355x_diag.h).
extern "C" void pm_debug_gemm_ring(int ring, int ringw, int split_force) {
  init_once();  // (first: a later first use must not overwrite these with the environment's values)
  if (ring >= 0) g_ring = ring;
  if (ringw >= 0) g_ringw = ringw;
  if (split_force >= 0) g_split_force = split_force;
}

extern "C" int pm_debug_conv_kernel_choice(int kind, int64_t F, int64_t H, int64_t W, int64_t Cin, int64_t Cout, int stride,
                                           int upsample2x, int pad_lo, int flags, size_t workspace_bytes) {
  // contiguous operands, no residual, no statistics; the pointers are never dereferenced (only their non-NULLness is checked)
  static float dummy;
  void* const d = &dummy;
  GemmParams p;
  int amode = A_CONVT3, rc;
  if (kind == 0)
    rc = plan_conv3x3(p, amode, d, Cin, d, nullptr, nullptr, 0, d, Cout, F, H, W, Cin, Cout, stride, upsample2x, pad_lo, d, flags,
                      workspace_bytes ? d : nullptr, workspace_bytes, nullptr);
  else if (kind == 1)
    rc = plan_conv_temporal(p, d, Cin, nullptr, nullptr, d, nullptr, nullptr, 0, d, Cout, F, F, H * W, Cin, Cout, d, flags,
                            workspace_bytes ? d : nullptr, workspace_bytes, nullptr);
  else
    return PM_E_SHAPE;
  return rc != PM_OK ? rc : (int)choose_kernel(p, flags, amode);
}
#endif

extern "C" int pm_gemm_colstats_rows(int64_t M, int64_t N, int64_t K, int act, size_t workspace_bytes) {
  int ktps;
  const int s = choose_splits(M, N, K, act, &ktps);
  const bool split = s > 1 && workspace_bytes >= (size_t)s * M * N * sizeof(float) && (N & 3) == 0 && act != PM_ACT_GEGLU;
  return split ? 16 : 64;
}

extern "C" int pm_gemm_kernel_choice(int64_t M, int64_t N, int64_t K, int act, int flags, size_t workspace_bytes) {
  // pm_gemm's own decision (plan_split + choose_kernel): which kernel a dense call of this shape runs on
  if (M < 1 || N < 1 || K < BK || (K % BK)) return PM_E_SHAPE;
  GemmParams p{};
  p.M = (int)M; p.N = (int)N; p.K = (int)K; p.act = act;
  p.ntiles = (int)((N + BN - 1) / BN);
  static float dummy_ws;  // (only its non-NULLness matters to plan_split)
  plan_split(p, workspace_bytes ? &dummy_ws : nullptr, workspace_bytes);
  // (dense 16-bit call of contiguous operands, no residual / statistics / f32 output: what the caller of this query describes)
  p.lda = K; p.ldw = K; p.ldc = act == PM_ACT_GEGLU ? N / 2 : N;
  return choose_kernel(p, flags, A_DENSE);
}

extern "C" size_t pm_gemm_workspace_bytes(int64_t M, int64_t N, int64_t K, int act) {
  int ktps;
  const int s = choose_splits(M, N, K, act, &ktps);
  return s > 1 ? (size_t)s * M * N * sizeof(float) : 0;
}
