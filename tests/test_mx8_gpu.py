"""GPU: the MXFP8 projections (pm_quant_mx8 / pm_gemm_mx8, HipOps(fp8_linear=True)).

The quantiser is held bit for bit to the numpy restatement of the rule (tests/test_mx8_cpu.py); the GEMM bit for bit to the f64
product on operands whose every partial sum is exact in f32 (small-integer e4m3 elements, a different power-of-two scale per
(row, 32-block), so that a scale applied to the wrong lane, row or block shows); then random data, NaN rows, refused shapes, the
reduced and the full-width U-Net in the mode, and graph replay.  Bounds are ~1.3x the measured values, printed as [parity]."""
import numpy as np
import pytest
import torch

from oracle import golden_recipe as gr
from open_pandora_amd import capi, factory
from open_pandora_amd.ddim import DDIMSampler
from open_pandora_amd.ddpm import LatentVisualDiffusion
from open_pandora_amd.ops_hip import HipOps
from open_pandora_amd.unet import _Transformer
from test_mx8_cpu import mx8_dequant_np, mx8_quant_np
from test_oracle_golden import load, rel
from test_unet_gpu import FWD_TOL_REDUCED, _CountingLib, _digest_err, small_model

pytestmark = pytest.mark.gpu

MX_SYMBOLS = ("pm_quant_mx8", "pm_gemm_mx8")


def edge_rows(K):
    """rows of hand-picked blocks: 448 edge, ties, subnormals, zero block, NaN / Inf blocks, 2^-20 ... 2^20"""
    r = np.zeros((8, K), np.float32)
    r[0, :6] = [448.0, 8.5, 9.5, 17.0, -19.0, 449.0 / 2]
    r[1, :6] = [448.0, 2.0 ** -10, 3 * 2.0 ** -10, 7.5 * 2.0 ** -9, -2.0 ** -11, 2.0 ** -9]
    r[2, 32:34] = [449.0, 3.0]
    r[3, 5] = np.nan
    r[3, 40] = np.inf
    r[4, :] = np.exp2(np.linspace(-20, 20, K)).astype(np.float32) * np.where(np.arange(K) % 3 == 0, -1, 1)
    r[5, :] = 1e-40
    r[6, ::7] = 65504.0
    return r


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16, torch.float32])
@pytest.mark.parametrize("K", [320, 1280])
def test_quant_plain_bit_exact(dtype, K):
    ops = HipOps(torch.float16, "cuda:0")
    rng = np.random.default_rng(K)
    M = 77  # (ragged: not a multiple of the 4 rows of a workgroup)
    x = (rng.standard_normal((M, K)) * np.exp2(rng.integers(-8, 8, (M, 1)))).astype(np.float32)
    x[:8] = edge_rows(K)
    xt = torch.from_numpy(x).to(dtype)
    wide = torch.zeros(M, K + 64, dtype=dtype)  # ldx > K
    wide[:, :K] = xt
    q, s = ops.quant_mx8(wide.cuda()[:, :K])
    torch.cuda.synchronize()
    wq, ws = mx8_quant_np(xt.float().numpy())
    assert np.array_equal(s.cpu().numpy(), ws), np.argwhere(s.cpu().numpy() != ws)[:5]
    assert np.array_equal(q.cpu().numpy(), wq), np.argwhere(q.cpu().numpy() != wq)[:5]


@pytest.mark.parametrize("K", [320, 1280])
def test_quant_layernorm_fused(K):
    """LayerNorm mode against the restatement applied to the f32 LayerNorm computed on the CPU: the two f32 LayerNorms differ in
    their last bits, so a code may differ by one step where the CPU value sits on a rounding boundary - nowhere else."""
    ops = HipOps(torch.float16, "cuda:0")
    rng = np.random.default_rng(7 + K)
    M = 301
    x = (rng.standard_normal((M, K)) * 3 + rng.standard_normal((M, 1))).astype(np.float32)
    x[5, 17] = np.nan
    g = (1 + 0.1 * rng.standard_normal(K)).astype(np.float32)
    b = (0.1 * rng.standard_normal(K)).astype(np.float32)
    q, s = ops.ln_quant_mx8(torch.from_numpy(x).cuda(), torch.from_numpy(g).cuda(), torch.from_numpy(b).cuda(), 1e-5)
    torch.cuda.synchronize()
    xd = x.astype(np.float64)
    mu = xd.mean(1, keepdims=True)
    y = ((xd - mu) / np.sqrt(((xd - mu) ** 2).mean(1, keepdims=True) + 1e-5) * g + b).astype(np.float32)
    wq, ws = mx8_quant_np(y)
    gq, gs = q.cpu().numpy(), s.cpu().numpy()
    assert (gs[5] == 0xFF).all() and (gq[5] == 0x7F).all()  # the NaN row: every block NaN (the row statistics are NaN)
    keep = np.ones(M, bool)
    keep[5] = False
    assert (gs[keep] == ws[keep]).mean() > 0.999
    same = gs[keep] == ws[keep]
    dq, dw = mx8_dequant_np(gq[keep], gs[keep]), mx8_dequant_np(wq[keep], ws[keep])
    mism = (gq[keep] != wq[keep])
    print(f"\n[parity] pm_quant_mx8 LayerNorm mode K={K}: {mism.mean():.2e} of the codes differ from the CPU-LayerNorm restatement")
    assert mism.mean() < 2e-3
    agree = np.repeat(same, 32, axis=1)
    step = np.maximum(np.abs(dw) * 2 ** -3, np.repeat(np.ldexp(1.0, gs[keep].astype(np.int64) - 127 - 9), 32, axis=1))
    assert (np.abs(dq - dw)[agree] <= 1.01 * step[agree]).all()  # (one e4m3 step at most where the scales agree)


def exact_operands(rng, M, N, K):
    """e4m3 codes of small integers (-3 ... 3) and E8M0 scales 2^-1 ... 2^2 (A) / 2^0 ... 2^3 (W): |sum| < 2^21 in steps of 2^-1."""
    enc = {0: 0x00, 1: 0x38, 2: 0x40, 3: 0x44}
    lut = np.array([enc[abs(v)] | (0x80 if v < 0 else 0) for v in range(-3, 4)], np.uint8)
    ai, wi = rng.integers(-3, 4, (M, K)), rng.integers(-3, 4, (N, K))
    asc, wsc = rng.integers(126, 130, (M, K // 32)).astype(np.uint8), rng.integers(127, 131, (N, K // 32)).astype(np.uint8)
    A = ai * np.repeat(np.ldexp(1.0, asc.astype(np.int64) - 127), 32, 1)
    W = wi * np.repeat(np.ldexp(1.0, wsc.astype(np.int64) - 127), 32, 1)
    dev = lambda t: torch.from_numpy(np.ascontiguousarray(t)).cuda()
    return (dev(lut[ai + 3]), dev(asc)), (dev(lut[wi + 3]), dev(wsc)), A @ W.T


@pytest.mark.parametrize("K,N", [(320, 960), (640, 960), (1280, 960), (5120, 960), (320, 320), (320, 2560)])
def test_gemm_exact_f32_output(K, N):
    ops = HipOps(torch.bfloat16, "cuda:0")
    rng = np.random.default_rng(K * 7 + N)
    M = 200  # ragged on 128-row tiles
    a, w, ref = exact_operands(rng, M, N, K)
    res = torch.from_numpy(rng.integers(-50, 50, (M, N)).astype(np.float32)).cuda()
    bias = torch.from_numpy((rng.integers(-8, 8, N) * 0.5).astype(np.float32)).cuda()
    out = ops.gemm_mx8(a, w, bias, residual=res, stream=True)
    want = ref + bias.cpu().numpy() + res.cpu().numpy()
    assert np.array_equal(out.cpu().numpy().astype(np.float64), want)
    out = ops.gemm_mx8(a, w, None, residual=torch.zeros_like(res), stream=True)
    assert np.array_equal(out.cpu().numpy().astype(np.float64), ref)


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_gemm_exact_16bit_flavours(dtype):
    ops = HipOps(dtype, "cuda:0")
    rng = np.random.default_rng(5)
    M, N, K = 131, 960, 320
    a, w, ref = exact_operands(rng, M, N, K)
    r16 = lambda v: torch.from_numpy(np.asarray(v, np.float64)).to(torch.float32).to(dtype)
    same = lambda got, v: torch.equal(got.cpu(), r16(v))
    bias = torch.from_numpy((rng.integers(-8, 8, N) * 0.5).astype(np.float32)).cuda()
    cscale = torch.from_numpy(np.ldexp(1.0, rng.integers(-3, 3, N)).astype(np.float32)).cuda()
    res32 = torch.from_numpy(rng.integers(-50, 50, (M, N)).astype(np.float32)).cuda()
    res16 = res32.to(dtype)
    assert same(ops.gemm_mx8(a, w), ref)                                          # plain, no bias (attn2 q, temporal q|k|v)
    assert same(ops.gemm_mx8(a, w, bias), ref + bias.cpu().numpy())
    assert same(ops.gemm_mx8(a, w, col_scale=cscale), ref * cscale.cpu().numpy())  # spatial q|k|v
    assert same(ops.gemm_mx8(a, w, bias, residual=res32), ref + bias.cpu().numpy() + res32.cpu().numpy())  # ff2
    assert same(ops.gemm_mx8(a, w, bias, residual=res16), ref + bias.cpu().numpy() + res16.float().cpu().numpy())


def _gelu(x):
    import math
    return 0.5 * x * (1 + np.vectorize(math.erf)(x / np.sqrt(2.0)))


@pytest.mark.parametrize("N", [640, 2560])
def test_gemm_geglu_and_mx8_output(N):
    """GEGLU (weights interleaved [16 value | 16 gate]): the 16-bit output against the f64 GEGLU of the exact product, and the MXFP8
    output's scales / e4m3 codes against the restatement applied to that f64 GEGLU (the kernel's erf-GELU is a 9e-7 fit: codes may
    differ by one step on a rounding boundary)."""
    ops = HipOps(torch.bfloat16, "cuda:0")
    rng = np.random.default_rng(N)
    M, K = 150, 320
    a, w, ref = exact_operands(rng, M, N, K)
    ref = ref / 64.0  # (gate arguments of order 1)
    w = (w[0], (w[1].int() - 6).to(torch.uint8))
    bias = (rng.integers(-8, 8, N) * 0.125).astype(np.float32)
    pre = ref + bias
    v = pre.reshape(M, N // 32, 2, 16)
    want = (v[:, :, 0] * _gelu(v[:, :, 1])).reshape(M, N // 2)
    got = ops.gemm_mx8(a, w, torch.from_numpy(bias).cuda(), act="geglu").float().cpu().numpy()
    assert np.abs(got - want).max() <= 2 ** -8 * np.abs(want).max() + 1e-5
    q, s = ops.gemm_mx8(a, w, torch.from_numpy(bias).cuda(), act="geglu", mx_out=True)
    gq, gs = q.cpu().numpy(), s.cpu().numpy()
    wq, ws = mx8_quant_np(want.astype(np.float32))
    gq, wq = np.where(gq == 0x80, 0, gq), np.where(wq == 0x80, 0, wq)  # (-0 and +0: the sign of a zero GELU gate is not pinned)
    print(f"\n[parity] GEGLU -> MXFP8 N={N}: scales equal {np.mean(gs == ws):.5f}, codes equal {np.mean(gq == wq):.5f}")
    assert np.mean(gs == ws) > 0.999 and np.mean(gq == wq) > 0.995
    dg, dw = mx8_dequant_np(gq, gs), mx8_dequant_np(wq, ws)
    agree = np.repeat(gs == ws, 32, 1)
    step = np.maximum(np.abs(dw) * 2 ** -3, np.repeat(np.ldexp(1.0, gs.astype(np.int64) - 127 - 9), 32, 1))
    assert (np.abs(dg - dw)[agree] <= 1.01 * step[agree]).all()  # (one e4m3 step at most where the scales agree)


def test_gemm_random_data_error():
    """N(0,1) activations x 0.02 N(0,1) weights, both through pm_quant_mx8: C equals the f64 product of the DEQUANTISED operands
    to f32-accumulation level, and its error against the unquantised product is the numpy chain's."""
    ops = HipOps(torch.bfloat16, "cuda:0")
    rng = np.random.default_rng(1)
    M, N, K = 1000, 960, 1280
    x = rng.standard_normal((M, K)).astype(np.float32)
    wt = (0.02 * rng.standard_normal((N, K))).astype(np.float32)
    a, w = ops.quant_mx8(torch.from_numpy(x).cuda()), ops.quant_mx8(torch.from_numpy(wt).cuda())
    out = ops.gemm_mx8(a, w, None, residual=torch.zeros(M, N, device="cuda"), stream=True).cpu().numpy().astype(np.float64)
    (xq, xs), (wq, ws) = mx8_quant_np(x), mx8_quant_np(wt)
    assert np.array_equal(a[0].cpu().numpy(), xq) and np.array_equal(w[1].cpu().numpy(), ws)
    deq = mx8_dequant_np(xq, xs) @ mx8_dequant_np(wq, ws).T
    exact = x.astype(np.float64) @ wt.astype(np.float64).T
    e_acc = np.linalg.norm(out - deq) / np.linalg.norm(deq)
    e_gpu, e_np = np.linalg.norm(out - exact) / np.linalg.norm(exact), np.linalg.norm(deq - exact) / np.linalg.norm(exact)
    print(f"\n[parity] pm_gemm_mx8 random 1000x960x1280: vs dequantised product {e_acc:.2e}, vs unquantised {e_gpu:.3e} "
          f"(numpy chain {e_np:.3e})")
    assert e_acc <= 2e-5  # (measured 1.49e-5: the instruction's internal accumulation of its 128 products, not an f32 fma chain)
    assert abs(e_gpu / e_np - 1) < 0.03 and 0.02 < e_np < 0.07


def test_nan_row_and_refused_shapes():
    ops = HipOps(torch.bfloat16, "cuda:0")
    rng = np.random.default_rng(2)
    x = torch.from_numpy(rng.standard_normal((100, 320)).astype(np.float32))
    x[37, 100] = float("nan")
    a = ops.quant_mx8(x.cuda())
    w = ops.quant_mx8(torch.from_numpy(0.02 * rng.standard_normal((320, 320)).astype(np.float32)).cuda())
    out = ops.gemm_mx8(a, w).float().cpu()
    assert torch.isnan(out[37]).all() and not torch.isnan(out[torch.arange(100) != 37]).any()
    lib, p = ops.lib, lambda t: t.data_ptr()
    c = torch.empty(100, 320, dtype=torch.bfloat16, device="cuda")

    def call(N=320, K=320, act=0, flags=0, dt=capi.PM_BF16):
        return lib.pm_gemm_mx8(p(a[0]), 320, p(a[1]), 10, p(w[0]), 320, p(w[1]), 10, None, None, 0, p(c), 320, None, 0, 100, N, K,
                               act, flags, dt, None)
    assert call() == 0
    torch.cuda.synchronize()
    E = -2
    for flags in (capi.PM_FLAG_A_F32, capi.PM_FLAG_W_WRAP, capi.PM_FLAG_STATS_I64, capi.PM_FLAG_A_LO, 3 << 8):
        assert call(flags=flags) == E, flags
    assert call(dt=capi.PM_BF16 | capi.PM_OUT_HILO) == E
    assert call(N=48) == E and call(K=288) == E and call(act=capi.PM_ACT_SILU) == E
    assert call(dt=capi.PM_BF16 | capi.PM_OUT_MX8) != 0  # (MXFP8 output: GEGLU only)
    assert lib.pm_quant_mx8(p(x.cuda()), 320, None, None, 0.0, p(a[0]), 320, p(a[1]), 10, 100, 300, capi.PM_F32, None) == E


def _count(ops):
    cl = _CountingLib(ops.lib)
    ops.lib = cl
    return cl


def _n_blocks(m):
    return sum(isinstance(mod, _Transformer) for mod in m.modules())


FP8_LINEAR_FWD_TOL_REDUCED = 1.6e-1  # 1.3 x measured (1.24e-1 / 1.13e-1 on the two cases, f16, every block in the mode)


@pytest.mark.parametrize("tag,mc,h,w,t,fs", gr.UNET_SMALL_CASES[:2])
def test_unet_small_forward_fp8_linear(tag, mc, h, w, t, fs):
    g = load("unet_small.npz")[tag]
    ins, _, _ = gr.sampler_inputs(h, w)
    x = torch.cat([ins["x_T"], ins["c_concat"]], 1).cuda()
    args = (torch.tensor([t]).cuda(),)
    kw = dict(context=ins["c_crossattn"].cuda(), fs=torch.tensor([fs]).cuda())
    ops = HipOps(torch.float16, "cuda:0", fp8_linear=True, fp8_linear_min_rows=0)
    m = small_model(mc, ops)
    m(x, *args, **kw)  # (packs and quantises the weights)
    real, cl = ops.lib, _count(ops)
    try:
        y = m(x, *args, **kw)
    finally:
        ops.lib = real
    err = rel(y.cpu(), g)
    print(f"\n[parity] unet_small {tag} f16 + MXFP8 transformer projections: rel err {err:.2e}")
    assert FWD_TOL_REDUCED[torch.float16] < err <= FP8_LINEAR_FWD_TOL_REDUCED
    assert cl.calls.get("pm_gemm_mx8", 0) == 6 * _n_blocks(m)
    # the default mode: bit-identical to a plain op table, no call to the new symbols
    plain = HipOps(torch.float16, "cuda:0")
    y0 = small_model(mc, plain)(x, *args, **kw)
    off = HipOps(torch.float16, "cuda:0", fp8_linear=False, fp8_linear_min_rows=0)
    m_off = small_model(mc, off)
    real, cl = off.lib, _count(off)
    try:
        y1 = m_off(x, *args, **kw)
    finally:
        off.lib = real
    assert torch.equal(y0, y1) and not any(k in cl.calls for k in MX_SYMBOLS)


def test_fp8_linear_refuses_parity():
    with pytest.raises(ValueError):
        HipOps(torch.float16, "cuda:0", fp8_linear=True, parity=True)
    with pytest.raises(ValueError):
        HipOps(torch.float16, "cuda:0", fp8_linear=True, parity="selective")
    HipOps(torch.float16, "cuda:0", fp8_linear=True, fp8_attention=True)


FP8_LINEAR_FWD_TOL_FULL = 1.2e-1  # 1.3 x measured (9.0e-2, bf16, default threshold)


def test_unet_full_width_fp8_linear_40x64():
    g = load("unet_full_40x64.npz")
    base = HipOps(torch.bfloat16, "cuda:0")
    pm = factory.build_diffusion("320x512", base, seed=gr.WEIGHT_SEED)
    ins, cond, _ = gr.sampler_inputs(40, 64)
    c = {k: [t.cuda() for t in v] for k, v in cond.items()}
    args = (ins["x_T"].cuda(), torch.tensor([500]).cuda(), c)
    fs = torch.tensor([15]).cuda()
    pm.apply_model(*args, fs=fs)
    real, cl = base.lib, _count(base)
    try:
        pm.apply_model(*args, fs=fs)
    finally:
        base.lib = real
    n_default = sum(cl.calls.values())
    ops = HipOps(torch.bfloat16, "cuda:0", fp8_linear=True)
    pm.model.diffusion_model.bind(ops)
    pm.apply_model(*args, fs=fs)
    real, cl = ops.lib, _count(ops)
    try:
        y = pm.apply_model(*args, fs=fs)
    finally:
        ops.lib = real
    n_mx = cl.calls.get("pm_gemm_mx8", 0)
    err, std, gstd = _digest_err(y, g, "cond", FP8_LINEAR_FWD_TOL_FULL)
    print(f"\n[parity] unet_full 40x64 cond bf16 + MXFP8 projections (rows >= {ops.fp8_linear_min_rows}): rel err {err:.2e}; "
          f"{n_mx} MX GEMMs, {sum(cl.calls.values())} C-ABI calls (default {n_default})")
    assert err <= FP8_LINEAR_FWD_TOL_FULL
    # 21 blocks with >= 8192 rows at 320x512: 10 spatial + 10 temporal at levels 0-1, plus the temporal init_attn block behind the
    # stem (level 0), 6 projections each
    blocks = n_mx // 6
    assert n_mx == 6 * 21
    # per block: 3 LayerNorm-fused quantisers + 2 attention-output quantisers + 6 GEMMs, where the default mode runs the level-0/1
    # LayerNorm sites as ONE fused pm_ln_gemm call each: at most 3 more calls per block (measured: 975 against 913, +62)
    assert sum(cl.calls.values()) <= n_default + 3 * blocks
    del pm
    torch.cuda.empty_cache()


def test_fp8_linear_graph_replay_bit_identical():
    tag, mc, h, w, t, fs = gr.UNET_SMALL_CASES[0]
    ins, cond, uc = gr.sampler_inputs(h, w)
    dev = lambda cc: {k: [t_.cuda() for t_ in v] for k, v in cc.items()}
    outs = []
    for use_graph in (False, True):
        ops = HipOps(torch.float16, "cuda:0", fp8_linear=True, fp8_linear_min_rows=0)
        pm = LatentVisualDiffusion(small_model(mc, ops))
        y, _ = DDIMSampler(pm, use_graph=use_graph).sample(
            S=3, batch_size=1, shape=(4, 16, h, w), conditioning=dev(cond), verbose=False, unconditional_guidance_scale=4.0,
            unconditional_conditioning=dev(uc), eta=0.0, fs=torch.tensor([fs]).cuda(), timestep_spacing="uniform_trailing",
            x_T=ins["x_T"].cuda())
        outs.append(y.cpu())
    assert torch.equal(outs[0], outs[1])
