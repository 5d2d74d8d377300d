"""GPU: the fused 8-bit self-attention chain, HipOps(fp8_block=True):
ln_quant_mx8 -> pm_gemm_mx8_qkv_fp8 (packed e4m3 q', k, v^T) -> pm_attention_fp8_packed (MXFP8 O) -> pm_gemm_mx8 (to_out).

The packed-operand attention is the kernel pm_attention_fp8 runs (bit for bit); the producer's bytes are held to the numpy
restatement (tests/test_fp8_block_cpu.py) of the f32 GEMM output and, on exactly representable operands, to the bytes the
existing pack pass writes; the MXFP8 output to the restatement of the MXFP8 rule (tests/test_mx8_cpu.py).  In the U-Net the
unfused chain (fp8_linear + fp8_attention, both on the parent) is the yardstick."""
import numpy as np
import pytest
import torch

from oracle import golden_recipe as gr
from open_pandora_amd import capi, synth
from open_pandora_amd.ddim import DDIMSampler
from open_pandora_amd.ddpm import LatentVisualDiffusion
from open_pandora_amd.ops_hip import HipOps, PackedQKV
from open_pandora_amd.unet import UNetModel
from test_fp8_block_cpu import pack_qkv_np
from test_mx8_cpu import E4M3, mx8_quant_np
from test_oracle_golden import RH_KW, load, rel
from test_unet_gpu import _CountingLib, small_model

pytestmark = pytest.mark.gpu

NEW_SYMBOLS = ("pm_gemm_mx8_qkv_fp8", "pm_attention_fp8_packed")


def _workspace_operands(ops, B, heads, Nq, Nk):
    """q8 / k8 / v8t as pm_attention_fp8 left them in its workspace (the layout of the header)."""
    ws = ops._workspaces[("fp8", ops._stream())]
    nq, nk = (Nq + 63) // 64 * 64, (Nk + 63) // 64 * 64
    a, b = B * heads * nq * 64, B * heads * nk * 64
    return PackedQKV(ws[:a], ws[a:a + b], ws[a + b:a + 2 * b], B, Nq, Nk)


def _rnd(*shape, scale=1.0, seed=0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g) * scale


# ---- 1. packed attention is the same kernel ---------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("B,heads,N", [(2, 5, 333), (1, 5, 2100), (3, 2, 192)])
def test_packed_attention_equals_attention_fp8_bit_for_bit(dtype, B, heads, N):
    ops = HipOps(dtype, "cuda:0")
    C = heads * 64
    q, k, v = (_rnd(B, N, C, scale=s, seed=i).to(dtype).cuda() for i, s in ((1, 1.0), (2, 1.2), (3, 1.0)))
    want = ops.attention_fp8(q, k, v, heads)
    got = ops.attention_fp8_packed(_workspace_operands(ops, B, heads, N, N), heads)
    torch.cuda.synchronize()
    assert torch.equal(got, want)


# ---- 2. producer bytes, random operands -------------------------------------------------------------------------------------
def _gemm_f32(ops, a, w, bias, flags):
    """pm_gemm_mx8 with PM_FLAG_OUT_F32 at the C ABI, no residual: acc * scale[n] (or acc + bias[n]) unrounded."""
    (aq, as_), (wq, ws) = a, w
    M, K = aq.shape
    N = wq.shape[0]
    c = torch.empty(M, N, dtype=torch.float32, device="cuda")
    rc = ops.lib.pm_gemm_mx8(aq.data_ptr(), K, as_.data_ptr(), K // 32, wq.data_ptr(), K, ws.data_ptr(), K // 32, bias.data_ptr(),
                             None, 0, c.data_ptr(), N, None, 0, M, N, K, capi.PM_ACT_NONE, flags | capi.PM_FLAG_OUT_F32,
                             ops.dt, ops._stream())
    assert rc == 0, rc
    return c


def _same_bytes(packed, want, what):
    for name, got, w in zip(("q8", "k8", "v8t"), packed[:3], want):
        g = got.cpu().numpy().reshape(w.shape)
        bad = np.argwhere(g != w)
        assert bad.size == 0, f"{what}: {name} differs at {bad[:5].tolist()} ({len(bad)} bytes)"


# (M, heads, K, P): inner = 320 / 640 / 1280 (a 128-column tile straddles q|k and k|v at 320), K % 128 == 64, M % 128 == 64, B > 1
QKV_CASES = [(192, 5, 320, 64), (512, 10, 640, 256), (384, 20, 1280, 128), (320, 5, 1280, 64), (448, 10, 320, 448)]


@pytest.mark.parametrize("M,heads,K,P", QKV_CASES)
def test_qkv_producer_bytes_random_operands(M, heads, K, P):
    ops = HipOps(torch.bfloat16, "cuda:0")
    rng = np.random.default_rng(M + heads + K)
    N = 3 * heads * 64
    x = (rng.standard_normal((M, K)) * np.exp2(rng.integers(-2, 9, (M, 1)))).astype(np.float32)  # (some values clamp at 448)
    x[7, 33] = np.nan  # one NaN block: every output of row 7 is NaN -> 0x7F
    a = ops.quant_mx8(torch.from_numpy(x).cuda())
    w = ops.quant_mx8(torch.from_numpy((0.05 * rng.standard_normal((N, K))).astype(np.float32)).cuda())
    scale = torch.cat([torch.full((heads * 64,), float(ops.q_prescale)), torch.ones(2 * heads * 64)]).float().cuda()
    y = _gemm_f32(ops, a, w, scale, capi.PM_FLAG_BIAS_IS_SCALE).cpu().numpy()
    packed = ops.gemm_mx8_qkv_fp8(a, w, scale, heads, P)
    torch.cuda.synchronize()
    assert np.isnan(y[7]).all() and np.abs(np.nan_to_num(y)).max() > 448
    _same_bytes(packed, pack_qkv_np(y, heads, P), "column scale")
    # the additive flavour, q prescale as qmul
    bias = torch.from_numpy((0.5 * rng.standard_normal(N)).astype(np.float32)).cuda()
    y = _gemm_f32(ops, a, w, bias, 0).cpu().numpy()
    packed = ops.gemm_mx8_qkv_fp8(a, w, None, heads, P, bias=bias, qmul=ops.q_prescale)
    torch.cuda.synchronize()
    _same_bytes(packed, pack_qkv_np(y, heads, P, qmul=np.float32(ops.q_prescale)), "bias + qmul")


def test_qkv_producer_refused_shapes():
    ops = HipOps(torch.bfloat16, "cuda:0")
    rng = np.random.default_rng(0)
    heads, K = 5, 320
    a = ops.quant_mx8(torch.from_numpy(rng.standard_normal((192, K)).astype(np.float32)).cuda())
    w = ops.quant_mx8(torch.from_numpy(rng.standard_normal((960, K)).astype(np.float32)).cuda())
    buf = torch.empty(3 * 192 * 320, dtype=torch.uint8, device="cuda")
    p = lambda t: t.data_ptr()

    def call(M=192, P=64, K=K, flags=0, q8=p(buf)):
        return ops.lib.pm_gemm_mx8_qkv_fp8(p(a[0]), 320, p(a[1]), 10, p(w[0]), 320, p(w[1]), 10, None, q8, p(buf) + 192 * 320,
                                           p(buf) + 2 * 192 * 320, M, K, heads, P, 1.0, flags, None)
    assert call() == 0
    torch.cuda.synchronize()
    assert call(P=96) == -2 and call(P=32, M=192) == -2 and call(M=160) == -2 and call(K=288) == -2  # PM_E_SHAPE
    assert call(flags=capi.PM_FLAG_BIAS_IS_SCALE) == -2 and call(flags=capi.PM_FLAG_OUT_F32) == -2
    assert call(q8=None) == -3 and call(q8=p(buf) + 4) == -2
    with pytest.raises(capi.PandoraKernelError):
        ops.gemm_mx8_qkv_fp8((a[0][:96], a[1][:96]), w, None, heads, 96)


# ---- 3. producer against the existing pack pass -----------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("M,heads,K,P", [(192, 5, 320, 64), (384, 10, 640, 128)])
def test_qkv_producer_equals_pack_pass_on_representable_values(dtype, M, heads, K, P):
    """One nonzero per row of A (+-1..3 times 2^-1..2^1), W small integers times 2^0..2^2, column scales 2^-2..2^0: every
    q|k|v value is a product a * w * s in {0, 1, 2, 3, 4, 6, 9} x 2^(-3 .. 3) - exact in e4m3, f16 and bf16."""
    ops = HipOps(dtype, "cuda:0")
    rng = np.random.default_rng(K + P)
    N = 3 * heads * 64
    enc = {0: 0x00, 1: 0x38, 2: 0x40, 3: 0x44}
    lut = np.array([enc[abs(v)] | (0x80 if v < 0 else 0) for v in range(-3, 4)], np.uint8)
    ai = np.zeros((M, K), np.int64)
    ai[np.arange(M), rng.integers(0, K, M)] = rng.choice([-3, -2, -1, 1, 2, 3], M)
    wi = rng.integers(-3, 4, (N, K))
    asc, wsc = rng.integers(126, 129, (M, K // 32)).astype(np.uint8), rng.integers(127, 130, (N, K // 32)).astype(np.uint8)
    dev = lambda t: torch.from_numpy(np.ascontiguousarray(t)).cuda()
    a, w = (dev(lut[ai + 3]), dev(asc)), (dev(lut[wi + 3]), dev(wsc))
    cs = torch.from_numpy(np.ldexp(1.0, rng.integers(-2, 1, N)).astype(np.float32)).cuda()
    qkv = ops.gemm_mx8(a, w, col_scale=cs).view(M // P, P, N)
    inner = heads * 64
    ops.attention_fp8(qkv[..., :inner], qkv[..., inner:2 * inner], qkv[..., 2 * inner:], heads, prescaled=True)
    torch.cuda.synchronize()
    want = [t.cpu().numpy().copy() for t in _workspace_operands(ops, M // P, heads, P, P)[:3]]
    assert len(np.unique(want[0])) > 10 and len(np.unique(want[2])) > 10  # (not a degenerate case)
    packed = ops.gemm_mx8_qkv_fp8(a, w, cs, heads, P)
    torch.cuda.synchronize()
    _same_bytes(packed, want, "fused against attn_fp8_pack_kernel")


# ---- 4. / 5. MXFP8 output ---------------------------------------------------------------------------------------------------
def test_mx8_output_exact_on_one_hot_softmax():
    """The one-hot construction of test_ops_gpu.py::test_attention_fp8_exact_on_fp8_representable_inputs with larger codes (q,
    k in {0, 64}): the matching key leads every other by >= 3072 in the base-2 domain, so every other probability and every
    rescale factor is exactly 0, the row sum exactly 1 and O exactly the gathered V rows, signs of zeros included."""
    ops = HipOps(torch.float16, "cuda:0")
    g = torch.Generator().manual_seed(3)
    B, heads, N = 2, 3, 192
    C = heads * 64
    grid = torch.tensor([-2.0, -1.5, -1.0, -0.5, 0.0, 0.5, 1.0, 1.5, 2.0])
    v = grid[torch.randint(0, 9, (B, N, C), generator=g)]
    v[0, :, :32] *= 2.0 ** -4  # (a block of small values, still normal e4m3 numbers: its scale differs from its neighbours')
    k = torch.zeros(B, N, C)
    q = torch.zeros(B, N, C)
    perm = torch.stack([torch.randperm(N, generator=g) for _ in range(B * heads)]).reshape(B, heads, N)
    for b in range(B):
        for h in range(heads):
            bits = ((torch.arange(N)[:, None] >> torch.arange(8)[None]) & 1).float()          # [N, 8]
            code = torch.cat([bits, 1 - bits], 1).repeat(1, 4) * 64.0                          # [N, 64], 32 entries of 64
            k[b, :, h * 64:(h + 1) * 64] = code
            q[b, :, h * 64:(h + 1) * 64] = code[perm[b, h]]
    want = torch.stack([torch.cat([v[b, perm[b, h], h * 64:(h + 1) * 64] for h in range(heads)], -1) for b in range(B)])
    o16 = ops.attention_fp8(q.half().cuda(), k.half().cuda(), v.half().cuda(), heads)
    assert torch.equal(o16.float().cpu(), want)  # (the construction is exact in the existing kernel already)
    o8, os_ = ops.attention_fp8_packed(_workspace_operands(ops, B, heads, N, N), heads, mx_out=True)
    torch.cuda.synchronize()
    wq, ws = mx8_quant_np(want.reshape(B * N, C).numpy())
    assert o8.shape == (B * N, C) and os_.shape == (B * N, C // 32)
    assert np.array_equal(os_.cpu().numpy(), ws), np.argwhere(os_.cpu().numpy() != ws)[:5]
    assert np.array_equal(o8.cpu().numpy(), wq), np.argwhere(o8.cpu().numpy() != wq)[:5]
    assert len(np.unique(ws)) >= 3


def _rule_exp(a):
    """X of the header's rule for block maxima a > 0 (f64 in, the f32 rule)."""
    f, e = np.frexp(np.asarray(a, np.float32))
    return np.clip(e.astype(np.int64) - 9 + (f > 0.875), -127, 127)


@pytest.mark.parametrize("B,heads,N", [(2, 5, 333), (1, 10, 1024)])
def test_mx8_output_random_data(B, heads, N):
    """Against the 16-bit output of the same kernel on the same packed operands: per element half an e4m3 step (normal: 2^-4
    relative; subnormal: 2^(X-10)) plus the f16 rounding of the comparison side; X by the rule from a block maximum within
    (1 +- 2^-10) of the 16-bit one.  Derived from the formats, no element exempt."""
    ops = HipOps(torch.float16, "cuda:0")
    C = heads * 64
    q, k, v = (_rnd(B, N, C, scale=s, seed=i).half().cuda() for i, s in ((4, 1.0), (5, 1.2), (6, 1.0)))
    v *= 8.0            # block maxima of O around 1 .. 10 (see the check on X below)
    v[..., :64] *= 16.0  # (one head on another scale)
    v[0, :, 64:96] = 0  # an all-zero block
    ops.attention_fp8(q, k, v, heads)
    packed = _workspace_operands(ops, B, heads, N, N)
    o16 = ops.attention_fp8_packed(packed, heads).float().cpu().numpy().reshape(B * N, C).astype(np.float64)
    o8, os_ = ops.attention_fp8_packed(packed, heads, mx_out=True)
    torch.cuda.synchronize()
    o8, os_ = o8.cpu().numpy(), os_.cpu().numpy()
    assert (os_ != 0xFF).all() and not np.isin(o8, (0x7F, 0xFF)).any()
    X = os_.astype(np.int64) - 127
    deq = (E4M3[o8].reshape(B * N, C // 32, 32) * np.ldexp(1.0, X)[..., None]).reshape(B * N, C)
    Xe = np.repeat(X, 32, 1)
    bound = 2.0 ** -4 * np.abs(o16) + np.ldexp(1.0, Xe - 10) + 2.0 ** -10 * np.abs(o16)
    # The bound's last term is the f16 rounding of the comparison side as a RELATIVE error: true for normal f16 numbers.  An
    # f16-subnormal o16 (|o| < 2^-14) is off by up to 2^-25 instead, which the e4m3 terms cover (2^-4 |o| >= 2^-25 around the
    # worst case |o| = 2^(X-10)) as long as X >= -11: the data above keeps every non-zero block there.
    nzb = np.abs(o16).reshape(B * N, C // 32, 32).max(-1) > 0
    assert X[nzb].min() >= -11, X[nzb].min()
    excess = np.abs(deq - o16) - bound
    print(f"\n[parity] MXFP8 attention output B={B} heads={heads} N={N}: max (|deq - o16| - bound) = {excess.max():.3e}, "
          f"worst ratio {np.max(np.abs(deq - o16) / bound):.3f}")
    assert (excess <= 0).all(), np.argwhere(excess > 0)[:5]
    amax = np.abs(o16).reshape(B * N, C // 32, 32).max(-1)
    nz = amax > 0
    lo, hi = _rule_exp(amax[nz] * (1 - 2.0 ** -10)), _rule_exp(amax[nz] * (1 + 2.0 ** -10))
    assert ((lo <= X[nz]) & (X[nz] <= hi)).all()
    assert (X[~nz] <= -127 + 24).all() and (~nz).sum() >= N  # the zero block: O is 0 (or an f16-underflow-sized residue)


# ---- 6. in the U-Net --------------------------------------------------------------------------------------------------------
def _forward_counted(ops, m, x, args, kw):
    m(x, *args, **kw)  # (packs and quantises the weights)
    real, cl = ops.lib, _CountingLib(ops.lib)
    ops.lib = cl
    tokens = []
    inner_fp8 = ops.attention_fp8
    ops.attention_fp8 = lambda q, *a, **k: (tokens.append(q.shape[1]), inner_fp8(q, *a, **k))[1]
    try:
        y = m(x, *args, **kw)
    finally:
        ops.lib = real
        del ops.attention_fp8
    return y, cl.calls, tokens


MODE = dict(fp8_linear=True, fp8_attention=True, fp8_linear_min_rows=0, fp8_min_tokens=0)


@pytest.mark.parametrize("tag,mc,h,w,t,fs", gr.UNET_SMALL_CASES[:2])
def test_unet_small_forward_fp8_block(tag, mc, h, w, t, fs):
    """The fused chain at every spatial self-attention with P % 64 == 0 (level 0 of these models), the unfused calls elsewhere;
    error against the CPU oracle within 1.1 x the unfused chain's on the same inputs (the fused chain drops two 16-bit roundings
    and adds none; 10 % for e4m3 tie flips from the moved rounding points)."""
    g = load("unet_small.npz")[tag]
    ins, _, _ = gr.sampler_inputs(h, w)
    x = torch.cat([ins["x_T"], ins["c_concat"]], 1).cuda()
    args = (torch.tensor([t]).cuda(),)
    kw = dict(context=ins["c_crossattn"].cuda(), fs=torch.tensor([fs]).cuda())
    ops_u = HipOps(torch.float16, "cuda:0", **MODE)
    y_u, calls_u, tokens = _forward_counted(ops_u, small_model(mc, ops_u), x, args, kw)
    n64 = sum(1 for p in tokens if p % 64 == 0)
    assert n64 > 0 and len(tokens) > n64 and not any(s in calls_u for s in NEW_SYMBOLS)
    ops_f = HipOps(torch.float16, "cuda:0", fp8_block=True, **MODE)
    y_f, calls_f, tokens_f = _forward_counted(ops_f, small_model(mc, ops_f), x, args, kw)
    assert calls_f.get("pm_gemm_mx8_qkv_fp8", 0) == n64 and calls_f.get("pm_attention_fp8_packed", 0) == n64
    assert calls_f.get("pm_attention_fp8", 0) == len(tokens) - n64 and all(p % 64 for p in tokens_f)  # no pack pass at fused sites
    assert calls_f["pm_gemm_mx8"] == calls_u["pm_gemm_mx8"] - n64
    assert calls_f["pm_quant_mx8"] == calls_u["pm_quant_mx8"] - n64  # no quantiser in front of those to_out's
    launches = lambda c: sum(n for k, n in c.items() if k != "pm_attention_fp8_workspace_bytes")  # (a size query, no launch)
    assert launches(calls_f) == launches(calls_u) - n64  # five calls per site become four
    e_u, e_f = rel(y_u.cpu(), g), rel(y_f.cpu(), g)
    print(f"\n[parity] unet_small {tag} f16: fused fp8 block rel err {e_f:.3e}, unfused chain {e_u:.3e} ({n64} fused sites of "
          f"{len(tokens)} spatial self-attentions)")
    assert e_f <= 1.1 * e_u


def _one_level_model(ops):
    m = UNetModel(**dict(RH_KW, model_channels=64, channel_mult=[1], attention_resolutions=[1])).eval()
    m.load_state_dict(synth.synth_state_dict(m, seed=gr.WEIGHT_SEED))
    return m.bind(ops)


def test_fp8_block_falls_back_where_tokens_are_not_whole_tiles():
    """A one-level U-Net (no downsampling: any map size runs) at 8 x 12 = 96 tokens: the mode makes the unfused calls and its
    output equals the unfused mode's bit for bit; at 8 x 8 the same model takes the fused chain."""
    outs = {}
    for hw in ((8, 12), (8, 8)):
        ins, _, _ = gr.sampler_inputs(*hw)
        x = torch.cat([ins["x_T"], ins["c_concat"]], 1).cuda()
        args = (torch.tensor([500]).cuda(),)
        kw = dict(context=ins["c_crossattn"].cuda(), fs=torch.tensor([15]).cuda())
        for fused in (False, True):
            ops = HipOps(torch.float16, "cuda:0", fp8_block=fused, **MODE)
            outs[hw, fused] = _forward_counted(ops, _one_level_model(ops), x, args, kw)
    y_u, calls_u, tokens = outs[(8, 12), False]
    y_f, calls_f, _ = outs[(8, 12), True]
    assert tokens and all(p == 96 for p in tokens)
    assert torch.equal(y_f, y_u) and calls_f == calls_u and not any(s in calls_f for s in NEW_SYMBOLS)
    y_u, calls_u, tokens = outs[(8, 8), False]
    y_f, calls_f, _ = outs[(8, 8), True]
    assert calls_f.get("pm_gemm_mx8_qkv_fp8", 0) == len(tokens) > 0 and "pm_attention_fp8" not in calls_f
    assert not torch.equal(y_f, y_u) and rel(y_f, y_u) < 0.1


def test_fp8_block_respects_the_thresholds_of_both_modes():
    """A site takes the fused chain only where it would take BOTH gemm_mx8 and attention_fp8."""
    tag, mc, h, w, t, fs = gr.UNET_SMALL_CASES[0]
    ins, _, _ = gr.sampler_inputs(h, w)
    x = torch.cat([ins["x_T"], ins["c_concat"]], 1).cuda()
    args = (torch.tensor([t]).cuda(),)
    kw = dict(context=ins["c_crossattn"].cuda(), fs=torch.tensor([fs]).cuda())
    for thr in (dict(fp8_min_tokens=100, fp8_linear_min_rows=0), dict(fp8_min_tokens=0, fp8_linear_min_rows=1 << 20)):
        ys = []
        for fused in (False, True):
            ops = HipOps(torch.float16, "cuda:0", fp8_linear=True, fp8_attention=True, fp8_block=fused, **thr)
            y, calls, _ = _forward_counted(ops, small_model(mc, ops), x, args, kw)
            assert not any(s in calls for s in NEW_SYMBOLS)
            ys.append(y)
        assert torch.equal(ys[0], ys[1])


# ---- 7. graph replay --------------------------------------------------------------------------------------------------------
def test_fp8_block_graph_replay_bit_identical():
    tag, mc, h, w, t, fs = gr.UNET_SMALL_CASES[0]
    ins, cond, uc = gr.sampler_inputs(h, w)
    dev = lambda cc: {k: [t_.cuda() for t_ in v] for k, v in cc.items()}
    outs = []
    for use_graph in (False, True):
        ops = HipOps(torch.float16, "cuda:0", fp8_block=True, **MODE)
        pm = LatentVisualDiffusion(small_model(mc, ops))
        y, _ = DDIMSampler(pm, use_graph=use_graph).sample(
            S=3, batch_size=1, shape=(4, 16, h, w), conditioning=dev(cond), verbose=False, unconditional_guidance_scale=4.0,
            unconditional_conditioning=dev(uc), eta=0.0, fs=torch.tensor([fs]).cuda(), timestep_spacing="uniform_trailing",
            x_T=ins["x_T"].cuda())
        outs.append(y.cpu())
    assert torch.equal(outs[0], outs[1]) and torch.isfinite(outs[0]).all()
