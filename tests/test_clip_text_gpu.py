"""GPU: the OpenCLIP text tower on the HIP kernels - pm_embed_tokens bit for bit, pm_attention_causal as an exact selection
(tests/attn_causal_exact.py), the tower against the fixture of HF transformers' CLIPTextModel at the reduced and the shipped
size (tests/golden/clip_text_hf.npz), and factory.build_runner on the kernels."""
import pytest
import torch

import attn_causal_exact as cx
import clip_text_ref as ref
from oracle import golden_recipe as gr
from open_pandora_amd import capi, factory
from open_pandora_amd.clip_text import VIT_H_14_TEXT, FrozenOpenCLIPEmbedder
from test_clip_text_cpu import reduced_yaml_and_checkpoint, runner_inputs, uncond_reference
from test_unet_gpu import FWD_TOL, FWD_TOL_REDUCED

pytestmark = pytest.mark.gpu
DTYPES = [torch.float16, torch.bfloat16]


@pytest.mark.parametrize("dtype", DTYPES, ids=["f16", "bf16"])
@pytest.mark.parametrize("B,N,V,W", [(2, 77, 1000, 128), (1, 5, 17, 8)])
def test_embed_tokens_bit_exact(hip_ops_factory, dtype, B, N, V, W):
    """out = f32(table[ids]) + pos: one f32 add per element, so bit for bit; the output is a column slice of a wider
    NaN-filled buffer whose guards survive; an id outside the table is refused before the launch."""
    ops = hip_ops_factory(dtype)
    g = torch.Generator().manual_seed(B * N + W)
    ids = torch.randint(0, V, (B, N), generator=g)
    ids[0, 0], ids[-1, -1] = 0, V - 1
    table = torch.randn(V, W, generator=g).to(dtype)
    pos = torch.randn(N, W, generator=g)
    want = table.float()[ids].reshape(B * N, W) + pos.repeat(B, 1)
    buf = torch.full((B * N + 2, W + 8), float("nan"), device="cuda")
    out = buf[1:1 + B * N, 4:4 + W]
    y = ops.embed_tokens(ids.cuda(), table.cuda(), pos.cuda(), out=out)
    torch.cuda.synchronize()
    assert y.data_ptr() == out.data_ptr() and torch.equal(out.cpu(), want)
    guard = torch.ones_like(buf, dtype=torch.bool)
    guard[1:1 + B * N, 4:4 + W] = False
    assert bool(torch.isnan(buf[guard]).all())
    assert torch.equal(ops.embed_tokens(ids.cuda(), table.cuda(), pos.cuda()).cpu(), want)  # the op's own buffer
    for bad in (-1, V):
        wrong = ids.clone()
        wrong[0, N // 2] = bad
        with pytest.raises(ValueError, match="token ids"):
            ops.embed_tokens(wrong.cuda(), table.cuda(), pos.cuda())


def _fused(d, Nq, Nk, C):
    """q | k | v as column slices of ONE NaN-filled [B, Nk, 8 + 3C + 8] buffer (q in its first Nq rows), and the output as a
    slice of a NaN-filled buffer with a guard row before and after every batch element and 8 columns on either side"""
    buf = torch.full((cx.B, Nk, 3 * C + 16), float("nan"), dtype=d["q"].dtype, device="cuda")
    q, k, v = buf[:, :Nq, 8:8 + C], buf[:, :, 8 + C:8 + 2 * C], buf[:, :, 8 + 2 * C:8 + 3 * C]
    q.copy_(d["q"]), k.copy_(d["k"]), v.copy_(d["v"])
    obuf = torch.full((cx.B, Nq + 2, C + 16), float("nan"), dtype=d["q"].dtype, device="cuda")
    return q, k, v, obuf, obuf[:, 1:1 + Nq, 8:8 + C]


@pytest.mark.parametrize("dtype", DTYPES, ids=["f16", "bf16"])
@pytest.mark.parametrize("D", cx.HEAD_DIMS)
@pytest.mark.parametrize("Nq,Nk,q_pos0", cx.CASES)
def test_attention_causal_exact_selection(hip_ops_factory, dtype, D, Nq, Nk, q_pos0):
    """Every query's code matches one visible key and (wherever a later key exists) one future key holding another v row: the
    kernel must return the visible row exactly.  Ignoring the mask gives `unmasked`, the mean of the two."""
    ops = hip_ops_factory(dtype)
    d = cx.build(Nq, Nk, q_pos0, D, dtype)
    C = cx.HEADS * D
    q, k, v, obuf, out = _fused(d, Nq, Nk, C)
    ops.attention_causal(q, k, v, cx.HEADS, q_pos0=q_pos0, out=out)
    torch.cuda.synchronize()
    got = out.cpu()
    if not torch.equal(got, d["want"]):
        bad = ((got != d["want"]) | torch.isnan(got)).reshape(cx.B, Nq, cx.HEADS, D).any(-1).nonzero()
        b, i, h = bad[0].tolist()
        same_as_unmasked = torch.equal(got.reshape(cx.B, Nq, cx.HEADS, D)[b, i, h], d["unmasked"].reshape(cx.B, Nq, cx.HEADS, D)[b, i, h])
        raise AssertionError(f"{bad.shape[0]} wrong rows; first: batch {b} head {h} row {i} (last visible key {q_pos0 + i}): "
                             f"visible matches {d['vis'][b][h][i]}, future matches {d['fut'][b][h][i]}; "
                             f"{'got = the mean over visible AND future matches: the mask is ignored' if same_as_unmasked else ''} "
                             f"got[:8] {got[b, i, h * D:h * D + 8].tolist()} want[:8] {d['want'][b, i, h * D:h * D + 8].tolist()}")
    guard = torch.ones_like(obuf, dtype=torch.bool)
    guard[:, 1:1 + Nq, 8:8 + C] = False
    assert bool(torch.isnan(obuf[guard]).all()), "wrote outside its output slice"
    # the op's own output buffer, contiguous operands
    assert torch.equal(ops.attention_causal(d["q"].cuda(), d["k"].cuda(), d["v"].cuda(), cx.HEADS, q_pos0=q_pos0).cpu(), d["want"])


@pytest.mark.parametrize("dtype", DTYPES, ids=["f16", "bf16"])
def test_attention_causal_guards(hip_ops_factory, dtype):
    """q_pos0 < 0 and q_pos0 + Nq > Nk: PM_E_SHAPE from the entry point, which returns before it launches anything."""
    ops = hip_ops_factory(dtype)
    q = torch.zeros(1, 3, 64, dtype=dtype, device="cuda")
    kv = torch.zeros(1, 70, 64, dtype=dtype, device="cuda")
    out = torch.full((1, 3, 64), 7.0, dtype=dtype, device="cuda")
    for p0 in (-1, 68, 1 << 40):
        with pytest.raises(capi.PandoraKernelError, match=r"shape.*\(code -2\)"):
            ops.attention_causal(q, kv, kv, 1, q_pos0=p0, out=out)
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())
    ops.attention_causal(q, kv, kv, 1, q_pos0=67, out=out)  # the last admissible offset
    torch.cuda.synchronize()
    assert bool((out == 0.0).all())


def _tower_on_kernels(cfg, layer, ops):
    with torch.device("meta"):
        m = FrozenOpenCLIPEmbedder(text_cfg=cfg, layer=layer)
    m.load_state_dict(ref.state_dict(cfg, "cuda"), assign=True, strict=True)
    return m.bind(ops)


@pytest.mark.parametrize("dtype", DTYPES, ids=["f16", "bf16"])
@pytest.mark.parametrize("tag", ["small", "vit_h_14"])
def test_tower_against_the_hf_clip_text_model_fixture(hip_ops_factory, dtype, tag):
    """The bound is the vision tower's rule (tests/test_clip_vision_gpu.py): FWD_TOL_REDUCED at the reduced size, 2 x FWD_TOL at
    the shipped one - the same op chain with 46 residual adds of 16-bit branch results in place of 64."""
    import time
    g = ref.load_golden()
    ops = hip_ops_factory(dtype)
    cfg, tol, layers = ((ref.SMALL, FWD_TOL_REDUCED[dtype], ("penultimate", "last")) if tag == "small"
                        else (dict(VIT_H_14_TEXT), 2 * FWD_TOL[dtype], ("penultimate",)))
    ids = torch.as_tensor(g[f"{tag}/ids"]).cuda()
    for layer in layers:
        m = _tower_on_kernels(cfg, layer, ops)
        got = m(ids)
        assert got.shape == (ids.shape[0], 77, cfg["width"])
        err = gr.compare_digest(got, g, f"{tag}/{layer}", tol)[0]
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        m([""])
        torch.cuda.synchronize()
        print(f"\n[parity] clip text tower {tag} {layer} {dtype} vs HF CLIPTextModel: rel err {err:.2e} (bound {tol:.1e}); "
              f'one [""] call {1e3 * (time.perf_counter() - t0):.1f} ms')
        assert err <= tol
        del m


@pytest.mark.parametrize("dtype", DTYPES, ids=["f16", "bf16"])
def test_build_runner_on_the_kernels(hip_ops_factory, tmp_path, dtype):
    ops = hip_ops_factory(dtype)
    ypath, cpath = reduced_yaml_and_checkpoint(tmp_path, "lightning")
    runner = factory.build_runner(ypath, cpath, ops)
    want = uncond_reference()
    err = ((runner.uncond_text_emb.float().cpu() - want).norm() / want.norm()).item()
    print(f"\n[parity] build_runner: unconditional text tokens {dtype} vs the HF-pinned restatement: rel err {err:.2e}")
    assert err <= FWD_TOL_REDUCED[dtype]
    text, videos, cond_image = runner_inputs("cuda")
    out = runner.image_guided_synthesis(text, videos, cond_image, [1, 4, 16, 8, 8], ddim_steps=2, ddim_eta=0.0,
                                        unconditional_guidance_scale=4.0, fs=15, timestep_spacing="uniform_trailing")
    torch.cuda.synchronize()
    assert out.shape == (1, 1, 3, 16, 64, 64) and bool(torch.isfinite(out).all()) and float(out.float().std()) > 0
    runner.sampler.close()
