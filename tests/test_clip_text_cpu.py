"""CPU: the OpenCLIP text tower (open_pandora_amd.clip_text) - the restatement (tests/clip_text_ref.py) against the fixture of
HF transformers' CLIPTextModel (tests/golden/clip_text_hf.npz, tools/make_clip_text_golden.py) and against the live HF
model, the product graph on the CPU op table against the same fixture, the key set, the tokenisation of "", and
factory.build_runner: a yaml plus a checkpoint in, a DiffusionRunner with the tower behind its empty prompt out."""
import pytest
import torch
import yaml

import clip_text_ref as ref
from oracle import golden_recipe as gr
from open_pandora_amd import checkpoint, factory, synth
from open_pandora_amd.clip_text import VIT_H_14_TEXT, FrozenOpenCLIPEmbedder
from test_oracle_golden import RH_KW

TOL = 2e-5  # the project's bound for a restatement against its third-party pin (the vision tower's)


def _rel(a, b):
    return ((a.double() - b.double()).norm() / b.double().norm()).item()


def _tower(cfg, layer, sd, ops=None):
    m = FrozenOpenCLIPEmbedder(text_cfg=cfg, layer=layer)
    m.load_state_dict(sd, strict=True)
    return m.bind(ops or ref.TextTorchOps())


def test_restatement_against_the_hf_fixture_small_and_full():
    g = ref.load_golden()
    assert "CLIPTextModel" in str(g["source"])
    sd = ref.state_dict(ref.SMALL)
    ids = ref.prompts("small")
    assert torch.equal(ids, torch.as_tensor(g["small/ids"])) and ids[0].tolist() == [49406, 49407] + [0] * 75
    for layer in ("penultimate", "last"):
        y = ref.text_tower_forward(sd, ids, ref.SMALL["heads"], layer)
        err = gr.compare_digest(y, g, f"small/{layer}", TOL)[0]
        assert err < TOL, (layer, err)
    # the shipped size on "" (row 0 of the record; the 75-token row runs on the GPU)
    cfg = dict(VIT_H_14_TEXT)
    y = ref.text_tower_forward(ref.state_dict(cfg), ref.prompts("vit_h_14")[:1], cfg["heads"], "penultimate")
    want = torch.as_tensor(g["vit_h_14/penultimate/full"])[:1]
    assert y.shape == (1, 77, 1024) and _rel(y, want) < TOL
    # what a wrong tower would do: no mask, or the other layer (far outside any tolerance used for this module)
    y_pen = torch.as_tensor(g["small/penultimate/full"])
    assert _rel(ref.text_tower_forward(sd, ids, ref.SMALL["heads"], "penultimate", causal=False), y_pen) > 0.1
    assert _rel(torch.as_tensor(g["small/last/full"]), y_pen) > 0.1


def test_restatement_against_the_live_hf_model():
    if ref.CLIPTextModel is None:
        pytest.skip("transformers' CLIPTextModel does not import here: the fixture checks stand")
    sd, ids = ref.state_dict(ref.SMALL), ref.prompts("small")
    hf = ref.hf_forward(ref.hf_text_model(ref.SMALL, sd), ids)
    for layer in ("penultimate", "last"):
        err = _rel(ref.text_tower_forward(sd, ids, ref.SMALL["heads"], layer), hf[layer])
        assert err < TOL, (layer, err)


def test_product_graph_on_the_cpu_op_table_and_layers():
    g = ref.load_golden()
    sd, ids = ref.state_dict(ref.SMALL), ref.prompts("small")
    got = {layer: _tower(ref.SMALL, layer, sd)(ids) for layer in ("penultimate", "last")}
    for layer, y in got.items():
        assert y.shape == (3, 77, 128)
        assert gr.compare_digest(y, g, f"small/{layer}", TOL)[0] < TOL  # each matches its own record
    assert _rel(got["last"], got["penultimate"]) > 0.1
    m = _tower(ref.SMALL, "penultimate", sd)
    assert torch.equal(m.encode([""]), got["penultimate"][:1])       # "" = row 0, through the in-module tokenisation
    with pytest.raises(RuntimeError, match="bind"):
        FrozenOpenCLIPEmbedder(text_cfg=ref.SMALL)(ids)               # no op table: loud, no eager fallback
    with pytest.raises(ValueError, match="token ids"):
        m.ops.embed_tokens(torch.tensor([[0, 49408]]), torch.zeros(49408, 8), torch.zeros(2, 8))


def test_state_dict_keys_and_a_full_size_checkpoint_loads_strictly():
    with torch.device("meta"):
        m = FrozenOpenCLIPEmbedder(layer="penultimate")
    sd = m.state_dict()
    assert sd["model.token_embedding.weight"].shape == (49408, 1024) and sd["model.positional_embedding"].shape == (77, 1024)
    assert sd["model.transformer.resblocks.23.attn.in_proj_weight"].shape == (3072, 1024)
    assert sd["model.transformer.resblocks.0.mlp.c_fc.weight"].shape == (4096, 1024)
    assert sd["model.text_projection"].shape == (1024, 1024) and sd["model.logit_scale"].shape == ()
    cfg = dict(VIT_H_14_TEXT)
    shapes = ref.shapes(cfg)
    used = set()

    class Recording(dict):
        def __getitem__(self, k):
            used.add(k)
            return torch.empty(3 * 8, 8)

    mapped = ref.hf_key_map(Recording(), cfg["layers"], 8)
    # the HF model's parameters (4 + 16 per layer) draw on every key but the two off-path ones
    assert len(mapped) == 4 + 16 * cfg["layers"] and used == set(shapes) - {"model.text_projection", "model.logit_scale"}
    assert len(shapes) == 2 + 2 + 2 + 24 * 12 and set(sd) == set(shapes)
    # `cond_stage_model.*` of a synthetic full-size checkpoint, among the other prefixes, in two wire formats
    meta = {k: torch.empty(s, device="meta") for k, s in shapes.items()}
    for blob in ({"state_dict": {**{"cond_stage_model." + k: v for k, v in meta.items()}, "embedder.model.logit_scale": meta["model.logit_scale"],
                                 "model.diffusion_model.out.2.bias": torch.zeros(4)}},
                 {**{"diffusion_model.cond_stage_model." + k: v for k, v in meta.items()}, "video_model.lm_head.weight": torch.zeros(2, 2)}):
        res = checkpoint.load_text_tower(m, blob, strict=True)
        assert not res.missing_keys and not res.unexpected_keys


def test_tokenisation_of_the_empty_prompt():
    m = FrozenOpenCLIPEmbedder(text_cfg=ref.SMALL)
    ids = m.tokenize([""])
    assert ids.dtype == torch.long and ids.tolist() == [[49406, 49407] + [0] * 75]
    assert m.tokenize(["", ""]).shape == (2, 77)
    with pytest.raises(ValueError, match="tokenizer"):
        m.tokenize(["a photo of a cat"])
    with pytest.raises(ValueError, match="tokenizer"):
        m.bind(ref.TextTorchOps())(["", "a photo of a cat"])
    tok = lambda texts: ref.prompts("small")[:len(texts)]
    assert torch.equal(FrozenOpenCLIPEmbedder(text_cfg=ref.SMALL, tokenizer=tok).tokenize(["x", "y"]), ref.prompts("small")[:2])


@pytest.mark.parametrize("D", [64, 80])
def test_causal_exact_construction_on_the_cpu_op_table(D):
    """tests/attn_causal_exact.py, the operands of the GPU test of pm_attention_causal: the closed form equals a masked softmax
    attention bit for bit, an unmasked one returns the mean over the visible AND the future match, and every instance has rows
    with one visible + one future match and rows whose only visible match is key q_pos0 + i."""
    import attn_causal_exact as cx
    ops = ref.TextTorchOps()
    for Nq, Nk, p0 in cx.CASES:
        for dtype in (torch.float16, torch.bfloat16):
            d = cx.build(Nq, Nk, p0, D, dtype)
            got = ops.attention_causal(d["q"], d["k"], d["v"], cx.HEADS, q_pos0=p0)
            assert torch.equal(got.to(dtype), d["want"]), (Nq, Nk, p0, dtype)
            k, v = d["k"], d["v"]
            free = ops.attention_generic(d["q"], k, v, cx.HEADS)
            assert torch.equal(free.to(dtype), d["unmasked"]) and not torch.equal(d["unmasked"], d["want"])
            cov = cx.coverage(d, Nq, p0)
            assert all(both >= 1 and edge >= 1 for both, edge in cov), (Nq, Nk, p0, cov)
            assert sum(both for both, _ in cov) >= (Nq - 1) * cx.B * cx.HEADS // 2
        with pytest.raises(ValueError, match="shape"):
            ops.attention_causal(d["q"], d["k"], d["v"], cx.HEADS, q_pos0=Nk - Nq + 1)
    with pytest.raises(ValueError, match="shape"):
        ops.attention_causal(d["q"], d["k"], d["v"], cx.HEADS, q_pos0=-1)


# ---- factory.build_runner -----------------------------------------------------------------------------------------------------
VISION_SMALL = dict(gr.CLIP_SMALL)
RESAMPLER_SMALL = dict(dim=128, depth=2, dim_head=64, heads=2, num_queries=16, embedding_dim=VISION_SMALL["width"],
                       output_dim=128, ff_mult=4, video_length=16)


def reduced_yaml_and_checkpoint(tmp_path, fmt):
    """A reduced `inference_512_v1.0.yaml` (U-Net 64 base channels over 128-wide context tokens, the reduced CLIP towers, a
    small Resampler and AutoencoderKL) and a synthetic checkpoint carrying all five prefixes, written to `tmp_path` in the
    `lightning` (`model.ckpt`) or `pandora` (`pytorch_model.bin`) wire format.  -> (yaml path, checkpoint path)."""
    from open_pandora_amd.autoencoder import DDCONFIG, AutoencoderKL
    from open_pandora_amd.clip_vision import FrozenOpenCLIPImageEmbedderV2
    from open_pandora_amd.resampler import Resampler
    from open_pandora_amd.unet import UNetModel
    unet_kw = dict(RH_KW, model_channels=64, context_dim=128)
    dd = dict(DDCONFIG, ch=32)
    dd = {k: (list(v) if isinstance(v, tuple) else v) for k, v in dd.items()}
    t = "lvdm.modules.encoders"
    params = dict(rescale_betas_zero_snr=True, parameterization="v", linear_start=0.00085, linear_end=0.012, timesteps=1000,
                  conditioning_key="hybrid", image_size=[8, 8], channels=4, scale_factor=0.18215, uncond_type="empty_seq",
                  use_dynamic_rescale=True, base_scale=0.7, fps_condition_type="fps", perframe_ae=True,
                  unet_config=dict(target="lvdm.modules.networks.openaimodel3d.UNetModel", params=unet_kw),
                  first_stage_config=dict(target="lvdm.models.autoencoder.AutoencoderKL",
                                          params=dict(embed_dim=4, monitor="val/rec_loss", ddconfig=dd,
                                                      lossconfig=dict(target="torch.nn.Identity"))),
                  cond_stage_config=dict(target=t + ".condition.FrozenOpenCLIPEmbedder",
                                         params=dict(freeze=True, layer="penultimate", text_cfg=dict(ref.SMALL))),
                  img_cond_stage_config=dict(target=t + ".condition.FrozenOpenCLIPImageEmbedderV2",
                                             params=dict(freeze=True, vision_cfg=VISION_SMALL)),
                  image_proj_stage_config=dict(target=t + ".resampler.Resampler", params=RESAMPLER_SMALL))
    ypath = tmp_path / "inference_reduced.yaml"
    ypath.write_text(yaml.safe_dump(dict(model=dict(target="lvdm.models.ddpm3d.LatentVisualDiffusion", params=params))))
    with torch.device("meta"):
        mods = {"model.diffusion_model.": UNetModel(**unet_kw), "first_stage_model.": AutoencoderKL(ddconfig=dd),
                "embedder.": FrozenOpenCLIPImageEmbedderV2(vision_cfg=VISION_SMALL), "image_proj_model.": Resampler(**RESAMPLER_SMALL)}
    sd = {"cond_stage_model." + k: v for k, v in ref.state_dict(ref.SMALL).items()}
    for prefix, m in mods.items():
        sd.update({prefix + k: v for k, v in synth.synth_state_dict({k: tuple(v.shape) for k, v in m.state_dict().items()},
                                                                    seed=gr.WEIGHT_SEED).items()})
    sd["embedder.model.logit_scale"] = torch.zeros(())  # (a text-side leftover the reference's image embedder keeps)
    sd["scale_arr"] = torch.zeros(3)
    if fmt == "lightning":
        cpath, blob = tmp_path / "model.ckpt", {"state_dict": sd}
    else:
        cpath, blob = tmp_path / "pytorch_model.bin", {**{"diffusion_model." + k: v for k, v in sd.items()},
                                                       "video_model.lm_head.weight": torch.zeros(2, 2)}
    torch.save(blob, cpath)
    return str(ypath), str(cpath)


def runner_inputs(device="cpu"):
    text = gr.module_input("clip_text/cond", 1, 77, 128).to(device)
    videos = gr.uniform_image(1, 64, 64, "clip_text/frame").reshape(1, 3, 1, 64, 64).to(device)
    return text, videos, gr.uniform_image(1, 64, 64, "clip_text/cond_image").to(device)


def uncond_reference():
    """The restatement on "" with the checkpoint's text weights - itself pinned to row 0 of the HF record."""
    y = ref.text_tower_forward(ref.state_dict(ref.SMALL), ref.prompts("small")[:1], ref.SMALL["heads"], "penultimate")
    assert _rel(y, torch.as_tensor(ref.load_golden()["small/penultimate/full"])[:1]) < TOL
    return y


@pytest.mark.parametrize("fmt", ["lightning", "pandora"])
def test_build_runner_from_yaml_and_checkpoint(tmp_path, fmt):
    torch.set_num_threads(4)
    ypath, cpath = reduced_yaml_and_checkpoint(tmp_path, fmt)
    runner = factory.build_runner(ypath, cpath, ref.TextTorchOps())
    pm = runner.diffusion_model
    tower = pm.cond_stage_model
    assert isinstance(tower, FrozenOpenCLIPEmbedder) and tower.layer == "penultimate"
    assert pm.first_stage_model is not None and pm.embedder is not None and pm.image_proj_model is not None
    assert not any(k.startswith(("cond_stage_model", "embedder", "image_proj_model", "first_stage_model")) for k in pm.state_dict())
    calls = []
    inner = tower.forward
    tower.forward = lambda text: (calls.append(text), inner(text))[1]
    assert not calls                                                   # lazy: nothing ran at build time
    text, videos, cond_image = runner_inputs()
    kw = dict(ddim_steps=2, ddim_eta=0.0, unconditional_guidance_scale=4.0, fs=15, timestep_spacing="uniform_trailing")
    out = runner.image_guided_synthesis(text, videos, cond_image, [1, 4, 16, 8, 8], **kw)
    assert out.shape == (1, 1, 3, 16, 64, 64) and bool(torch.isfinite(out).all()) and float(out.std()) > 0
    assert calls == [[""]]
    runner.image_guided_synthesis(text, videos, cond_image, [1, 4, 16, 8, 8], **kw)
    assert calls == [[""]]                                             # computed once, cached
    assert _rel(runner.uncond_text_emb, uncond_reference()) < TOL
    assert torch.equal(pm.get_learned_conditioning([""]), runner.uncond_text_emb)
    # a tensor keeps working as before, and the checkpoint may be an already loaded object
    r2 = factory.build_runner(ypath, torch.load(cpath), ref.TextTorchOps(), decode=False)
    r2.uncond_text_emb = runner.uncond_text_emb
    lat = r2.image_guided_synthesis(text, videos, cond_image, [1, 4, 16, 8, 8], **kw)
    assert lat.shape == (1, 1, 4, 16, 8, 8) and r2.uncond_text_emb is runner.uncond_text_emb


def test_shell_without_attachments_is_unchanged():
    from open_pandora_amd.ddpm import LatentVisualDiffusion
    from open_pandora_amd.unet import UNetModel
    with torch.device("meta"):
        unet = UNetModel(**dict(RH_KW, model_channels=64))
    pm = LatentVisualDiffusion(unet)
    keys = set(pm.state_dict())
    assert keys == {"model.diffusion_model." + k for k in unet.state_dict()} | {
        "betas", "alphas_cumprod", "alphas_cumprod_prev", "sqrt_alphas_cumprod", "sqrt_one_minus_alphas_cumprod",
        "log_one_minus_alphas_cumprod", "sqrt_recip_alphas_cumprod", "sqrt_recipm1_alphas_cumprod", "scale_arr"}
    assert not hasattr(pm, "cond_stage_model") and not hasattr(pm, "first_stage_model")
    with pytest.raises(RuntimeError, match="cond_stage_model"):
        pm.get_learned_conditioning([""])
    pm.attach_conditioners(cond_stage_model=FrozenOpenCLIPEmbedder(text_cfg=ref.SMALL))
    assert set(pm.state_dict()) == keys and pm.cond_stage_model.layer == "last"
