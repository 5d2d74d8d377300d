"""OpenCLIP ViT-H/14 text tower of the conditioning tail: drop-in for
lvdm.modules.encoders.condition.FrozenOpenCLIPEmbedder (condition.py:179-239) on the MI355X op table.

The reference builds `open_clip.create_model_and_transforms("ViT-H-14", pretrained="laion2b_s32b_b79k")` (third-party
`open_clip_torch`), deletes the vision transformer and runs the text transformer itself (`encode_with_transformer`,
:219-236): token embedding + positional embedding, the pre-LN residual blocks under the causal `attn_mask` - all of them
(`layer="last"`) or all but the last (`layer="penultimate"`, what the three shipped inference yamls set) - then `ln_final`
on every one of the 77 tokens; no pooling, no `text_projection`.  This module restates that published architecture -
open_clip's `CLIP` text side: width 1024, 24 blocks, nn.MultiheadAttention with 16 heads of 64 channels, MLP 4096 with erf
GELU - with open_clip's parameter names under `model.*`, so the `cond_stage_model.*` tensors of a DynamiCrafter checkpoint
load with `strict=True` (`text_projection` and `logit_scale` are kept for the key set and are not on the path; `attn_mask`
is a non-persistent buffer there and is the kernel's causal flag here).

Graph: ids -> pm_embed_tokens (table row + position, the f32 residual stream) -> per block: LayerNorm, fused in_proj GEMM
(+bias), pm_attention_causal (head dim 64), out_proj GEMM + residual, LayerNorm, c_fc GEMM with the erf-GELU epilogue,
c_proj GEMM + residual -> ln_final.

Text: the only string the denoiser's caller needs is "" (the unconditional prompt of classifier-free guidance,
model.py:723-725), whose open_clip tokenisation is fixed - start token, end token, zero padding - and is produced here.
Any other string needs open_clip's BPE vocabulary, which is not shipped: pass `tokenizer=open_clip.tokenize` (any callable
list[str] -> LongTensor (b, 77)), or hand `forward` the token ids.
"""
import torch
import torch.nn as nn

from . import packing
from .clip_vision import _Transformer

VIT_H_14_TEXT = dict(context_length=77, vocab_size=49408, width=1024, heads=16, layers=24)
SOT_TOKEN, EOT_TOKEN = 49406, 49407  # open_clip.tokenizer: <start_of_text>, <end_of_text>; padding is 0


class _ClipTextShell(nn.Module):
    """open_clip.model.CLIP after `del model.visual`: the text side's parameters, by open_clip's names."""

    def __init__(self, context_length, vocab_size, width, heads, layers, mlp_ratio=4.0, embed_dim=None):
        super().__init__()
        self.context_length, self.vocab_size, self.width, self.heads = context_length, vocab_size, width, heads
        self.token_embedding = nn.Embedding(vocab_size, width)
        self.positional_embedding = nn.Parameter(0.01 * torch.randn(context_length, width))
        self.transformer = _Transformer(width, layers, heads, mlp_ratio)
        self.ln_final = nn.LayerNorm(width)
        self.text_projection = nn.Parameter(width ** -0.5 * torch.randn(width, embed_dim or width))  # (not on this path)
        self.logit_scale = nn.Parameter(torch.ones([]) * 2.6592)                                    # (idem)


class FrozenOpenCLIPEmbedder(packing.PackedWeights, nn.Module):
    LAYERS = ["last", "penultimate"]

    def __init__(self, arch="ViT-H-14", version="laion2b_s32b_b79k", device="cuda", max_length=77, freeze=True, layer="last",
                 text_cfg=None, tokenizer=None):
        super().__init__()
        if arch != "ViT-H-14" and text_cfg is None:
            raise NotImplementedError(f"arch {arch!r}: the shipped configs use ViT-H-14 (pass text_cfg for others)")
        if layer not in self.LAYERS:
            raise NotImplementedError(f"layer={layer!r}: one of {self.LAYERS}")
        self.model = _ClipTextShell(**dict(text_cfg or VIT_H_14_TEXT))
        self.max_length, self.layer, self.layer_idx = max_length, layer, self.LAYERS.index(layer)
        self.tokenizer = tokenizer
        self.ops = None
        self._init_packed()
        if freeze:
            self.eval()
            for p in self.parameters():
                p.requires_grad = False

    def bind(self, ops):
        self.ops = ops
        self.invalidate_packed()
        return self

    def tokenize(self, text):
        """list of strings -> LongTensor (b, context_length).  "" without a vocabulary; anything else through `tokenizer`."""
        text = [text] if isinstance(text, str) else list(text)
        if self.tokenizer is not None:
            return torch.as_tensor(self.tokenizer(text)).long()
        if any(t != "" for t in text):
            raise ValueError("FrozenOpenCLIPEmbedder tokenises only the empty prompt itself (no BPE vocabulary is shipped): "
                             "pass tokenizer=open_clip.tokenize to the constructor, or call it with token ids")
        ids = torch.zeros(len(text), self.model.context_length, dtype=torch.long)
        ids[:, 0], ids[:, 1] = SOT_TOKEN, EOT_TOKEN
        return ids

    def prepare(self):
        ops, m = self.ops, self.model
        dev = ops.device
        wt = lambda t: t.detach().to(device=dev, dtype=ops.dtype).contiguous()
        f32 = lambda t: t.detach().to(device=dev, dtype=torch.float32).contiguous()
        W = {"table": wt(m.token_embedding.weight), "pos": f32(m.positional_embedding),
             "ln_final": (f32(m.ln_final.weight), f32(m.ln_final.bias)), "blocks": []}
        blocks = m.transformer.resblocks
        for blk in blocks[:len(blocks) - self.layer_idx]:  # (condition.py:228-236: "penultimate" stops before the last block)
            W["blocks"].append({"ln1": (f32(blk.ln_1.weight), f32(blk.ln_1.bias)),
                                "qkv": (wt(blk.attn.in_proj_weight), f32(blk.attn.in_proj_bias)),
                                "out": (wt(blk.attn.out_proj.weight), f32(blk.attn.out_proj.bias)),
                                "ln2": (f32(blk.ln_2.weight), f32(blk.ln_2.bias)),
                                "fc": (wt(blk.mlp.c_fc.weight), f32(blk.mlp.c_fc.bias)),
                                "proj": (wt(blk.mlp.c_proj.weight), f32(blk.mlp.c_proj.bias))})
        self._packed = W
        return self

    @torch.no_grad()
    def forward(self, text):
        """list of strings or LongTensor (b, 77) of token ids -> (b, 77, width): ln_final of every token."""
        if self.ops is None:
            raise RuntimeError("FrozenOpenCLIPEmbedder.bind(ops) must be called first (no implicit CPU fallback)")
        ops, W, m = self.ops, self.packed(), self.model
        ids = text if torch.is_tensor(text) else self.tokenize(text)
        if ids.dim() != 2 or ids.shape[1] != m.context_length or ids.dtype != torch.long:
            raise ValueError(f"token ids: want a LongTensor (b, {m.context_length}), got {ids.dtype} {tuple(ids.shape)}")
        B, n, C, heads = ids.shape[0], ids.shape[1], m.width, m.heads
        h = ops.embed_tokens(ids.to(ops.device), W["table"], W["pos"])
        for L in W["blocks"]:
            qkv = ops.gemm(ops.layernorm(h, *L["ln1"]), *L["qkv"]).view(B, n, 3 * C)
            att = ops.attention_causal(qkv[..., :C], qkv[..., C:2 * C], qkv[..., 2 * C:], heads)
            h = ops.gemm(att.view(B * n, C), *L["out"], residual=h, stream=True)
            y = ops.gemm(ops.layernorm(h, *L["ln2"]), *L["fc"], act="gelu")
            h = ops.gemm(y, *L["proj"], residual=h, stream=True)
        return ops.layernorm(h, *W["ln_final"], out=ops.empty(B * n, C)).view(B, n, C)

    def encode(self, text):
        return self(text)
