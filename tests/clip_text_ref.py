"""Test infrastructure (not product code): CPU f32 restatement of the OpenCLIP text tower as FrozenOpenCLIPEmbedder runs it
(condition.py:179-239), functional over a state_dict with open_clip's key names under `model.`, the CPU op table extended by
the two ops the tower adds, and the recipe (sizes, seed, prompts, HF key map) shared by tools/make_clip_text_golden.py and
the tests.

PARITY: open_clip_torch is a third-party package absent here; the restatement is pinned against HF
`transformers.CLIPTextModel` - a third-party implementation of the same architecture - on seeded weights in open_clip's
key layout (tests/golden/clip_text_hf.npz, 2e-5).  The reference's `layer="penultimate"` output (all blocks but the last,
then ln_final) is HF's `final_layer_norm(hidden_states[-2])`; `layer="last"` is `last_hidden_state`.
"""
import os

import numpy as np
import torch
import torch.nn.functional as F

from oracle.ops_torch import TorchOps, _f
from open_pandora_amd import synth

try:  # at import (test collection): transformers resolves its optional dependencies lazily, and oracle/ref_harness.py later
    # puts spec-less stand-ins for some of them (torchvision) into sys.modules, after which these classes no longer import
    from transformers import CLIPTextConfig, CLIPTextModel
except Exception:  # not installed, or not importable: the fixture checks stand, the live comparison is skipped
    CLIPTextConfig = CLIPTextModel = None

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "clip_text_hf.npz")
SEED = 11
SMALL = dict(context_length=77, vocab_size=49408, width=128, heads=2, layers=4)  # head dim 64, as the shipped tower
SOT, EOT = 49406, 49407
LAYER_IDX = {"last": 0, "penultimate": 1}


def prompt_ids(n_tokens, name, vocab=49408):
    """open_clip.tokenize's layout for a prompt of `n_tokens` BPE tokens: start, the tokens, end, ZERO padding, 77 wide.
    The tokens are seeded ids in [1, SOT): what they spell does not matter to the arithmetic."""
    ids = torch.zeros(77, dtype=torch.long)
    body = ((synth.uniform_pm1(n_tokens, SEED, f"clip_text/{name}") + 1.0) * 0.5 * (min(vocab, SOT) - 2)).long() + 1
    ids[0], ids[1:1 + n_tokens], ids[1 + n_tokens] = SOT, body, EOT
    return ids


def prompts(tag):
    """small: "", 8 tokens, 75 tokens (the longest that fits); full: "" and 75 tokens."""
    rows = [prompt_ids(0, "empty")] + ([prompt_ids(8, "p8")] if tag == "small" else []) + [prompt_ids(75, "p75")]
    return torch.stack(rows)


def shapes(cfg):
    from open_pandora_amd.clip_text import FrozenOpenCLIPEmbedder
    with torch.device("meta"):
        return {k: tuple(v.shape) for k, v in FrozenOpenCLIPEmbedder(text_cfg=cfg).state_dict().items()}


def state_dict(cfg, device="cpu"):
    return {k: synth.synth_tensor(k, s, SEED, device) for k, s in shapes(cfg).items()}


def _ln(sd, p, x):
    return F.layer_norm(x, (x.shape[-1],), sd[p + ".weight"].float(), sd[p + ".bias"].float(), 1e-5)


def text_tower_forward(sd, ids, heads, layer="penultimate", causal=True):
    """ids LongTensor (b, n) -> (b, n, width).  causal=False drops the mask (the tests show how far that moves the result)."""
    m = "model."
    x = sd[m + "token_embedding.weight"].float()[ids] + sd[m + "positional_embedding"].float()
    depth = 1 + max(int(k.split(".")[3]) for k in sd if k.startswith(m + "transformer.resblocks."))
    b, n, c = x.shape
    d = c // heads
    mask = torch.full((n, n), float("-inf")).triu(1) if causal else torch.zeros(n, n)
    for i in range(depth - LAYER_IDX[layer]):
        p = f"{m}transformer.resblocks.{i}."
        y = _ln(sd, p + "ln_1", x)
        qkv = y @ sd[p + "attn.in_proj_weight"].float().t() + sd[p + "attn.in_proj_bias"].float()
        q, k, val = (t.reshape(b, n, heads, d).transpose(1, 2) for t in qkv.chunk(3, -1))
        att = torch.softmax((q * d ** -0.5) @ k.transpose(-1, -2) + mask, -1) @ val
        att = att.transpose(1, 2).reshape(b, n, c)
        x = x + att @ sd[p + "attn.out_proj.weight"].float().t() + sd[p + "attn.out_proj.bias"].float()
        y = _ln(sd, p + "ln_2", x)
        y = F.gelu(y @ sd[p + "mlp.c_fc.weight"].float().t() + sd[p + "mlp.c_fc.bias"].float())
        x = x + y @ sd[p + "mlp.c_proj.weight"].float().t() + sd[p + "mlp.c_proj.bias"].float()
    return _ln(sd, m + "ln_final", x)


def hf_key_map(sd, layers, width):
    """open_clip keys -> HF CLIPTextModel keys (`text_projection` / `logit_scale` have no counterpart there)."""
    m = "model."
    out = {"text_model.embeddings.token_embedding.weight": sd[m + "token_embedding.weight"],
           "text_model.embeddings.position_embedding.weight": sd[m + "positional_embedding"],
           "text_model.final_layer_norm.weight": sd[m + "ln_final.weight"],
           "text_model.final_layer_norm.bias": sd[m + "ln_final.bias"]}
    for i in range(layers):
        a, b = f"{m}transformer.resblocks.{i}.", f"text_model.encoder.layers.{i}."
        w, bias = sd[a + "attn.in_proj_weight"], sd[a + "attn.in_proj_bias"]
        for j, n in enumerate(("q_proj", "k_proj", "v_proj")):
            out[f"{b}self_attn.{n}.weight"], out[f"{b}self_attn.{n}.bias"] = w[j * width:(j + 1) * width], bias[j * width:(j + 1) * width]
        for src, dst in (("attn.out_proj", "self_attn.out_proj"), ("ln_1", "layer_norm1"), ("ln_2", "layer_norm2"),
                         ("mlp.c_fc", "mlp.fc1"), ("mlp.c_proj", "mlp.fc2")):
            out[f"{b}{dst}.weight"], out[f"{b}{dst}.bias"] = sd[a + src + ".weight"], sd[a + src + ".bias"]
    return out


def hf_text_model(cfg, sd):
    """HF transformers' CLIPTextModel holding `sd` (erf GELU as open_clip's nn.GELU, eps 1e-5)."""
    C, L = cfg["width"], cfg["layers"]
    hf = CLIPTextModel(CLIPTextConfig(vocab_size=cfg["vocab_size"], hidden_size=C, intermediate_size=4 * C, num_hidden_layers=L,
                                      num_attention_heads=cfg["heads"], max_position_embeddings=cfg["context_length"],
                                      hidden_act="gelu", layer_norm_eps=1e-5, attention_dropout=0.0, projection_dim=C,
                                      pad_token_id=0, bos_token_id=SOT, eos_token_id=EOT)).eval()
    m = hf_key_map(sd, L, C)
    have = {k for k in hf.state_dict() if not k.endswith("position_ids")}
    if not any(k.startswith("text_model.") for k in have):  # (a transformers without the wrapper level)
        m = {k[len("text_model."):]: v for k, v in m.items()}
    assert set(m) == have, sorted(set(m) ^ have)[:6]
    missing, unexpected = hf.load_state_dict(m, strict=False)
    assert not unexpected and all(k.endswith("position_ids") for k in missing), (missing, unexpected)
    return hf


@torch.no_grad()
def hf_forward(hf, ids):
    """-> {"penultimate", "last"}: final_layer_norm(hidden_states[-2]) and last_hidden_state."""
    out = hf(input_ids=ids, output_hidden_states=True)
    ln = (hf.text_model if hasattr(hf, "text_model") else hf).final_layer_norm
    return {"penultimate": ln(out.hidden_states[-2]), "last": out.last_hidden_state}


def load_golden():
    return np.load(GOLDEN)


class TextTorchOps(TorchOps):
    """The CPU op table + the two ops of the text tower, for host-graph tests."""

    def attention_causal(self, q, k, v, heads, q_pos0=0, out=None):
        B, Nq, C = q.shape
        Nk, D = k.shape[1], C // heads
        if q_pos0 < 0 or q_pos0 + Nq > Nk:
            raise ValueError("pm_attention_causal: shape or alignment precondition violated")
        sp = lambda t: _f(t).reshape(t.shape[0], t.shape[1], heads, D).permute(0, 2, 1, 3)
        hidden = torch.arange(Nk)[None, :] > q_pos0 + torch.arange(Nq)[:, None]
        s = (sp(q) @ sp(k).transpose(-1, -2) * D ** -0.5).masked_fill(hidden, float("-inf"))
        return self._out((torch.softmax(s, -1) @ sp(v)).permute(0, 2, 1, 3).reshape(B, Nq, C), out)

    def embed_tokens(self, ids, table, pos, out=None):
        V = table.shape[0]
        if int(ids.min()) < 0 or int(ids.max()) >= V:
            raise ValueError(f"embed_tokens: token ids outside [0, {V})")
        y = (_f(table)[ids] + _f(pos)).reshape(-1, table.shape[1])
        if out is not None:
            out.copy_(y)
            return out
        return y
