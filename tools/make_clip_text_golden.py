"""Writes tests/golden/clip_text_hf.npz: the OpenCLIP text tower's outputs as HF `transformers.CLIPTextModel` computes them
(f32, CPU) on seeded weights in open_clip's key layout - the third-party pin of open_pandora_amd.clip_text, as
tests/golden/clip_vision_hf.npz is for the image tower.  Recipe (sizes, seed, prompts, key map): tests/clip_text_ref.py.

  small     width 128, 4 layers, 2 heads: "", an 8-token and a 75-token prompt; `penultimate` and `last`
  vit_h_14  the shipped text tower (width 1024, 24 layers, 16 heads): "" and the 75-token prompt; `penultimate` (what
            the shipped yamls set)
Each record is oracle.golden_recipe.make_digest's: the whole tensor plus its moments and row / column profiles.

    python tools/make_clip_text_golden.py
"""
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import clip_text_ref as ref  # noqa: E402
from oracle import golden_recipe as gr  # noqa: E402
from open_pandora_amd.clip_text import VIT_H_14_TEXT  # noqa: E402


def main():
    import transformers
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    out = {"source": np.array(f"transformers {transformers.__version__} CLIPTextModel: final_layer_norm(hidden_states[-2]) "
                              f"(penultimate), last_hidden_state (last); f32, CPU")}
    for tag, cfg, layers in (("small", ref.SMALL, ("penultimate", "last")), ("vit_h_14", dict(VIT_H_14_TEXT), ("penultimate",))):
        sd = ref.state_dict(cfg)
        ids = ref.prompts(tag)
        t0 = time.time()
        y = ref.hf_forward(ref.hf_text_model(cfg, sd), ids)
        out[f"{tag}/ids"] = ids.numpy()
        for layer in layers:
            print(f"HF CLIPTextModel {tag} {layer}: {time.time() - t0:.1f}s out {tuple(y[layer].shape)} std {y[layer].std():.4f}")
            for k, val in gr.make_digest(y[layer]).items():
                out[f"{tag}/{layer}/{k}"] = val
    np.savez_compressed(ref.GOLDEN, **out)
    print(f"wrote {ref.GOLDEN}: {os.path.getsize(ref.GOLDEN)} bytes")


if __name__ == "__main__":
    main()
