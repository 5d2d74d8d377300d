"""Dump the output of one reduced-width U-Net forward in each precision mode, to compare two trees bit for bit.

Run it in each tree (same script, same GPU), then compare:
    python tools/mode_latents.py --out DIR_A            (in tree A)
    python tools/mode_latents.py --out DIR_B            (in tree B)
    python tools/mode_latents.py --compare DIR_A DIR_B  (lists every mode both trees know; exit status 1 on a difference)
Modes a tree's HipOps does not know (a switch newer than the tree) are skipped there."""
import argparse
import inspect
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

MODES = {"default": {}, "fp8_attention": dict(fp8_attention=True, fp8_min_tokens=0),
         "fp8_linear": dict(fp8_linear=True, fp8_linear_min_rows=0),
         "fp8_linear+fp8_attention": dict(fp8_linear=True, fp8_linear_min_rows=0, fp8_attention=True, fp8_min_tokens=0),
         "fp8_block": dict(fp8_linear=True, fp8_linear_min_rows=0, fp8_attention=True, fp8_min_tokens=0, fp8_block=True)}


def dump(out):
    import torch
    from open_pandora_amd import synth
    from open_pandora_amd.ops_hip import HipOps
    from open_pandora_amd.unet import UNetModel
    known = inspect.signature(HipOps.__init__).parameters
    os.makedirs(out, exist_ok=True)
    kw = dict(in_channels=8, out_channels=4, attention_resolutions=[4, 2, 1], num_res_blocks=2, channel_mult=[1, 2, 4, 4],
              num_head_channels=64, transformer_depth=1, context_dim=1024, use_linear=True, temporal_conv=True,
              temporal_attention=True, temporal_selfatt_only=True, use_relative_position=False, temporal_length=16,
              addition_attention=True, image_cross_attention=True, default_fs=24, fs_condition=True, model_channels=64)
    for dtype in (torch.float16, torch.bfloat16):
        for (h, w) in ((8, 8), (8, 16)):
            ins = synth.synth_inputs(h, w, 16, seed=5)
            x = torch.cat([ins["x_T"], ins["c_concat"]], 1).cuda()
            for name, mode in MODES.items():
                if not set(mode) <= set(known):
                    continue
                m = UNetModel(**kw).eval()
                m.load_state_dict(synth.synth_state_dict(m, seed=11))
                y = m.bind(HipOps(dtype, "cuda:0", **mode))(x, torch.tensor([500]).cuda(), context=ins["c_crossattn"].cuda(),
                                                             fs=torch.tensor([15]).cuda())
                tag = f"{name}_{str(dtype).split('.')[-1]}_{h}x{w}"
                np.save(os.path.join(out, tag + ".npy"), y.float().cpu().numpy())
                print(f"{tag}: |y| = {y.float().norm().item():.6f}", flush=True)


def compare(a, b):
    names = sorted(set(os.listdir(a)) & set(os.listdir(b)))
    bad = 0
    for n in names:
        same = np.array_equal(np.load(os.path.join(a, n)), np.load(os.path.join(b, n)), equal_nan=True)
        bad += not same
        print(f"{n}: {'bit-identical' if same else 'DIFFERENT'}")
    print(f"{len(names)} outputs compared, {bad} differ")
    return 1 if bad or not names else 0


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--compare", nargs=2)
    a = ap.parse_args()
    if a.compare:
        sys.exit(compare(*a.compare))
    dump(a.out)
