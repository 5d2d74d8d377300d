"""MXFP8 ResBlock convolutions (HipOps(fp8_conv=True)) against the 16-bit launches of the same sites, per site and per forward.

Per site (levels 0 and 1 of 320x512 and 576x1024, 16 frames; the 3x3 and the temporal conv, Cin = Cout): GroupNorm-apply + conv on
the 16-bit path (groupnorm_apply -> conv3x3 / conv_t3, stream output) against the new pair (groupnorm_mx8 -> conv3x3_mx8 /
conv_t3_mx8); both start from the same f32 input and its statistics and end with the f32 conv output.  Same process, interleaved,
median of `rounds` rounds of `reps` back-to-back launches (HIP events).  Per forward: the full-width U-Net with the mode off / on.

    python tools/fp8_conv_bench.py [--reps 10] [--rounds 5] [--out profiles/fp8_conv] [--no-forward] [--forward-res 320x512,576x1024]
"""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from open_pandora_amd import build as _b  # noqa: E402
from open_pandora_amd.ops_hip import HipOps  # noqa: E402

# (resolution, level, frames, latent H, latent W, channels)
SITES = [("320x512", 0, 16, 40, 64, 320), ("320x512", 1, 16, 20, 32, 640),
         ("576x1024", 0, 16, 72, 128, 320), ("576x1024", 1, 16, 36, 64, 640)]
LATENT = {"320x512": (40, 64), "576x1024": (72, 128)}


def burst_ms(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def interleaved(fns, reps, rounds):
    """median over rounds of each function's burst time, the functions taking turns inside every round"""
    for fn in fns:
        fn()
    torch.cuda.synchronize()
    t = [[] for _ in fns]
    for _ in range(rounds):
        for i, fn in enumerate(fns):
            t[i].append(burst_ms(fn, reps))
    return [statistics.median(x) for x in t]


def site_table(reps, rounds):
    ops = HipOps(torch.bfloat16, "cuda:0", fp8_conv=True)
    dev, rows = "cuda:0", []
    for res, lv, F, H, W, C in SITES:
        torch.manual_seed(lv)
        M = F * H * W
        x = torch.randn(M, C, device=dev)
        g, b, bias = torch.ones(C, device=dev), torch.zeros(C, device=dev), torch.zeros(C, device=dev)
        out = torch.empty(M, C, device=dev)
        for kind, taps in (("conv3x3", 9), ("conv_t3", 3)):
            w16 = (0.02 * torch.randn(C, taps * C, device=dev)).to(torch.bfloat16)
            wmx = ops.quant_mx8(w16)
            NI = F if kind == "conv3x3" else 1  # per-frame statistics in front of the 3x3, (T, H, W) in front of the temporal conv
            tot = ops.groupnorm_stats(x, NI)
            if kind == "conv3x3":
                f16 = lambda: ops.conv3x3(ops.groupnorm_apply(x, tot, g, b, 1e-5, NI, True), w16, bias, F, H, W, stream=True, out=out)
                fmx = lambda: ops.conv3x3_mx8(ops.groupnorm_mx8(x, g, b, 1e-5, NI, True, totals=tot), wmx, bias, F, H, W, out=out)
            else:
                f16 = lambda: ops.conv_t3(ops.groupnorm_apply(x, tot, g, b, 1e-5, NI, True), w16, bias, F, H * W, stream=True, out=out)
                fmx = lambda: ops.conv_t3_mx8(ops.groupnorm_mx8(x, g, b, 1e-5, NI, True, totals=tot), wmx, bias, F, H * W, out=out)
            t16, tmx = interleaved([f16, fmx], reps, rounds)
            flops = 2 * M * C * taps * C
            rows.append((res, lv, kind, M, C, t16, tmx))
            print(f"{res:>8} L{lv} {kind:>7} M={M:>6} C={C:>4}: bf16 {t16 * 1e3:8.1f} us  mxfp8 {tmx * 1e3:8.1f} us  x{t16 / tmx:5.2f}  "
                  f"({flops / t16 / 1e9:6.0f} / {flops / tmx / 1e9:6.0f} TFLOP/s incl. the GroupNorm pass)", flush=True)
            del w16, wmx
        del x, out
        torch.cuda.empty_cache()
    return rows


def forward_table(resolutions, reps, rounds):
    from oracle import golden_recipe as gr
    from open_pandora_amd import factory
    out = []
    for res in resolutions:
        h, w = LATENT[res]
        off, on = HipOps(torch.bfloat16, "cuda:0"), HipOps(torch.bfloat16, "cuda:0", fp8_conv=True)
        pm = factory.build_diffusion(res, off, seed=gr.WEIGHT_SEED)
        ins, cond, _ = gr.sampler_inputs(h, w)
        c = {k: [t.cuda() for t in v] for k, v in cond.items()}
        args = (ins["x_T"].cuda(), torch.tensor([500]).cuda(), c)
        fs = torch.tensor([15]).cuda()
        unet = pm.model.diffusion_model
        fwd = lambda: pm.apply_model(*args, fs=fs)
        t = {False: [], True: []}
        for _ in range(rounds):  # (a re-bind re-packs the weights: outside the timed bursts)
            for on_, ops in ((False, off), (True, on)):
                unet.bind(ops)
                fwd()
                torch.cuda.synchronize()
                t[on_].append(burst_ms(fwd, reps))
        t_off, t_on = statistics.median(t[False]), statistics.median(t[True])
        out.append((res, t_off, t_on))
        print(f"{res} forward bf16: fp8_conv off {t_off:7.2f} ms, on {t_on:7.2f} ms", flush=True)
        del pm, unet
        torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fp8_conv"))
    ap.add_argument("--no-forward", action="store_true")
    ap.add_argument("--forward-res", default="320x512")
    a = ap.parse_args()
    os.makedirs(a.out, exist_ok=True)
    head = f"# tools/fp8_conv_bench.py --reps {a.reps} --rounds {a.rounds}; library sources digest {_b.sources_digest()[:16]}\n"
    rows = site_table(a.reps, a.rounds)
    with open(os.path.join(a.out, "site_times.txt"), "w") as f:
        f.write(head + "# per ResBlock conv site (Cin = Cout = C, 16 frames): GroupNorm-apply + SiLU + conv, 16-bit path (groupnorm_apply +\n"
                "# conv3x3 / conv_t3) against the MXFP8 pair (groupnorm_mx8 + conv3x3_mx8 / conv_t3_mx8); median burst times\n"
                "res level site M C bf16_us mxfp8_us speedup\n")
        for res, lv, kind, M, C, t16, tmx in rows:
            f.write(f"{res} {lv} {kind} {M} {C} {t16 * 1e3:.1f} {tmx * 1e3:.1f} {t16 / tmx:.2f}\n")
    if not a.no_forward:
        fw = forward_table(a.forward_res.split(","), max(2, a.reps // 3), a.rounds)
        with open(os.path.join(a.out, "forward_times.txt"), "w") as f:
            f.write(head + "# one full-width U-Net forward (bf16, 16 frames), eager, default fp8_conv_min_rows; median burst times\n"
                    "res fp8_conv_off_ms fp8_conv_on_ms\n")
            for res, t_off, t_on in fw:
                f.write(f"{res} {t_off:.2f} {t_on:.2f}\n")


if __name__ == "__main__":
    main()
