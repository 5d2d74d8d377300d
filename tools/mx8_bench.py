"""MXFP8 projections (HipOps(fp8_linear=True)) against today's 16-bit launches, per transformer-block site and per forward.

Per site: the bf16 launch(es) the default mode runs (ln_gemm / gemm) against the MXFP8 launches of the same site, quantisation
passes included (LayerNorm-fused quantiser + pm_gemm_mx8 for q|k|v, attn2 q and ff1; quantiser + pm_gemm_mx8 for to_out; ff2
alone, its A operand coming from ff1's MXFP8 output).  Per forward: the full-width 320x512 U-Net with fp8_linear off / on x
fp8_attention off / on.  Random data, HIP events over `reps` back-to-back launches, interleaved in one process.

    python tools/mx8_bench.py [--reps 20] [--out profiles/mx8] [--no-forward]
"""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from open_pandora_amd.ops_hip import HipOps  # noqa: E402

# (resolution, level, tokens = 16 frames x latent pixels, channels) of the levels that carry transformer blocks
LEVELS = [("320x512", 0, 16 * 40 * 64, 320), ("320x512", 1, 16 * 20 * 32, 640), ("320x512", 2, 16 * 10 * 16, 1280),
          ("576x1024", 0, 16 * 72 * 128, 320), ("576x1024", 1, 16 * 36 * 64, 640), ("576x1024", 2, 16 * 18 * 32, 1280)]


def time_ms(fn, reps):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def site_table(reps):
    ops = HipOps(torch.bfloat16, "cuda:0", fp8_linear=True)
    dev = "cuda:0"
    rows = []
    for res, lv, M, C in LEVELS:
        torch.manual_seed(lv)
        h = torch.randn(M, C, device=dev)
        g, b = torch.ones(C, device=dev), torch.zeros(C, device=dev)
        w = lambda n, k: (0.02 * torch.randn(n, k, device=dev)).to(torch.bfloat16)
        wqkv, wo, wf1, wf2 = w(3 * C, C), w(C, C), w(8 * C, C), w(C, 4 * C)
        bo, bf1, bf2 = torch.zeros(C, device=dev), torch.zeros(8 * C, device=dev), torch.zeros(C, device=dev)
        qs = torch.ones(3 * C, device=dev)
        mq = {k: ops.quant_mx8(v) for k, v in (("qkv", wqkv), ("o", wo), ("f1", wf1), ("f2", wf2))}
        a16 = torch.randn(M, C, device=dev).to(torch.bfloat16)
        g16 = torch.randn(M, 4 * C, device=dev).to(torch.bfloat16)
        gmx = ops.quant_mx8(g16)
        flops = {"qkv": 2 * M * 3 * C * C, "out": 2 * M * C * C, "ff1": 2 * M * 8 * C * C, "ff2": 2 * M * 4 * C * C}
        sites = {
            "qkv": (lambda: ops.ln_gemm(h, g, b, wqkv, col_scale=qs),
                    lambda: ops.gemm_mx8(ops.ln_quant_mx8(h, g, b), mq["qkv"], col_scale=qs)),
            "out": (lambda: ops.gemm(a16, wo, bo, residual=h, stream=True),
                    lambda: ops.gemm_mx8(ops.quant_mx8(a16), mq["o"], bo, residual=h, stream=True)),
            "ff1": (lambda: ops.ln_gemm(h, g, b, wf1, bf1, act="geglu"),
                    lambda: ops.gemm_mx8(ops.ln_quant_mx8(h, g, b), mq["f1"], bf1, act="geglu", mx_out=True)),
            "ff2": (lambda: ops.gemm(g16, wf2, bf2, residual=h),
                    lambda: ops.gemm_mx8(gmx, mq["f2"], bf2, residual=h)),
        }
        for name, (f16, fmx) in sites.items():
            t16, tmx = time_ms(f16, reps), time_ms(fmx, reps)
            rows.append((res, lv, name, M, C, t16, tmx, flops[name]))
            print(f"{res:>8} L{lv} {name:>4} M={M:>6} C={C:>4}: bf16 {t16 * 1e3:8.1f} us  mxfp8 {tmx * 1e3:8.1f} us  "
                  f"x{t16 / tmx:5.2f}  ({flops[name] / tmx / 1e9:6.0f} TFLOP/s mx incl. quantisation)", flush=True)
        del h, a16, g16, gmx, mq
        torch.cuda.empty_cache()
    return rows


def forward_table(reps):
    from oracle import golden_recipe as gr
    from open_pandora_amd import factory
    base = HipOps(torch.bfloat16, "cuda:0")
    pm = factory.build_diffusion("320x512", base, seed=gr.WEIGHT_SEED)
    ins, cond, _ = gr.sampler_inputs(40, 64)
    c = {k: [t.cuda() for t in v] for k, v in cond.items()}
    args = (ins["x_T"].cuda(), torch.tensor([500]).cuda(), c)
    fs = torch.tensor([15]).cuda()
    out = []
    for fl in (False, True):
        for fa in (False, True):
            ops = HipOps(torch.bfloat16, "cuda:0", fp8_linear=fl, fp8_attention=fa)
            pm.model.diffusion_model.bind(ops)
            t = time_ms(lambda: pm.apply_model(*args, fs=fs), reps)
            out.append((fl, fa, t))
            print(f"320x512 forward bf16 fp8_linear={fl!s:5} fp8_attention={fa!s:5}: {t:7.2f} ms", flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mx8"))
    ap.add_argument("--no-forward", action="store_true")
    a = ap.parse_args()
    os.makedirs(a.out, exist_ok=True)
    rows = site_table(a.reps)
    with open(os.path.join(a.out, "site_times.txt"), "w") as f:
        f.write(f"# tools/mx8_bench.py --reps {a.reps}: per-launch time of each transformer-block site, bf16 (default mode) vs MXFP8\n"
                "# (quantisation passes included; ff2's A operand comes from ff1's MXFP8 output)\n"
                "res level site M C bf16_us mxfp8_us speedup\n")
        for res, lv, name, M, C, t16, tmx, _ in rows:
            f.write(f"{res} {lv} {name} {M} {C} {t16 * 1e3:.1f} {tmx * 1e3:.1f} {t16 / tmx:.2f}\n")
    if not a.no_forward:
        fw = forward_table(max(3, a.reps // 5))
        with open(os.path.join(a.out, "forward_times.txt"), "w") as f:
            f.write("# tools/mx8_bench.py: one full-width 320x512 U-Net forward (bf16, 16 x 40 x 64 latent), eager\n"
                    "fp8_linear fp8_attention ms\n")
            for fl, fa, t in fw:
                f.write(f"{int(fl)} {int(fa)} {t:.2f}\n")


if __name__ == "__main__":
    main()
