"""The fused 8-bit self-attention chain (HipOps(fp8_block=True)) against the unfused one, per site and per forward.

Per site (levels 0 and 1 of 320x512 and 576x1024, 16 frames): `gemm_mx8 (16-bit q|k|v) -> attention_fp8 (pack pass + kernel) ->
quant_mx8` against `gemm_mx8_qkv_fp8 -> attention_fp8_packed(mx_out)`; both start from the same MXFP8 LayerNorm output and end
with to_out's MXFP8 A operand.  Same process, interleaved, median of `rounds` rounds of `reps` back-to-back launches (HIP events).
Per forward: the full-width 320x512 U-Net with fp8_linear + fp8_attention, fp8_block off / on, interleaved alike.

    python tools/fp8_block_bench.py [--reps 10] [--rounds 5] [--out profiles/fp8_block] [--no-forward]
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

# (resolution, level, frames, tokens per frame, channels)
SITES = [("320x512", 0, 16, 40 * 64, 320), ("320x512", 1, 16, 20 * 32, 640),
         ("576x1024", 0, 16, 72 * 128, 320), ("576x1024", 1, 16, 36 * 64, 640)]


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
    ops = HipOps(torch.bfloat16, "cuda:0", fp8_linear=True, fp8_attention=True, fp8_block=True)
    dev, rows = "cuda:0", []
    for res, lv, F, P, C in SITES:
        torch.manual_seed(lv)
        heads, M = C // 64, F * P
        h = torch.randn(M, C, device=dev)
        g, b = torch.ones(C, device=dev), torch.zeros(C, device=dev)
        wq = ops.quant_mx8((0.05 * torch.randn(3 * C, C, device=dev)).to(torch.bfloat16))
        qs = torch.cat([torch.full((C,), float(ops.q_prescale)), torch.ones(2 * C)]).to(dev)
        a = ops.ln_quant_mx8(h, g, b)

        def unfused():
            qkv = ops.gemm_mx8(a, wq, col_scale=qs).view(F, P, 3 * C)
            o = ops.attention_fp8(qkv[..., :C], qkv[..., C:2 * C], qkv[..., 2 * C:], heads, prescaled=True)
            return ops.quant_mx8(o.view(M, C))

        def fused():
            return ops.attention_fp8_packed(ops.gemm_mx8_qkv_fp8(a, wq, qs, heads, P), heads, mx_out=True)

        parts = {"gemm16": lambda: ops.gemm_mx8(a, wq, col_scale=qs), "gemm_qkv8": lambda: ops.gemm_mx8_qkv_fp8(a, wq, qs, heads, P)}
        tu, tf, tg16, tg8 = interleaved([unfused, fused, parts["gemm16"], parts["gemm_qkv8"]], reps, rounds)
        rows.append((res, lv, M, P, C, tu, tf, tg16, tg8))
        print(f"{res:>8} L{lv} M={M:>6} P={P:>5} C={C:>4}: unfused {tu * 1e3:9.1f} us  fused {tf * 1e3:9.1f} us  x{tu / tf:5.3f}   "
              f"(q|k|v GEMM alone: 16-bit out {tg16 * 1e3:8.1f} us, packed e4m3 out {tg8 * 1e3:8.1f} us)", flush=True)
        del h, a, wq
        torch.cuda.empty_cache()
    return rows


def forward_table(reps, rounds):
    from oracle import golden_recipe as gr
    from open_pandora_amd import factory
    table = [HipOps(torch.bfloat16, "cuda:0", fp8_linear=True, fp8_attention=True, fp8_block=fb) for fb in (False, True)]
    pm = factory.build_diffusion("320x512", table[0], seed=gr.WEIGHT_SEED)
    ins, cond, _ = gr.sampler_inputs(40, 64)
    c = {k: [t.cuda() for t in v] for k, v in cond.items()}
    args = (ins["x_T"].cuda(), torch.tensor([500]).cuda(), c)
    fs = torch.tensor([15]).cuda()
    unet = pm.model.diffusion_model

    def run(ops):
        def f():
            unet.ops = ops  # (not bind(): the packed weight set is the same in both modes and must not be rebuilt per turn)
            return pm.apply_model(*args, fs=fs)
        return f
    t = interleaved([run(o) for o in table], reps, rounds)
    for fb, ms in zip((False, True), t):
        print(f"320x512 forward bf16 fp8_linear + fp8_attention, fp8_block={fb!s:5}: {ms:7.2f} ms", flush=True)
    return t


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fp8_block"))
    ap.add_argument("--no-forward", action="store_true")
    a = ap.parse_args()
    os.makedirs(a.out, exist_ok=True)
    head = f"# tools/fp8_block_bench.py --reps {a.reps} --rounds {a.rounds}; library sources digest {_b.sources_digest()[:16]}\n"
    rows = site_table(a.reps, a.rounds)
    with open(os.path.join(a.out, "site_times.txt"), "w") as f:
        f.write(head + "# per spatial self-attention site, from the MXFP8 LayerNorm output to to_out's MXFP8 operand: unfused = gemm_mx8 +\n"
                "# attention_fp8 (pack + kernel) + quant_mx8, fused = gemm_mx8_qkv_fp8 + attention_fp8_packed(mx_out); median burst times\n"
                "res level M P C unfused_us fused_us speedup gemm_16bit_out_us gemm_packed_out_us\n")
        for res, lv, M, P, C, tu, tf, tg16, tg8 in rows:
            f.write(f"{res} {lv} {M} {P} {C} {tu * 1e3:.1f} {tf * 1e3:.1f} {tu / tf:.3f} {tg16 * 1e3:.1f} {tg8 * 1e3:.1f}\n")
    if not a.no_forward:
        t = forward_table(max(2, a.reps // 3), a.rounds)
        with open(os.path.join(a.out, "forward_times.txt"), "w") as f:
            f.write(head + "# one full-width 320x512 U-Net forward (bf16, 16 x 40 x 64 latent), eager, fp8_linear + fp8_attention on\n"
                    "fp8_block ms\n")
            for fb, ms in zip((0, 1), t):
                f.write(f"{fb} {ms:.2f}\n")


if __name__ == "__main__":
    main()
