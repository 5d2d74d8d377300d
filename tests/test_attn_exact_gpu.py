"""Exact selection and guard tests of every attention kernel (csrc/attn_cross.hpp, attn_self.hpp, attn_fp8.hpp, attn_temporal.hpp,
attn_small.hpp - one unit with the host side, csrc/attn.hip - and csrc/attn16.hip): attn_kernel (two segments, and
one segment as diagnostics variant 9), attn_self_kernel in its template forms (variants 0 / 1: QB 1, RING 2; 3: QB 2, PIPE,
RING 4; 5: QB 2, PIPE, POST, RING 4), attn_self16_kernel (by the shipped rule at >= 4096 tokens, forced as variant 16, and its
diagnostics forms 17 / 18 / 19: per-lane K/V addresses, row sums on the vector pipe, hipcc's own PV order),
attn_fp8_pack_kernel + attn_fp8_kernel (and the latter alone on the packed operands; variant 2: 64 rows per wave),
tattn_kernel and attn_small_kernel.

Every case of oracle/attn_exact.py CASES (the table tests/test_attn_exact_cpu.py proves against an f64 softmax) has a result
that is exact in f16 and bf16 - ties of 1, 2 or 4 keys placed across the first / fast / ragged tiles and ring stages, every
other key >= 192 base-2 units below - so every comparison is torch.equal: one key dropped, weighted twice or taken from
another tile, head or batch element fails, and the message names the row, the keys and what came back instead.
Strided cases pass q / k / v as column slices of (fused) buffers full of NaN - one read outside the operands turns a row NaN -
and the output as a slice of a buffer full of GUARD, which must still be there afterwards."""
import os
import re

import pytest
import torch

from oracle import attn_exact as ax

pytestmark = pytest.mark.gpu

DTYPES = [torch.float16, torch.bfloat16]
GUARD = 24576.0  # around a strided output (exact in f16 and bf16)
GUARD_ROWS, COL0, COL_TAIL = 3, 64, 8
SELF_VARIANTS = {0: "attn_self_kernel<QB 1, RING 2> (shipped library)", 1: "attn_self_kernel<QB 1, RING 2> (forced)",
                 3: "attn_self_kernel<QB 2, PIPE, RING 4>", 5: "attn_self_kernel<QB 2, PIPE, POST, RING 4>",
                 9: "attn_kernel<one segment>", 16: "attn_self16_kernel (forced)",
                 17: "attn_self16_kernel<per-lane K/V addresses>", 18: "attn_self16_kernel<row sums on the vector pipe>",
                 19: "attn_self16_kernel<hipcc's own PV order>"}
FP8_VARIANTS = {0: "", 2: " <QB 2: 64 rows per wave>"}
OTHER_KERNELS = {"cross": "attn_kernel<two segments>", "temporal": "tattn_kernel", "generic": "attn_small_kernel",
                 "fp8": "attn_fp8_pack_kernel + attn_fp8_kernel, and attn_fp8_kernel on the packed operands"}


def _params():
    out = []
    for c in ax.CASES:
        if c.kind == "fp8":
            variants = tuple(FP8_VARIANTS)
        else:
            variants = (0,) if c.kind != "self" or c.long else tuple(SELF_VARIANTS)  # (the long case: the shipped rule's own choice)
        out += [pytest.param(c, v, id=f"{c.id}-v{v}") for v in variants]
    return out


def _embed(ts, fill, per_batch):
    """same-shape [X, Y, C] CPU tensors -> views of ONE GPU buffer full of `fill` holding them side by side as column slices
    (the fused q | k | v layout), COL0 columns before and COL_TAIL behind; per_batch: GUARD_ROWS rows before and after each
    batch element's rows, else (frame-major temporal operands: frame stride = P rows) before and after all rows"""
    X, Y, C = ts[0].shape
    W = COL0 + len(ts) * C + COL_TAIL
    if per_batch:
        buf = torch.full((X, 2 * GUARD_ROWS + Y, W), fill, dtype=ts[0].dtype, device="cuda")
        body = buf[:, GUARD_ROWS:GUARD_ROWS + Y]
    else:
        buf = torch.full((2 * GUARD_ROWS + X * Y, W), fill, dtype=ts[0].dtype, device="cuda")
        body = buf[GUARD_ROWS:GUARD_ROWS + X * Y].view(X, Y, W)
    views = [body[..., COL0 + i * C:COL0 + (i + 1) * C] for i in range(len(ts))]
    for v, t in zip(views, ts):
        v.copy_(t)
    return buf, views


def _operands(case, d, dtype):
    """-> (q, k, v, k2, v2, out, obuf) on the GPU in the layout of the op that serves `case` (out / obuf None: the op allocates)"""
    turn = ax.frames_first if case.kind == "temporal" else (lambda t: t)
    q, k, v = turn(d["q"]), turn(d["k"]), turn(d["v"])
    k2, v2 = d["k2"], d["v2"]
    if not case.strided:
        dev = lambda t: None if t is None else t.cuda()
        return dev(q), dev(k), dev(v), dev(k2), dev(v2), None, None
    nan, per_batch = float("nan"), case.kind != "temporal"
    if q.shape == k.shape:
        q, k, v = _embed([q, k, v], nan, per_batch)[1]  # the model's fused [B, N, 3C] projection output
    else:
        q = _embed([q], nan, per_batch)[1][0]
        k, v = _embed([k, v], nan, per_batch)[1]
    if k2 is not None:
        k2, v2 = _embed([k2, v2], nan, per_batch)[1]
    obuf, (out,) = _embed([torch.zeros_like(turn(d["q"]))], GUARD, per_batch)
    return q, k, v, k2, v2, out, obuf


def _guard_intact(obuf, out, per_batch):
    mask = torch.ones_like(obuf, dtype=torch.bool)
    X, Y, C = out.shape
    body = mask[:, GUARD_ROWS:GUARD_ROWS + Y] if per_batch else mask[GUARD_ROWS:GUARD_ROWS + X * Y].view(X, Y, -1)
    body[..., COL0:COL0 + C] = False
    return bool((obuf[mask] == GUARD).all().item())


def _workspace_operands(ops, B, heads, Nq, Nk):
    """q8 / k8 / v8t as pm_attention_fp8's pack pass left them in its workspace (the layout of include/pandora_mi355x.h)"""
    from open_pandora_amd.ops_hip import PackedQKV
    ws = ops._workspaces[("fp8", ops._stream())]
    nq, nk = (Nq + 63) // 64 * 64, (Nk + 63) // 64 * 64
    a, b = B * heads * nq * 64, B * heads * nk * 64
    return PackedQKV(ws[:a], ws[a:a + b], ws[a + b:a + 2 * b], B, Nq, Nk)


def _run(ops, case, d, dtype):
    """-> list of (name, result [B, Nq, C] on the CPU), guard check of a strided output (None: not strided)"""
    q, k, v, k2, v2, out, obuf = _operands(case, d, dtype)
    results = []
    if case.kind in ("self", "cross"):
        y = ops.attention(q, k, v, case.heads, k2=k2, v2=v2, w2=case.w2, out=out, prescaled=case.prescaled)
    elif case.kind == "generic":
        y = ops.attention_generic(q, k, v, case.heads, out=out)
    elif case.kind == "temporal":
        y = ops.attention_temporal(q, k, v, case.heads, out=out).transpose(0, 1)
    else:
        y = ops.attention_fp8(q, k, v, case.heads, out=out, prescaled=case.prescaled)
        packed = ops.attention_fp8_packed(_workspace_operands(ops, case.B, case.heads, case.Nq, case.Nk), case.heads)
        results.append(("pm_attention_fp8_packed", packed.cpu()))
    torch.cuda.synchronize()
    results.insert(0, ("op", y.cpu()))
    return results, (None if obuf is None else _guard_intact(obuf, out, case.kind != "temporal"))


def _shipped_rule_takes_attn16(case):
    """pm_attention's rule as csrc/attn.hip states it (and test_attention_long_sequences_16x16x32_form relies on it)"""
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "open-pandora_amd", "csrc", "attn.hip")).read()
    m = re.search(r"if \(Nq >= (\d+) && Nk1 >= (\d+)\) return launch_attn_self16\(p, dtype, grid, \(hipStream_t\)stream\);", src)
    return m is not None and case.Nq >= int(m.group(1)) and case.Nk >= int(m.group(2)) and case.Nq >= 4096 and case.Nk >= 4096


@pytest.mark.parametrize("dtype", DTYPES, ids=["f16", "bf16"])
@pytest.mark.parametrize("case,variant", _params())
def test_attn_exact(hip_ops_factory, case, variant, dtype):
    ops = hip_ops_factory(dtype) if variant == 0 else hip_ops_factory(dtype, diag=True)
    d = ax.build(case, dtype)
    wanted = ax.want(case, d, dtype)
    kernel = SELF_VARIANTS[variant] if case.kind == "self" else OTHER_KERNELS[case.kind] + FP8_VARIANTS.get(variant, "")
    if case.long:
        assert _shipped_rule_takes_attn16(case), (case.id, "the shipped rule no longer sends this shape to attn_self16_kernel")
        kernel = "attn_self16_kernel (shipped library, Nq and Nk >= 4096)"
    else:
        assert case.Nq < 4096 or case.Nk < 4096  # (variant 0 of every other case: the 32x32x16 form)
    try:
        if variant:
            ops.lib.pm_debug_attn_variant(variant)
        results, guard_ok = _run(ops, case, d, dtype)
    finally:
        if variant:
            ops.lib.pm_debug_attn_variant(0)
    for name, got in results:
        assert got.dtype == wanted.dtype and got.shape == wanted.shape, name
        assert torch.equal(got, wanted), (name, kernel, ax.describe_mismatch(case, d, got, wanted))
    assert guard_ok is not False, (case.id, kernel, "wrote outside its output slice")
    if dtype == DTYPES[0]:
        print(f"[parity] attn_exact {case.id}: {kernel}{', NaN around q / k / v, guards around the output' if case.strided else ''}"
              f": exact")


@pytest.mark.parametrize("dtype", DTYPES, ids=["f16", "bf16"])
def test_memory_efficient_attention_exact(hip_ops_factory, dtype):
    """the xformers-shaped seam: (b * heads, n, 64) tensors, each (batch, head) pair one batch element of a 1-head call"""
    from open_pandora_amd.ops_hip import memory_efficient_attention
    ops = hip_ops_factory(dtype)
    (case,) = [c for c in ax.CASES if c.mea]
    d = ax.build(case, dtype)
    wanted = ax.want(case, d, dtype)
    split = lambda t: t.reshape(t.shape[0], t.shape[1], case.heads, 64).permute(0, 2, 1, 3).reshape(-1, t.shape[1], 64).cuda()
    got = memory_efficient_attention(split(d["q"]), split(d["k"]), split(d["v"]), ops=ops)
    assert got.shape == (case.B * case.heads, case.Nq, 64)
    got = got.reshape(case.B, case.heads, case.Nq, 64).permute(0, 2, 1, 3).reshape(case.B, case.Nq, -1).cpu()
    assert torch.equal(got, wanted), ax.describe_mismatch(case, d, got, wanted)
    if dtype == DTYPES[0]:
        print(f"[parity] attn_exact {case.id} through memory_efficient_attention: {SELF_VARIANTS[0]}: exact")
