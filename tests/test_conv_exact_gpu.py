"""Exact gather tests of the conv loaders on every kernel that serves them (csrc/gemm_2stage.hpp, csrc/gemm_ring.hpp: the 2-stage
kernel, the 128x128 ring, the 256x128 ring; loader modes A_CONV3X3, A_CONV3X3_FAST, A_CONVT3).

Every case of oracle/conv_exact.py CASES (the table tests/test_conv_exact_cpu.py proves against the per-op oracle) runs through
the diagnostics build with the kernel FORCED by pm_debug_gemm_ring - or left to the shipped rule - and first asserts, through
pm_debug_conv_kernel_choice (the entry point's own plan + choose_kernel), that the call runs on the kernel the case claims.
The inputs are integers whose results are exact in f32, f16 and bf16, so every comparison is torch.equal: one wrong tap on one
border pixel fails, and the message names the pixel, the tap and the channel."""
import pytest
import torch

from oracle import conv_exact as cx

pytestmark = pytest.mark.gpu

DTYPES = [torch.float16, torch.bfloat16]
GUARD = 24576.0  # what surrounds a strided operand (exact in f16 and bf16): one read of it, or one write over it, shows
GUARD_ROWS, COL0 = 3, 64


def _flags(case):
    from open_pandora_amd import capi
    stream = case.epi in ("stream", "stream_res32")
    return (capi.PM_FLAG_A_F32 if case.x32 else 0) | (capi.PM_FLAG_OUT_F32 if stream else 0)


def _choice(ops, case, ws_bytes):
    return ops.lib.pm_debug_conv_kernel_choice(0 if case.kind == "c3" else 1, case.F, case.H, case.W, case.Cin, case.Cout,
                                               case.stride, int(case.ups), case.pad_lo, _flags(case), ws_bytes)


def _slice_of_wider(t):
    """t [M, C] as a column slice of a wider GPU buffer full of GUARD, GUARD_ROWS rows before and behind it"""
    M, C = t.shape
    buf = torch.full((2 * GUARD_ROWS + M, COL0 + C + 8), GUARD, dtype=t.dtype, device="cuda")
    view = buf[GUARD_ROWS:GUARD_ROWS + M, COL0:COL0 + C]
    view.copy_(t)
    return buf, view


def _run(ops, case, d, dtype):
    """the op on the case's inputs -> (result on the CPU, guard check of a strided output or None)"""
    dev = lambda t: None if t is None else t.cuda()
    x, lo, hi = dev(d["x"]), dev(d["halo_lo"]), dev(d["halo_hi"])
    out = obuf = None
    if case.strided:
        x = _slice_of_wider(d["x"])[1]
        lo = None if lo is None else _slice_of_wider(d["halo_lo"])[1]  # (the same width: halo frames share x's row stride)
        hi = None if hi is None else _slice_of_wider(d["halo_hi"])[1]
        obuf, out = _slice_of_wider(torch.zeros(cx.rows_out(case), case.Cout, dtype=cx.out_dtype(case, dtype)))
    stream = cx.out_dtype(case, dtype) == torch.float32
    if case.kind == "c3":
        y = ops.conv3x3(x, dev(d["wp"]), dev(d["bias"]), case.F, case.H, case.W, stride=case.stride, upsample=case.ups,
                        residual=dev(d["residual"]), out=out, stream=stream, pad_lo=case.pad_lo)
    else:
        y = ops.conv_t3(x, dev(d["wp"]), dev(d["bias"]), case.F, case.H * case.W, residual=dev(d["residual"]), halo_lo=lo,
                        halo_hi=hi, out=out, stream=stream, clip_frames=case.clip)
    torch.cuda.synchronize()
    guard_ok = None
    if obuf is not None:
        mask = torch.ones_like(obuf, dtype=torch.bool)
        mask[GUARD_ROWS:GUARD_ROWS + y.shape[0], COL0:COL0 + y.shape[1]] = False
        guard_ok = bool((obuf[mask] == GUARD).all().item())
    return y.cpu(), guard_ok


def _mode_and_path(case):
    mode = "A_CONVT3" if case.kind == "t3" else ("A_CONV3X3_FAST" if case.Cin % 64 == 0 and not case.ups else "A_CONV3X3")
    if case.x32:
        return mode, "f32 A through registers"
    if mode == "A_CONV3X3":
        return mode, "per-lane select"
    return mode, "buffer descriptor" if case.halo == "none" else "select vs zero page"


@pytest.mark.parametrize("dtype", DTYPES, ids=["f16", "bf16"])
@pytest.mark.parametrize("case", cx.CASES, ids=[c.id for c in cx.CASES])
def test_conv_exact(hip_ops_factory, case, dtype):
    from open_pandora_amd.ops_hip import HipOps
    ops = hip_ops_factory(dtype, diag=True)
    lib = ops.lib
    d = cx.build(case, dtype)
    wanted = cx.want(case, d, dtype)
    presplit = ops.presplit
    try:
        lib.pm_debug_gemm_ring(*cx.FORCE[case.force])
        ops.presplit = not case.x32  # x32: the f32 operand reaches the kernel (register-staged loader), no pm_split16 pass
        choice = _choice(ops, case, ops.ws_bytes)
        assert choice == case.expect, (case.id, "runs on kernel", choice, "claimed", case.expect)
        splits = lib.pm_gemm_workspace_bytes(cx.rows_out(case), case.Cout, cx.taps_of(case) * case.Cin, 0) > 0
        assert splits or not case.split  # a `split` case: the library's own plan must split this shape
        got, guard_ok = _run(ops, case, d, dtype)
        assert got.dtype == wanted.dtype and got.shape == wanted.shape
        assert torch.equal(got, wanted), cx.describe_mismatch(case, d, got, wanted)
        assert guard_ok is not False, (case.id, "wrote outside its output slice")
        if case.split:
            nows = HipOps(dtype, "cuda:0", workspace_mb=0, diag=True)  # NULL workspace: the same call, unsplit
            assert _choice(nows, case, 0) == case.expect
            unsplit, _ = _run(nows, case, d, dtype)
            assert torch.equal(unsplit, wanted), cx.describe_mismatch(case, d, unsplit, wanted)
            assert torch.equal(unsplit, got)
    finally:
        ops.presplit = presplit
        lib.pm_debug_gemm_ring(1, 1, 0)
    if dtype == DTYPES[0]:
        mode, path = _mode_and_path(case)
        print(f"[parity] conv_exact {case.id}: {mode} on kernel {choice} ({cx.KERNEL_NAMES[choice]}), {path}"
              f"{', split-K' if splits else ''}: exact")


def test_shipped_rule_reaches_each_conv_kernel(hip_ops_factory):
    """The shipped rule itself (nothing forced), asked over a grid of model-like conv shapes: which kernels it ever picks per
    loader mode.  The "default" cases of the table sit on shapes this scan finds; a rule that reaches other kernels fails here."""
    ops = hip_ops_factory(torch.float16, diag=True)
    ops.lib.pm_debug_gemm_ring(1, 1, 0)
    seen = {0: set(), 1: set()}
    for kind in (0, 1):
        for F in (2, 3, 8, 16, 17):
            for H, W in ((5, 8), (10, 16), (20, 32), (40, 64), (48, 64), (72, 128)):
                for cin, cout in ((64, 72), (64, 128), (192, 128), (320, 320), (640, 640), (1280, 1280)):
                    seen[kind].add(ops.lib.pm_debug_conv_kernel_choice(kind, F, H, W, cin, cout, 1, 0, 1, 0, ops.ws_bytes))
    print(f"[parity] conv kernel choices of the shipped rule: 3x3 fast {sorted(seen[0])}, temporal {sorted(seen[1])}")
    # (never the 2-stage kernel with 16-bit A: see the "default" cases of oracle/conv_exact.py - if this set grows, add a case)
    assert seen[0] == {cx.K_RING, cx.K_RINGW} and seen[1] == {cx.K_RING, cx.K_RINGW}
