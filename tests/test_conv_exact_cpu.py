"""The exact conv cases of oracle/conv_exact.py against the per-op oracle, on the CPU: for every case of the table the GPU test
runs (tests/test_conv_exact_gpu.py), builders + index-gather reference == TorchOps.conv3x3 / conv_t3 bit for bit, in both
dtypes.  This is the proof that the reference the kernels are held to is right on its own: it shares no code with the oracle
(no convolution call), so a wrong border tap in either of them fails here."""
import pytest
import torch

from oracle import conv_exact as cx
from oracle.ops_torch import TorchOps

DTYPES = [torch.float16, torch.bfloat16]


def oracle_result(case, d, dtype):
    """TorchOps on the case's inputs as the ideal 16-bit-operand machine (f32 math, 16-bit or f32-stream output)"""
    ref = TorchOps(dtype, model_16bit=True)
    stream = cx.out_dtype(case, dtype) == torch.float32
    if case.kind == "c3":
        return ref.conv3x3(d["x"], d["wp"], d["bias"], case.F, case.H, case.W, stride=case.stride, upsample=case.ups,
                           residual=d["residual"], stream=stream, pad_lo=case.pad_lo)
    P, fc = case.H * case.W, case.clip or case.F
    outs = []
    for c in range(case.F // fc):  # the oracle knows one clip: clips batched along the frames are independent calls
        rows = slice(c * fc * P, (c + 1) * fc * P)
        res = None if d["residual"] is None else d["residual"][rows]
        outs.append(ref.conv_t3(d["x"][rows], d["wp"], d["bias"], fc, P, residual=res, halo_lo=d["halo_lo"], halo_hi=d["halo_hi"],
                                stream=stream))
    return torch.cat(outs)


@pytest.mark.parametrize("dtype", DTYPES, ids=["f16", "bf16"])
@pytest.mark.parametrize("case", cx.CASES, ids=[c.id for c in cx.CASES])
def test_gather_reference_equals_oracle(case, dtype):
    d = cx.build(case, dtype)
    wanted = cx.want(case, d, dtype)
    got = oracle_result(case, d, dtype)
    assert got.dtype == wanted.dtype == cx.out_dtype(case, dtype) and got.shape == wanted.shape
    assert torch.equal(got, wanted), cx.describe_mismatch(case, d, got, wanted)


def test_case_table_covers_every_reachable_cell():
    """(loader mode x kernel x padding path): every cell the code can reach has a case"""
    cells = set()
    for c in cx.CASES:
        mode = "t3" if c.kind == "t3" else ("c3fast" if c.Cin % 64 == 0 and not c.ups else "c3gen")
        path = "regs" if c.x32 else ("select" if c.halo != "none" or mode == "c3gen" else "desc")
        cells.add((mode, c.expect, path))
    for mode in ("c3fast", "t3"):
        for k in (cx.K_TWO_STAGE, cx.K_RING, cx.K_RINGW):
            assert (mode, k, "desc") in cells
            assert mode == "c3fast" or (mode, k, "select") in cells  # (only the temporal conv takes halo frames)
        assert (mode, cx.K_TWO_STAGE, "regs") in cells
    assert ("c3gen", cx.K_TWO_STAGE, "select") in cells and ("c3gen", cx.K_TWO_STAGE, "regs") in cells

