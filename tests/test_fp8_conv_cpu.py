"""CPU: the MXFP8 ResBlock convolutions (pm_conv2d_3x3_mx8 / pm_conv_temporal_k3_mx8, HipOps(fp8_conv=True)) restated in numpy.

The conv on MXFP8 operands is a gather of A's BYTES AND SCALES by the index arithmetic of oracle/conv_exact.py (gather_rows: for
every output row and tap, which input row it reads, or none - then zero bytes with scale 2^0), followed by the dequantisation of
tests/test_mx8_cpu.py and an f64 product per tap against the tap's slice of the tap-major packed weight.  Here it is checked
against TorchOps.conv3x3 / conv_t3 on the dequantised tensors; tests/test_fp8_conv_gpu.py holds the kernels to it.  Also here:
the GroupNorm(+SiLU) references of pm_groupnorm_apply_mx8 (f64, and the kernel's own formula in f32), and the mode's host rules."""
import os
import re

import numpy as np
import pytest
import torch

from oracle import conv_exact as cx
from oracle.ops_torch import TorchOps
from test_mx8_cpu import mx8_dequant_np, mx8_quant_np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("pm_groupnorm_apply_mx8", "pm_conv2d_3x3_mx8", "pm_conv_temporal_k3_mx8")


def geometry(kind, F, H, W=1, clip=None):
    """the conv_exact case that carries a geometry (3x3: stride 1, pad 1; temporal: P = H * W pixels, no halo frames)"""
    return cx._case(f"mx8-{kind}-{F}x{H}x{W}-{clip}", kind=kind, F=F, H=H, W=W, clip=clip)


def gather_mx8(case, a, tap, shift=0):
    """A's bytes and scales as tap `tap` reads them: (e4m3 [M, Cin], E8M0 [M, Cin/32]); padding = zero bytes, scale 127.
    `shift` moves the tap's index (a deliberately wrong gather, for the test of the test)."""
    aq, as_ = a
    idx = cx.gather_rows(case, tap).numpy()
    if shift:
        idx = np.where(idx >= 0, np.clip(idx + shift, 0, aq.shape[0] - 1), idx)
    pad = idx < 0
    q, s = aq[np.where(pad, 0, idx)].copy(), as_[np.where(pad, 0, idx)].copy()
    q[pad], s[pad] = 0, 127
    return q, s


def im2col_mx8(case, a):
    """the im2col MXFP8 operand [M, taps * Cin] (tap-major K) and its scales: pm_gemm_mx8's A for the same product"""
    parts = [gather_mx8(case, a, t) for t in range(cx.taps_of(case))]
    return np.concatenate([p[0] for p in parts], 1), np.concatenate([p[1] for p in parts], 1)


def conv_mx8_np(case, a, w, bias=None, residual=None, shift_tap=None):
    """f64 [M, Cout]: sum over taps of deq(gathered A) @ deq(W)[:, tap]^T + bias + residual"""
    wq, ws = w
    taps, cin, cout = cx.taps_of(case), a[0].shape[1], wq.shape[0]
    wd = mx8_dequant_np(wq, ws).reshape(cout, taps, cin)
    y = np.zeros((cx.rows_out(case), cout))
    for t in range(taps):
        q, s = gather_mx8(case, a, t, shift=1 if t == shift_tap else 0)
        y += mx8_dequant_np(q, s) @ wd[:, t].T
    if bias is not None:
        y += np.asarray(bias, np.float64)
    if residual is not None:
        y += np.asarray(residual, np.float64)
    return y


def groupnorm_f64(x, gamma, beta, eps, NI, silu, groups=32):
    """f32 [M, C]: GroupNorm (biased variance over the P x C/groups values of an instance's group) + SiLU, evaluated in f64"""
    M, C = x.shape
    xd = np.asarray(x, np.float64).reshape(NI, M // NI, groups, C // groups)
    mu = xd.mean((1, 3), keepdims=True)
    var = ((xd - mu) ** 2).mean((1, 3), keepdims=True)
    y = ((xd - mu) / np.sqrt(var + eps)).reshape(M, C) * np.asarray(gamma, np.float64) + np.asarray(beta, np.float64)
    if silu:
        y = y / (1 + np.exp(-y))
    return y.astype(np.float32)


def groupnorm_kernel_f32(x, gamma, beta, eps, NI, silu, groups=32):
    """the same GroupNorm by the kernel's formula in f32: totals {sum, sumsq} -> mean, var = E[x^2] - mean^2, rstd; per channel
    sc = rstd * gamma, sh = beta - mean * sc; v = x * sc + sh; SiLU"""
    M, C = x.shape
    f = np.float32
    xg = np.asarray(x, f).reshape(NI, M // NI, groups, C // groups)
    inv = f(1.0 / ((M // NI) * (C // groups)))
    mean = xg.sum((1, 3), dtype=f) * inv
    var = np.maximum((xg * xg).sum((1, 3), dtype=f) * inv - mean * mean, f(0))
    rstd = (f(1) / np.sqrt(var + f(eps))).astype(f)
    sc = np.repeat(rstd, C // groups, 1) * np.asarray(gamma, f)  # [NI, C]
    sh = np.asarray(beta, f) - np.repeat(mean, C // groups, 1) * sc
    v = (np.asarray(x, f).reshape(NI, M // NI, C) * sc[:, None] + sh[:, None]).astype(f).reshape(M, C)
    if silu:
        v = (v / (f(1) + np.exp(-v))).astype(f)
    return v


def quant_caps(gq, gs, wq, ws):
    """The caps of test_quant_layernorm_fused for two MXFP8 pairs from two evaluations of the same f32 value: share of equal scale
    codes, share of differing element codes, and whether every differing code is within one e4m3 step where the scales agree."""
    same = gs == ws
    dq, dw = mx8_dequant_np(gq, gs), mx8_dequant_np(wq, ws)
    agree = np.repeat(same, 32, axis=1)
    step = np.maximum(np.abs(dw) * 2 ** -3, np.repeat(np.ldexp(1.0, gs.astype(np.int64) - 127 - 9), 32, axis=1))
    return same.mean(), (gq != wq).mean(), bool((np.abs(dq - dw)[agree] <= 1.01 * step[agree]).all())


def gn_inputs(C, M, seed, dtype=np.float32):
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal((M, C)) * 2 + rng.standard_normal((1, C))).astype(np.float32)
    g = (1 + 0.1 * rng.standard_normal(C)).astype(np.float32)
    b = (0.1 * rng.standard_normal(C)).astype(np.float32)
    return x, g, b


def _random_pairs(rng, rows, cin, cout, taps):
    a = mx8_quant_np(rng.standard_normal((rows, cin)).astype(np.float32))
    w = mx8_quant_np((0.02 * rng.standard_normal((cout, taps * cin))).astype(np.float32))
    return a, w


def _t(v):
    return torch.from_numpy(np.ascontiguousarray(v, dtype=np.float32))


@pytest.mark.parametrize("F,H,W,cin,cout", [(3, 9, 7, 64, 96), (2, 5, 6, 32, 32)])
def test_conv3x3_restatement_against_torch(F, H, W, cin, cout):
    rng = np.random.default_rng(F * H)
    case = geometry("c3", F, H, W)
    a, w = _random_pairs(rng, F * H * W, cin, cout, 9)
    bias = rng.standard_normal(cout).astype(np.float32)
    res = rng.standard_normal((F * H * W, cout)).astype(np.float32)
    got = conv_mx8_np(case, a, w, bias, res)
    want = TorchOps().conv3x3(_t(mx8_dequant_np(*a)), _t(mx8_dequant_np(*w)), _t(bias), F, H, W, residual=_t(res),
                              stream=True).double().numpy()
    assert np.abs(got - want).max() <= 1e-5 * np.abs(want).max()
    # the im2col operand is the same statement
    iq, is_ = im2col_mx8(case, a)
    assert np.allclose(mx8_dequant_np(iq, is_) @ mx8_dequant_np(*w).T + bias + res, got, rtol=0, atol=1e-12)
    # a border tap gathered one row further: no longer the conv
    for tap in (0, 5):
        bad = conv_mx8_np(case, a, w, bias, res, shift_tap=tap)
        assert np.abs(bad - want).max() > 1e-2 * np.abs(want).max()


@pytest.mark.parametrize("clip", [None, 4, 1])
def test_conv_t3_restatement_against_torch(clip):
    rng = np.random.default_rng(11)
    F, P, cin, cout = 8, 37, 64, 96
    case = geometry("t3", F, P, clip=clip)
    a, w = _random_pairs(rng, F * P, cin, cout, 3)
    bias = rng.standard_normal(cout).astype(np.float32)
    got = conv_mx8_np(case, a, w, bias)
    ad, wd = _t(mx8_dequant_np(*a)), _t(mx8_dequant_np(*w))
    fc = clip or F
    want = torch.cat([TorchOps().conv_t3(ad[j * fc * P:(j + 1) * fc * P], wd, _t(bias), fc, P, stream=True)
                      for j in range(F // fc)]).double().numpy()
    assert np.abs(got - want).max() <= 1e-5 * np.abs(want).max()
    if fc > 1:
        bad = conv_mx8_np(case, a, w, bias, shift_tap=2)
        assert np.abs(bad - want).max() > 1e-2 * np.abs(want).max()


@pytest.mark.parametrize("silu", [False, True])
@pytest.mark.parametrize("C", [320, 1280])
def test_groupnorm_restatement_holds_the_caps_against_an_f32_evaluation(C, silu):
    """The caps the GPU test puts on pm_groupnorm_apply_mx8 against quantise(f64 GroupNorm) must already hold for the kernel's own
    formula evaluated in f32 on the CPU: two f32-level evaluations differ by a few ulp against an e4m3 step of 2^-3 relative."""
    x, g, b = gn_inputs(C, 2 * 150, C + silu)
    ref = mx8_quant_np(groupnorm_f64(x, g, b, 1e-5, 2, silu))
    f32 = mx8_quant_np(groupnorm_kernel_f32(x, g, b, 1e-5, 2, silu))
    scales_equal, codes_differ, one_step = quant_caps(*f32, *ref)
    assert scales_equal > 0.999 and codes_differ < 2e-3 and one_step, (scales_equal, codes_differ, one_step)


def test_fp8_conv_refuses_parity():
    from open_pandora_amd.ops_hip import HipOps
    for parity in (True, "selective", [("gn3", 0)]):
        with pytest.raises(ValueError):
            HipOps(torch.float16, "cuda:0", fp8_conv=True, parity=parity)


def test_symbols_declared():
    from open_pandora_amd import capi
    text = open(os.path.join(ROOT, "include", "pandora_mi355x.h")).read()
    for name in NEW_SYMBOLS:
        assert name in capi.SIGNATURES, name
        m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*)\)\s*;", text)
        assert m, f"{name} is not declared in include/pandora_mi355x.h"
        assert len(m.group(1).split(",")) == len(capi.SIGNATURES[name][1]), name
