"""CPU: the packed fp8 attention operands (include/pandora_mi355x.h, "Packed fp8 attention operands") and the element rule of
pm_gemm_mx8_qkv_fp8 restated in numpy.  The GPU tests (tests/test_fp8_block_gpu.py) hold the kernels to this restatement bit
for bit.

Layout: q8 / k8 [B*heads][P][64] rows, v8t [B*heads][64][P] with key r of a 64-key tile at byte pos(r) of the tile's row.
Element rule: f32 value (acc * scale[n] or acc + bias[n]), q columns * qmul, clamp to +-448, e4m3 round-to-nearest-even
(subnormals included), NaN -> 0x7F."""
import os
import re

import numpy as np

from test_mx8_cpu import E4M3, e4m3_rne

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def pos(r):
    """byte of key r (0..63) inside its tile's 64-byte row of v8t"""
    r = np.asarray(r)
    return 32 * ((r >> 2) & 1) + 4 * (r >> 3) + (r & 3)


def e4m3_sat_np(y):
    """e4m3fn codes of ANY f32: clamp to +-448 (infinities included), round to nearest even; NaN -> 0x7F."""
    y = np.asarray(y, dtype=np.float32)
    nan = np.isnan(y)
    c = e4m3_rne(np.clip(np.where(nan, 0, y), -448.0, 448.0).astype(np.float32))
    return np.where(nan, 0x7F, c).astype(np.uint8)


def pack_qkv_np(y, heads, P, qmul=1.0):
    """y f32 [B*P, 3*heads*64] (the projection's f32 output) -> (q8 [B*heads, P, 64], k8 alike, v8t [B*heads, 64, P])."""
    y = np.asarray(y, dtype=np.float32)
    M, N = y.shape
    inner = heads * 64
    assert N == 3 * inner and M % P == 0 and P % 64 == 0
    B = M // P
    y = y.copy()
    y[:, :inner] = y[:, :inner] * np.float32(qmul)  # (f32 product, as the kernel forms it)
    c = e4m3_sat_np(y).reshape(B, P, 3, heads, 64)   # row m -> (m / P, m % P); column n -> (n / inner, (n % inner) / 64, n % 64)
    rows = lambda part: np.ascontiguousarray(c[:, :, part].transpose(0, 2, 1, 3)).reshape(B * heads, P, 64)
    q8, k8, v = rows(0), rows(1), rows(2)
    v8t = np.zeros((B * heads, 64, P), np.uint8)
    tok = np.arange(P)
    v8t[:, :, (tok & ~63) + pos(tok & 63)] = v.transpose(0, 2, 1)
    return q8, k8, v8t


def test_pos_is_a_permutation_and_inverts():
    p = pos(np.arange(64))
    assert sorted(p.tolist()) == list(range(64))
    inv = np.empty(64, np.int64)
    inv[p] = np.arange(64)
    # the inverse read off the layout statement: byte 32 h + 4 g + e holds key 8 g + 4 h + e
    byte = np.arange(64)
    h, g, e = byte >> 5, (byte >> 2) & 7, byte & 3
    assert np.array_equal(inv, 8 * g + 4 * h + e)
    assert np.array_equal(pos(inv), byte)
    assert [int(pos(r)) for r in (0, 1, 3, 4, 7, 8, 12, 63)] == [0, 1, 3, 32, 35, 4, 36, 63]


def test_pack_layout_against_a_plain_loop():
    rng = np.random.default_rng(0)
    heads, P, B = 2, 128, 3
    inner = heads * 64
    y = rng.integers(-8, 9, (B * P, 3 * inner)).astype(np.float32)  # exactly representable: the layout alone is under test
    q8, k8, v8t = pack_qkv_np(y, heads, P)
    for _ in range(300):
        m, n = int(rng.integers(B * P)), int(rng.integers(3 * inner))
        b, t = divmod(m, P)
        part, rest = divmod(n, inner)
        hd, d = divmod(rest, 64)
        code = e4m3_sat_np(y[m, n])
        if part < 2:
            assert (q8, k8)[part][b * heads + hd, t, d] == code
        else:
            assert v8t[b * heads + hd, d, (t // 64) * 64 + int(pos(t % 64))] == code
    assert E4M3[q8[1 * heads + 1, 5, 7]] == y[1 * P + 5, 64 + 7]


def test_element_rule_edges():
    y = np.array([449.0, -1e9, np.inf, -np.inf, np.nan, 448.0, 8.5, 9.5, 2.0 ** -10, 3 * 2.0 ** -10, -2.0 ** -11, -0.0, 0.0,
                  7.5 * 2.0 ** -9, 464.0, 1.0], np.float32)
    want = [0x7E, 0xFE, 0x7E, 0xFE, 0x7F, 0x7E, 0x50, 0x52, 0x00, 0x02, 0x80, 0x80, 0x00, 0x08, 0x7E, 0x38]
    assert e4m3_sat_np(y).tolist() == want
    # q columns carry qmul, applied in f32 before the clamp; k and v columns do not
    heads, P = 1, 64
    yy = np.full((P, 192), 3.0, np.float32)
    q8, k8, v8t = pack_qkv_np(yy, heads, P, qmul=0.5)
    assert (E4M3[q8] == 1.5).all() and (E4M3[k8] == 3.0).all() and (E4M3[v8t] == 3.0).all()


def _params(decl):
    return [a for a in re.sub(r"\s+", " ", decl).split(",") if a.strip()]


def test_header_declares_the_entry_points_and_capi_mirrors_them():
    from open_pandora_amd import capi
    text = open(os.path.join(ROOT, "include", "pandora_mi355x.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in ("pm_attention_fp8_packed", "pm_gemm_mx8_qkv_fp8"):
        m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)", code)
        assert m, f"{name} is not declared in include/pandora_mi355x.h"
        assert name in capi.SIGNATURES and len(capi.SIGNATURES[name][1]) == len(_params(m.group(1))), name
    # the layout is stated in the header, formula included
    assert "pos(r) = 32 * ((r >> 2) & 1) + 4 * (r >> 3) + (r & 3)" in text


def test_fp8_block_switch_is_validated_without_a_gpu():
    """fp8_block needs both 8-bit modes and refuses parity: checked before any device work."""
    import pytest
    import torch
    from open_pandora_amd import build
    from open_pandora_amd.ops_hip import HipOps
    build.build()
    for kw in (dict(fp8_block=True), dict(fp8_block=True, fp8_linear=True), dict(fp8_block=True, fp8_attention=True),
               dict(fp8_block=True, fp8_linear=True, fp8_attention=True, parity=True)):
        with pytest.raises(ValueError):
            HipOps(torch.float16, "cuda:0", **kw)
