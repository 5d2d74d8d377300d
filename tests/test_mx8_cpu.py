"""CPU: the MXFP8 quantisation rule of pm_quant_mx8 / pm_gemm_mx8 (include/pandora_mi355x.h, "MXFP8") restated in numpy, checked
against hand-worked values.  The GPU tests (tests/test_mx8_gpu.py) hold the kernels to this restatement bit for bit.

Rule, per block of 32 values along K with amax a: X = clamp(ceil(log2(a / 448)), -127, 127), E8M0 code X + 127 (0 for an
all-zero block); elements = v / 2^X rounded to nearest-even in e4m3fn, subnormals included; a block with a NaN / Inf: code 0xFF
and NaN (0x7F) elements."""
import numpy as np
import pytest

E4M3_MAX = 448.0


def e4m3_values():
    """float64 value of each of the 256 e4m3fn codes (NaN for 0x7F / 0xFF)."""
    v = np.empty(256)
    for c in range(256):
        s = -1.0 if c & 0x80 else 1.0
        e, m = (c >> 3) & 15, c & 7
        v[c] = s * (m * 2.0 ** -9 if e == 0 else (1 + m / 8) * 2.0 ** (e - 7))
    v[0x7F] = v[0xFF] = np.nan
    return v


E4M3 = e4m3_values()


def e4m3_rne(y):
    """e4m3fn codes of float32 values |y| <= 448 (finite), round to nearest even, subnormals included, sign kept."""
    y = np.asarray(y, dtype=np.float32)
    shape, y = y.shape, y.reshape(-1)
    a = np.abs(y).astype(np.float64)
    sign = np.where(np.signbit(y), 0x80, 0).astype(np.uint32)
    code = np.rint(a * 512.0).astype(np.uint32)  # subnormal range: steps of 2^-9 (8 -> 0x08 = 2^-6)
    normal = a >= 2.0 ** -6
    if normal.any():
        f, e = np.frexp(a[normal])                # a = f 2^e, f in [0.5, 1)
        E = e - 1
        r = np.rint(a[normal] * np.ldexp(1.0, 3 - E))  # mantissa with 3 bits, in [8, 16]
        up = r == 16
        E, r = np.where(up, E + 1, E), np.where(up, 8, r)
        assert (E <= 8).all(), "a value above 448"
        code[normal] = (((E + 7) << 3) | (r.astype(np.int64) - 8)).astype(np.uint32)
    return (code | sign).astype(np.uint8).reshape(shape)


def mx8_quant_np(x):
    """x [M, K] (any float dtype, converted to f32) -> (e4m3 codes uint8 [M, K], E8M0 codes uint8 [M, K/32])."""
    x = np.asarray(x, dtype=np.float32)
    M, K = x.shape
    assert K % 32 == 0
    b = x.reshape(M, K // 32, 32)
    bad = ~np.isfinite(b).all(-1)
    with np.errstate(invalid="ignore"):
        a = np.where(bad, 0, np.abs(b).max(-1)).astype(np.float32)
    f, e = np.frexp(a)                            # a = f 2^e, f in [0.5, 1): X = (e - 1) - 8 + (2f > 1.75)
    X = np.clip(e.astype(np.int64) - 9 + (f > 0.875), -127, 127)
    X = np.where(a == 0, -127, X)
    scale = (X + 127).astype(np.uint8)
    inv = np.ldexp(np.float32(1.0), -X).astype(np.float32)
    y = np.where(bad[..., None], 0, b) * inv[..., None]  # exact: a power of two
    q = e4m3_rne(y.astype(np.float32))
    q[bad] = 0x7F
    scale[bad] = 0xFF
    return q.reshape(M, K), scale


def mx8_dequant_np(q, s):
    """float64 values of an MXFP8 pair."""
    M, K = q.shape
    sc = np.where(s == 0xFF, np.nan, np.ldexp(1.0, s.astype(np.int64) - 127))
    return (E4M3[q].reshape(M, K // 32, 32) * sc[..., None]).reshape(M, K)


def block(*vals, fill=0.0):
    v = np.full(32, fill, dtype=np.float32)
    v[:len(vals)] = vals
    return v[None]


def test_e4m3_table_edges():
    assert E4M3[0x7E] == 448.0 and E4M3[0x01] == 2.0 ** -9 and E4M3[0x08] == 2.0 ** -6 and E4M3[0x38] == 1.0
    assert np.isnan(E4M3[0x7F]) and E4M3[0xFE] == -448.0


def test_block_max_448_is_unscaled():
    q, s = mx8_quant_np(block(448.0, -448.0, 1.0, 0.5))
    assert s[0, 0] == 127 and list(q[0, :4]) == [0x7E, 0xFE, 0x38, 0x30]


def test_scale_rounds_up_not_floor():
    # amax 449: X = 1 (the OCP floor rule would take X = 0 and clip 449 to 448)
    q, s = mx8_quant_np(block(449.0, 3.0))
    assert s[0, 0] == 128 and E4M3[q[0, 0]] * 2 == 448.0 and E4M3[q[0, 1]] * 2 == 3.0
    # amax exactly 448 * 2^k keeps the scale 2^k; amax 1 gets 2^-8 (1 -> 256)
    for k in (-20, -3, 0, 5, 20):
        q, s = mx8_quant_np(block(448.0 * 2.0 ** k))
        assert s[0, 0] == 127 + k and q[0, 0] == 0x7E
    q, s = mx8_quant_np(block(1.0))
    assert s[0, 0] == 119 and E4M3[q[0, 0]] == 256.0


def test_ties_round_to_even():
    # scale 2^0 (amax 448): in [8, 16) e4m3 steps by 1; 8.5 -> 8, 9.5 -> 10; 17 (step 2) -> 16, 19 -> 20
    q, s = mx8_quant_np(block(448.0, 8.5, 9.5, 17.0, 19.0, -8.5, 8.5000005))
    assert s[0, 0] == 127
    assert list(E4M3[q[0, 1:7]]) == [8.0, 10.0, 16.0, 20.0, -8.0, 9.0]


def test_subnormals():
    # scale 2^0: subnormal steps of 2^-9; 2^-10 is a tie -> 0 (even), 3 * 2^-10 -> 2 * 2^-9, 2^-9 * 7.5 -> 8 * 2^-9 = 2^-6
    q, s = mx8_quant_np(block(448.0, 2.0 ** -10, 3 * 2.0 ** -10, 7.5 * 2.0 ** -9, 2.0 ** -9, -2.0 ** -11))
    assert s[0, 0] == 127
    assert list(q[0, 1:6]) == [0x00, 0x02, 0x08, 0x01, 0x80]


def test_zero_and_nan_blocks():
    q, s = mx8_quant_np(np.concatenate([block(), block(1.0, np.nan), block(np.inf), block(-0.0, 2.0)], 1))
    assert list(s[0]) == [0, 0xFF, 0xFF, 120]  # amax 2: X = 1 - 8
    assert (q[0, :32] == 0).all() and (q[0, 32:96] == 0x7F).all() and q[0, 96] == 0x80
    d = mx8_dequant_np(q, s)
    assert np.isnan(d[0, 32:96]).all() and not np.isnan(d[0, :32]).any()


def test_wide_dynamic_range_round_trip():
    """Blocks spanning 2^-20 ... 2^20: relative error of every element within half an e4m3 step of its block's grid."""
    rng = np.random.default_rng(3)
    rows = []
    for k in range(-20, 21, 4):
        rows.append(rng.standard_normal(128).astype(np.float32) * np.float32(2.0 ** k))
    x = np.stack(rows)
    q, s = mx8_quant_np(x)
    d = mx8_dequant_np(q, s)
    xb, db = x.reshape(-1, 32).astype(np.float64), d.reshape(-1, 32)
    amax = np.abs(xb).max(-1, keepdims=True)
    assert (amax <= 448.0 * np.ldexp(1.0, s.reshape(-1, 1).astype(np.int64) - 127)).all()  # the scale rounds up: no clipping
    step = np.maximum(2.0 ** (np.floor(np.log2(np.maximum(np.abs(xb), 1e-300))) - 3),
                      np.ldexp(1.0, s.reshape(-1, 1).astype(np.int64) - 127 - 9))
    assert (np.abs(db - xb) <= 0.5 * step * (1 + 1e-12)).all()
    assert int(s.max()) - int(s.min()) >= 38  # (both ends of the range present)


def test_block_of_tiny_values_hits_the_scale_floor():
    # amax an f32 subnormal: the scale clamps at 2^-127 (code 0) and the elements are v * 2^127, exact in f32
    q, s = mx8_quant_np(block(np.float32(1e-40), np.float32(2.0 ** -130), np.float32(2.0 ** -140)))
    assert s[0, 0] == 0 and list(q[0, :3]) == [e4m3_rne(np.float32(1e-40) * np.float32(2.0 ** 127)), 0x20, 0x00]


@pytest.mark.parametrize("K", [64, 320])
def test_restatement_matches_exhaustive_scalar_rule(K):
    """The vectorised restatement against a plain per-element loop over the same rule."""
    rng = np.random.default_rng(K)
    x = (rng.standard_normal((3, K)) * np.exp2(rng.integers(-12, 12, (3, 1)))).astype(np.float32)
    q, s = mx8_quant_np(x)
    for m in range(3):
        for b in range(K // 32):
            v = x[m, 32 * b:32 * b + 32].astype(np.float64)
            a = np.abs(v).max()
            X = max(-127, min(127, int(np.ceil(np.log2(a / 448.0)))))
            assert s[m, b] == X + 127
            grid = E4M3[:0x7F]
            for i in range(32):
                y = v[i] / 2.0 ** X
                d = np.abs(grid - abs(y))
                best = np.flatnonzero(d == d.min())
                pick = best[0] if len(best) == 1 else [c for c in best if c % 2 == 0][0]
                assert E4M3[q[m, 32 * b + i]] == np.copysign(grid[pick], y)
