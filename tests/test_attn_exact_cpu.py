"""The exact attention cases of oracle/attn_exact.py proved on the CPU: for every case of the table the GPU test runs
(tests/test_attn_exact_gpu.py) and both dtypes, the closed form (`want`: group means by index arithmetic) equals a plain f64
softmax attention with the real scale on the same tensors, rounded once - bit for bit; every operand round-trips through f16,
bf16 (and e4m3 for the fp8 cases); after the kernels' own treatment of q the winning score lies >= 64 base-2 units (in fact
>= MIN_GAP = 192) above every other score and all winners of a row tie exactly; groups have 1, 2 or 4 keys; and every tie
placement the GPU test is meant to reach occurs in the table."""
import pytest
import torch

from oracle import attn_exact as ax

DTYPES = [torch.float16, torch.bfloat16]
IDS = [c.id for c in ax.CASES]


def _heads(t, case):
    return t.double().reshape(t.shape[0], t.shape[1], case.heads, case.D).permute(0, 2, 1, 3)


def softmax_reference(case, d):
    """f64 [B, Nq, C]: sum over the segments of w * softmax(scale * q k^T) v, per head (prescaled: scale = ln 2, i.e. base 2)"""
    q = _heads(d["q"], case)
    y = 0.0
    for k, v, w in ((d["k"], d["v"], 1.0), (d["k2"], d["v2"], case.w2)):
        if k is None:
            continue
        s = torch.einsum("bhid,bhjd->bhij", q, _heads(k, case).expand(case.B, -1, -1, -1)) * ax.scale_of(case)
        y = y + w * torch.einsum("bhij,bhjd->bhid", torch.softmax(s, -1), _heads(v, case).expand(case.B, -1, -1, -1))
    return y.permute(0, 2, 1, 3).reshape(case.B, case.Nq, case.heads * case.D)


@pytest.mark.parametrize("dtype", DTYPES, ids=["f16", "bf16"])
@pytest.mark.parametrize("case", ax.CASES, ids=IDS)
def test_closed_form_equals_f64_softmax(case, dtype):
    d = ax.build(case, dtype)
    wanted = ax.want(case, d, dtype)
    ref = softmax_reference(case, d).to(dtype)
    assert wanted.dtype == dtype and wanted.shape == (case.B, case.Nq, case.heads * case.D)
    assert torch.equal(ref, wanted), ax.describe_mismatch(case, d, ref, wanted)


@pytest.mark.parametrize("dtype", DTYPES, ids=["f16", "bf16"])
@pytest.mark.parametrize("case", ax.CASES, ids=IDS)
def test_operands_round_trip_and_scores_are_separated(case, dtype):
    d = ax.build(case, dtype)
    st = d["st"]
    for name in ("q", "k", "v", "k2", "v2"):
        t = d[name]
        if t is None:
            continue
        f = t.float()
        assert torch.equal(f.half().float(), f) and torch.equal(f.bfloat16().float(), f), (case.id, name)
        if case.kind == "fp8":
            assert torch.equal(f.to(torch.float8_e4m3fn).float(), f), (case.id, name, "not on the e4m3 grid")
    for s, k in enumerate((d["k"], d["k2"])):
        if k is None:
            continue
        gid = st["key_gid"][s].expand(case.B, -1, -1)  # [B, H, Nk]
        win = gid[:, :, None, :] == st["sel"][s][..., None]  # [B, H, Nq, Nk]: the keys each query averages
        mult = win.sum(-1)
        assert set(mult.unique().tolist()) <= {1, 2, 4}, (case.id, s)
        for rounded in (False, True):
            qe = ax.q_effective(case, d["q"], dtype, rounded)
            sc = torch.einsum("bhid,bhjd->bhij", _heads(qe, case), _heads(k, case).expand(case.B, -1, -1, -1))  # base-2 units
            top = sc.max(-1).values
            assert bool((sc[win] == top[..., None].expand_as(sc)[win]).all()), (case.id, s, "winners do not tie exactly")
            gap = (top - sc.masked_fill(win, float("-inf")).max(-1).values).min().item()
            assert gap >= 64.0 and gap >= ax.MIN_GAP, (case.id, s, rounded, gap)


def test_every_tie_placement_occurs():
    """each placement of the issue's list is reached on the one-segment MFMA kernels (both scaling modes where the kernel
    treats q differently), on the long form, on each segment of the two-segment kernel where its tiles allow it, and on fp8"""
    seen = {}
    for c in ax.CASES:
        if c.kind in ("self", "fp8"):
            key = "long" if c.long else (c.kind, c.prescaled)
            seen.setdefault(key, set()).update(ax.placements(c, ax._structure(c)))
        elif c.kind == "cross":
            for s in (0, 1):
                seen.setdefault(("cross", s), set()).update(ax.placements(c, ax._structure(c), s))
        else:
            seen.setdefault(c.kind, set()).update(ax.placements(c, ax._structure(c)))
    everything = set(ax.PLACEMENTS)
    for key in (("self", False), ("self", True), "long"):
        assert seen[key] == everything, (key, everything - seen[key])
    one_tile = {"last key + a key of tile 0", "last key alone", "row 0", "row Nq-1"}
    assert seen[("fp8", False)] >= everything - {"fast+fast in two ring stages"} | one_tile, seen[("fp8", False)]
    assert seen[("cross", 0)] >= one_tile | {"tile 0 alone, later tiles far below"} and seen[("cross", 1)] >= one_tile
    assert seen["temporal"] >= one_tile and seen["generic"] >= one_tile


def test_table_holds_the_shapes_the_kernels_branch_on():
    by = {c.id: c for c in ax.CASES}
    assert {c.Nk for c in ax.CASES if c.kind == "self" and c.Nq == c.Nk} >= {40, 64, 65, 448, 488, 4136}
    long = [c for c in ax.CASES if c.long]
    assert len(long) == 1 and long[0].Nq >= 4096 and long[0].Nk >= 4096 and not any(
        c.Nq >= 4096 and c.Nk >= 4096 for c in ax.CASES if not c.long)
    assert any(c.kind == "temporal" and c.B * c.heads > 8192 for c in ax.CASES)  # the capped grid's second trip
    assert by["temporal-F5-P37"].Nk % 4 != 0
    assert {(c.Nq, c.w2) for c in ax.CASES if c.kind == "cross"} >= {(160, 1.0), (160, 0.5), (40, 1.0), (40, 0.5)}
    assert any(c.kind == "self" and c.strided for c in ax.CASES) and any(c.kind == "cross" and c.strided for c in ax.CASES)
    for c in ax.CASES:  # selections differ between instances: the query -> label maps of two heads / batch elements are not equal
        ql = ax._structure(c)["q_label"].reshape(c.B * c.heads, c.Nq)
        assert c.B * c.heads == 1 or not torch.equal(ql[0], ql[1]), c.id
    t = ax._structure(by["temporal-F16-P1100-h8"])["q_label"].reshape(-1, 16)
    assert t.shape[0] == 8800 and not torch.equal(t[:608], t[8192:])  # problems 8192.. are not a replay of 0..607
