"""ORACLE (test infrastructure): exact-integer inputs, an index-gather reference and the ONE case table of the conv loader tests
(tests/test_conv_exact_cpu.py: the reference equals oracle/ops_torch.py bit for bit; tests/test_conv_exact_gpu.py: every kernel
that serves a conv loader equals the reference bit for bit).

Two kinds of inputs, both with integer values small enough that every f32 partial sum, and the final value in f16 and bf16
where it is stored as 16 bit, is exact - so the comparisons are torch.equal, never a tolerance:

  "probe"  Wp[co, tap, c] is 1.0 at exactly one (tap(co), c(co)) per output channel (tap(co) = co % taps, c(co) seeded at random)
           and 0 elsewhere; x, halo frames and the residual are integers in [-100, 100], the bias integers in [-20, 20].  An output
           element is x[neighbour(pixel, tap(co)), c(co)] + bias + residual, or bias + residual where the tap is padding:
           |value| <= 220 < 256.  A wrong element names the pixel, the tap and the channel that was gathered wrongly.
  "int"    x in [-3, 3], w in [-2, 2] with every third K column zeroed, full K: integer sums far below 2^24 (the K walk,
           split-K slices and their reduce); f32 output equals the reference, 16-bit output equals reference.to(dtype).

The reference is a gather by index arithmetic (gather_rows: for every output row and tap, WHICH input row it reads, or none)
followed by an f64 product per tap (integers far below 2^53: exact).  It calls no convolution, so it shares nothing with TorchOps.conv3x3 / conv_t3.
"""
import collections

import torch

# kernel ids: what pm_gemm_kernel_choice / pm_debug_conv_kernel_choice return for the three kernels that carry conv loaders
K_TWO_STAGE, K_RING, K_RINGW = 0, 1, 3
KERNEL_NAMES = {K_TWO_STAGE: "2-stage", K_RING: "ring", K_RINGW: "ringw"}
# `force` -> (ring, ringw, split_force) of pm_debug_gemm_ring; "default" is the shipped rule.  The 256x128 ring kernel has no
# split-K form (a call whose plan splits goes to the 128x128 ring): its cases run with split_force = 1 = never split, so that
# the long-K shapes reach it; on the other two kernels the library's own plan decides (the Cin = 320 3x3 cases split).
FORCE = {"2stage": (0, 1, 0), "ring": (2, 0, 0), "ringw": (2, 2, 1), "default": (1, 1, 0)}
FORCED_KERNEL = {"2stage": K_TWO_STAGE, "ring": K_RING, "ringw": K_RINGW}

_FIELDS = dict(
    id=None, kind="c3",      # "c3": conv3x3 (F frames of H x W), "t3": temporal conv (F frames of P = H pixels, W = 1)
    inputs="probe",          # "probe" / "int" (module docstring)
    F=3, H=9, W=7, Cin=64, Cout=72, stride=1, pad_lo=1, ups=False,
    halo="none",             # t3: "none" (buffer-descriptor padding) / "both" / "lo" / "hi" (select-against-zero-page padding)
    clip=None,               # t3: clip_frames (None = F)
    force="2stage",          # key of FORCE
    expect=None,             # kernel id the case must run on (None: FORCED_KERNEL[force])
    epi="bias",              # "none" / "bias" / "bias_res16" (16-bit out + 16-bit residual) / "stream" (f32 out) / "stream_res32"
    x32=False,               # x is f32 and staged through registers (HipOps.presplit = False): 2-stage kernel only
    strided=False,           # x (and halos) / the output are column slices of wider buffers with guard values around them
    split=False,             # the library's own plan splits K (deep-level shape); run with and without a workspace
)
Case = collections.namedtuple("Case", list(_FIELDS))


def _case(id, **kw):
    f = dict(_FIELDS, id=id, **kw)
    assert set(f) == set(_FIELDS), set(f) - set(_FIELDS)
    if f["expect"] is None:
        f["expect"] = K_TWO_STAGE if f["x32"] else FORCED_KERNEL[f["force"]]
    return Case(**f)


def _cases():
    out = []
    kernels = ("2stage", "ring", "ringw")
    # ---- 3x3 fast mode (Cin % 64 == 0, no upsample) on all three kernels: stride x pad_lo, frames of 9 x 7 and 10 x 16 pixels
    # (M = 189 / 480 at stride 1: 128- and 256-row tiles straddle frame borders, ragged last tile), ragged / tiny column tiles,
    # one and five channel chunks x 9 taps
    for k in kernels:
        for stride, pad_lo in ((1, 1), (2, 1), (2, 0), (1, 0)):
            out.append(_case(f"c3fast-{k}-9x7-s{stride}p{pad_lo}-64to72", force=k, F=3, H=9, W=7, Cin=64, Cout=72, stride=stride,
                             pad_lo=pad_lo, epi="bias"))
        out.append(_case(f"c3fast-{k}-10x16-s1p1-320to4", force=k, F=3, H=10, W=16, Cin=320, Cout=4))
        out.append(_case(f"c3fast-{k}-10x16-s2p0-320to72", force=k, F=4, H=10, W=16, Cin=320, Cout=72, stride=2, pad_lo=0))
        out.append(_case(f"c3fast-{k}-10x16-int-320to72", force=k, F=3, H=10, W=16, Cin=320, Cout=72, inputs="int", epi="none"))
        out.append(_case(f"c3fast-{k}-9x7-int-stream-64to72", force=k, F=5, H=9, W=7, Cin=64, Cout=72, inputs="int", epi="stream"))
        out.append(_case(f"c3fast-{k}-9x7-res16", force=k, F=3, H=9, W=7, Cin=64, Cout=72, epi="bias_res16"))
        out.append(_case(f"c3fast-{k}-9x7-stream-res32", force=k, F=3, H=9, W=7, Cin=64, Cout=72, stride=2, epi="stream_res32"))
        out.append(_case(f"c3fast-{k}-10x16-strided", force=k, F=3, H=10, W=16, Cin=64, Cout=72, strided=True))
        out.append(_case(f"c3fast-{k}-9x7-s2p0-strided", force=k, F=3, H=9, W=7, Cin=64, Cout=72, stride=2, pad_lo=0, strided=True))
    # ---- 3x3 general mode (2-stage kernel only): K tail inside a K-tile (Cin = 8: K = 72), Cin = 72, nearest x2, f32 x
    for cin in (8, 72):
        for stride, pad_lo in ((1, 1), (2, 1), (2, 0)):
            out.append(_case(f"c3gen-{cin}to72-s{stride}p{pad_lo}", force="default", expect=K_TWO_STAGE, F=3, H=9, W=7, Cin=cin,
                             Cout=72, stride=stride, pad_lo=pad_lo))
        out.append(_case(f"c3gen-{cin}to4-int", force="default", expect=K_TWO_STAGE, F=3, H=10, W=16, Cin=cin, Cout=4, inputs="int",
                         epi="none"))
    out.append(_case("c3gen-ups-64to72", force="default", expect=K_TWO_STAGE, F=3, H=5, W=7, Cin=64, Cout=72, ups=True))
    out.append(_case("c3gen-ups-72to72-res16", force="ring", expect=K_TWO_STAGE, F=3, H=5, W=4, Cin=72, Cout=72, ups=True,
                     epi="bias_res16"))
    out.append(_case("c3gen-ups-8to72-strided", force="default", expect=K_TWO_STAGE, F=2, H=5, W=7, Cin=8, Cout=72, ups=True,
                     strided=True))
    out.append(_case("c3-x32-fast-64to72", x32=True, force="ring", F=3, H=9, W=7, Cin=64, Cout=72, epi="stream_res32"))
    out.append(_case("c3-x32-fast-s2p0-320to72", x32=True, force="default", F=3, H=10, W=16, Cin=320, Cout=72, stride=2, pad_lo=0))
    out.append(_case("c3-x32-gen-8to72", x32=True, force="default", F=3, H=9, W=7, Cin=8, Cout=72, stride=2))
    out.append(_case("c3-x32-ups-64to72-int", x32=True, force="default", F=2, H=5, W=7, Cin=64, Cout=72, ups=True, inputs="int",
                     epi="stream"))
    # ---- temporal conv on all three kernels: no halo (descriptor), halos (select), clips, P = 37 (frames straddle tiles), F = 2
    for k in kernels:
        for halo in ("none", "both", "lo", "hi"):
            out.append(_case(f"t3-{k}-F8P37-halo-{halo}", kind="t3", force=k, F=8, H=37, W=1, Cin=64, Cout=72, halo=halo))
        for clip in (8, 4, 1):
            out.append(_case(f"t3-{k}-F8P37-clip{clip}", kind="t3", force=k, F=8, H=37, W=1, Cin=128, Cout=72, clip=clip,
                             epi="bias_res16"))
        out.append(_case(f"t3-{k}-F2P37-none", kind="t3", force=k, F=2, H=37, W=1, Cin=64, Cout=4))
        out.append(_case(f"t3-{k}-F2P37-both", kind="t3", force=k, F=2, H=37, W=1, Cin=64, Cout=4, halo="both"))
        out.append(_case(f"t3-{k}-F2P37-clip1", kind="t3", force=k, F=2, H=37, W=1, Cin=64, Cout=72, clip=1))
        out.append(_case(f"t3-{k}-F6P150-int-320", kind="t3", force=k, F=6, H=150, W=1, Cin=320, Cout=72, inputs="int", epi="none",
                         clip=3))
        out.append(_case(f"t3-{k}-F4P37-int-stream-both", kind="t3", force=k, F=4, H=37, W=1, Cin=320, Cout=72, inputs="int",
                         epi="stream", halo="both"))
        out.append(_case(f"t3-{k}-F8P37-stream-res32", kind="t3", force=k, F=8, H=37, W=1, Cin=64, Cout=72, clip=4,
                         epi="stream_res32"))
        out.append(_case(f"t3-{k}-F8P37-strided-none", kind="t3", force=k, F=8, H=37, W=1, Cin=64, Cout=72, strided=True))
        out.append(_case(f"t3-{k}-F8P37-strided-clip2", kind="t3", force=k, F=8, H=37, W=1, Cin=64, Cout=72, strided=True, clip=2))
        out.append(_case(f"t3-{k}-F4P37-strided-both", kind="t3", force=k, F=4, H=37, W=1, Cin=64, Cout=72, strided=True,
                         halo="both"))
    out.append(_case("t3-x32-F4P37-none", kind="t3", x32=True, force="ring", F=4, H=37, W=1, Cin=64, Cout=72, clip=2))
    out.append(_case("t3-x32-F4P37-both", kind="t3", x32=True, force="default", F=4, H=37, W=1, Cin=64, Cout=72, halo="both"))
    # ---- split-K by the library's own plan: the deepest U-Net level, 16 x 5 x 8 pixels, 1280 -> 1280 channels
    for k in ("2stage", "ring"):
        out.append(_case(f"c3fast-{k}-splitk-1280", force=k, F=16, H=5, W=8, Cin=1280, Cout=1280, inputs="int", epi="stream",
                         split=True))
        out.append(_case(f"t3-{k}-splitk-1280", kind="t3", force=k, F=16, H=40, W=1, Cin=1280, Cout=1280, inputs="int",
                         epi="stream", split=True))
    # ---- the shipped rule, unforced: shapes on which choose_kernel itself picks a kernel (256 CUs; found by scanning
    # pm_debug_conv_kernel_choice - the GPU test asserts the choice, so a changed rule fails here instead of silently moving the
    # case).  With 16-bit A the rule NEVER picks the 2-stage kernel for the fast 3x3 or the temporal loader: prefer_ring compares
    # nwork / roundup(nwork, CUs) with nwork / roundup(nwork, 2 CUs) and the first is never the smaller one; the 2-stage kernel
    # serves these loaders for f32 A (the x32 cases) and when PANDORA_GEMM_RING=0 only.
    out.append(_case("c3fast-default-ring", force="default", expect=K_RING, F=3, H=10, W=16, Cin=64, Cout=72))
    out.append(_case("c3fast-default-ringw", force="default", expect=K_RINGW, F=16, H=48, W=64, Cin=64, Cout=128))
    out.append(_case("t3-default-ring", kind="t3", force="default", expect=K_RING, F=8, H=37, W=1, Cin=64, Cout=72, clip=4))
    out.append(_case("t3-default-ringw", kind="t3", force="default", expect=K_RINGW, F=16, H=3072, W=1, Cin=192, Cout=128, clip=8))
    ids = [c.id for c in out]
    assert len(set(ids)) == len(ids)
    return out


CASES = _cases()


# ---- geometry --------------------------------------------------------------------------------------------------------------------
def taps_of(case):
    return 9 if case.kind == "c3" else 3


def out_hw(case):
    """conv3x3: (Ho, Wo) with pad_lo rows / columns of zeros before and one after the (virtual, possibly upsampled) image"""
    hv, wv = (2 * case.H, 2 * case.W) if case.ups else (case.H, case.W)
    return (hv + case.pad_lo - 2) // case.stride + 1, (wv + case.pad_lo - 2) // case.stride + 1


def rows_in(case):
    return case.F * case.H * case.W


def rows_out(case):
    if case.kind == "t3":
        return rows_in(case)
    ho, wo = out_hw(case)
    return case.F * ho * wo


def gather_rows(case, tap):
    """For every output row m of `case` the input row that tap `tap` reads: int64 [M] indexing the rows of
    cat([x, halo_lo, halo_hi]) (x: F*H*W rows, a halo frame: P rows), and -1 where the tap is zero padding."""
    m = torch.arange(rows_out(case))
    if case.kind == "c3":
        ho, wo = out_hw(case)
        hv, wv = (2 * case.H, 2 * case.W) if case.ups else (case.H, case.W)
        f, rem = m // (ho * wo), m % (ho * wo)
        oy, ox = rem // wo, rem % wo
        dy, dx = tap // 3, tap % 3
        vy = oy * case.stride + dy - case.pad_lo  # position in the virtual image (the padding sits outside [0, hv) x [0, wv))
        vx = ox * case.stride + dx - case.pad_lo
        ok = (vy >= 0) & (vy < hv) & (vx >= 0) & (vx < wv)
        sy, sx = (vy // 2, vx // 2) if case.ups else (vy, vx)  # nearest x2: virtual pixel (vy, vx) is source pixel (vy/2, vx/2)
        idx = (f * case.H + sy) * case.W + sx
        return torch.where(ok, idx, torch.full_like(idx, -1))
    P, F = case.H * case.W, case.F
    fc_n = case.clip or F
    f, pix = m // P, m % P
    sf = f % fc_n + tap - 1  # source frame inside the clip
    idx = (f + tap - 1) * P + pix
    below, above = sf < 0, sf >= fc_n
    lo = F * P + pix if case.halo in ("both", "lo") else torch.full_like(idx, -1)
    hi = F * P + P + pix if case.halo in ("both", "hi") else torch.full_like(idx, -1)
    return torch.where(below, lo, torch.where(above, hi, idx))


# ---- inputs ----------------------------------------------------------------------------------------------------------------------
def _ints(g, lo, hi, *shape):
    return torch.randint(lo, hi + 1, shape, generator=g).float()


def build(case, dtype, seed=0):
    """-> dict of CPU tensors: x [Min, Cin] (f32 when case.x32 else dtype), wp [Cout, taps*Cin] dtype, bias f32 [Cout] or None,
    residual [M, Cout] (dtype / f32) or None, halo_lo / halo_hi [P, Cin] of x's type or None; probes also tap [Cout], ch [Cout]."""
    g = torch.Generator().manual_seed(1000 + seed)
    taps, cin, cout = taps_of(case), case.Cin, case.Cout
    P = case.H * case.W
    d = dict(tap=None, ch=None, bias=None, residual=None, halo_lo=None, halo_hi=None)
    if case.inputs == "probe":
        lim = 100
        d["tap"] = torch.arange(cout) % taps
        d["ch"] = torch.randint(0, cin, (cout,), generator=g)
        w = torch.zeros(cout, taps, cin)
        w[torch.arange(cout), d["tap"], d["ch"]] = 1.0
    else:
        lim = 3
        w = _ints(g, -2, 2, cout, taps * cin)
        w[:, 1::3] = 0
    d["wp"] = w.reshape(cout, taps * cin).to(dtype)
    d["x"] = _ints(g, -lim, lim, rows_in(case), cin).to(torch.float32 if case.x32 else dtype)
    if case.halo in ("both", "lo"):
        d["halo_lo"] = _ints(g, -lim, lim, P, cin).to(d["x"].dtype)
    if case.halo in ("both", "hi"):
        d["halo_hi"] = _ints(g, -lim, lim, P, cin).to(d["x"].dtype)
    if case.epi != "none" and case.inputs == "probe":
        d["bias"] = _ints(g, -20, 20, cout)
    if case.epi in ("bias_res16", "stream_res32"):
        d["residual"] = _ints(g, -100, 100, rows_out(case), cout).to(dtype if case.epi == "bias_res16" else torch.float32)
    return d


def out_dtype(case, dtype):
    return torch.float32 if case.epi in ("stream", "stream_res32") else dtype


def reference(case, d):
    """f64 [M, Cout] of integers: sum over taps of (gathered x rows) @ W_tap^T + bias + residual (every value far below 2^53: exact)"""
    taps, cin = taps_of(case), case.Cin
    P = case.H * case.W
    zeros = torch.zeros(P, cin, dtype=torch.float64)
    rows = torch.cat([d["x"].to(torch.float64), zeros if d["halo_lo"] is None else d["halo_lo"].to(torch.float64),
                      zeros if d["halo_hi"] is None else d["halo_hi"].to(torch.float64),
                      torch.zeros(1, cin, dtype=torch.float64)])  # (last row: what index -1 reads - the zero padding)
    w = d["wp"].to(torch.float64).reshape(case.Cout, taps, cin)
    y = torch.zeros(rows_out(case), case.Cout, dtype=torch.float64)
    for t in range(taps):
        y += rows[gather_rows(case, t)] @ w[:, t].t()
    if d["bias"] is not None:
        y += d["bias"].to(torch.float64)
    if d["residual"] is not None:
        y += d["residual"].to(torch.float64)
    return y


def want(case, d, dtype):
    """the reference as the tensor the op must return, bit for bit (probe values and f32 sums are exact; 16-bit sums round once)"""
    y = reference(case, d)
    if case.inputs == "probe":
        assert y.abs().max().item() < 256
    assert y.abs().max().item() < 2 ** 24
    return y.float().to(out_dtype(case, dtype))


def describe_mismatch(case, d, got, wanted):
    """first wrong element as (output row -> frame, y, x; output channel -> tap, input channel), for the assertion message"""
    bad = (got.float() != wanted.float()).nonzero()
    if bad.numel() == 0:
        return "equal"
    m, co = bad[0].tolist()
    if case.kind == "c3":
        ho, wo = out_hw(case)
        where = f"frame {m // (ho * wo)} oy {m % (ho * wo) // wo} ox {m % wo}"
    else:
        P = case.H * case.W
        where = f"frame {m // P} pixel {m % P}"
    what = f"tap {d['tap'][co].item()} channel {d['ch'][co].item()}" if d["tap"] is not None else "integer sum"
    rows = sorted(set(bad[:, 0].tolist()))
    return (f"{case.id}: {bad.shape[0]} wrong elements in {len(rows)} rows (first rows {rows[:8]}); first at row {m} ({where}) "
            f"column {co} ({what}): got {got[m, co].item()} want {wanted[m, co].item()}")
