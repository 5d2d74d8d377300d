"""ORACLE (test infrastructure): attention inputs whose result is exact in f16 and bf16, a closed-form reference and the ONE case
table of the exact attention tests (tests/test_attn_exact_cpu.py: the closed form equals an f64 softmax attention bit for bit;
tests/test_attn_exact_gpu.py: every attention kernel equals the closed form bit for bit).

Construction, per (batch element, head) - an "instance":
  * the keys are partitioned into groups of 1, 2 or 4 keys; every group has its own label of L bits.  Key j carries the code
    c(label) in {+1, -1}^D times an amplitude ak: channel d holds bit d % L of the label (D = 64, L = 16: each of the four
    16-channel k-steps of the MFMA kernels carries all 16 bits).  Query i carries A * c(label of the group it selects);
  * the score of a query against a key of its group is D * q' * ak (q' = what the kernel makes of A: `q_effective`), against any
    other key at most that minus 2 * (D / L) * q' * ak (one differing bit).  `amplitudes` picks ak so that this gap is >= 192
    in base-2 units: the softmax weight of every other key is exp2(<= -192) = 0 in f32 (flushed or not: 2^-149 is the
    smallest f32), so - whenever the winners arrive, whatever stale maximum a kernel keeps - the row sum is exactly the group
    size (a power of two), the only exp2 arguments that matter are 0 and "below -149", and a mean that is 0 comes back as 0;
  * all keys of a group have the SAME code, so their scores are bit-identical in any summation order: exact ties;
  * v holds integers in [-8, 8]: the mean over 1, 2 or 4 rows is a multiple of 0.25 (two segments: mean1 + w2 * mean2 with
    w2 in {1, 0.5}, a multiple of 0.125 of magnitude <= 16) - exact in f32, f16 and bf16.
  * groups, labels, the query -> group map and the positions of tied keys are drawn afresh per instance: a kernel that mixes up
    heads, batch elements, tiles or ring stages returns another key's row, and `describe_mismatch` names that key.
Every operand value is a small integer (times a power of two): it round-trips through f16, bf16 and - the fp8 cases - e4m3.

`want` is the closed form (group means by index arithmetic): it computes no score, no softmax."""
import collections
import functools
import random

import numpy as np
import torch

KV_TILE = 64          # keys per tile of the MFMA kernels (csrc/attn_common.hpp)
LOG2E = 1.4426950408889634
MIN_GAP = 192.0       # base-2 units; exp2(-149) is the smallest f32 - see the module docstring
V_MAX = 8

_FIELDS = dict(
    id=None,
    kind="self",        # "self" pm_attention one segment / "cross" two segments / "fp8" pm_attention_fp8 (+ packed) /
                        # "generic" pm_attention_generic / "temporal" pm_attention_temporal (B = pixels, Nq / Nk = frames)
    B=2, heads=3, Nq=64, Nk=64, D=64,
    L=16,               # label bits
    prescaled=False,    # q already carries scale * log2 e (scale = ln 2 at the C ABI)
    Nk2=0, w2=1.0,      # cross: the second segment (per batch element); the first is ONE [1, Nk, C] tensor for all of them
    strided=False,      # operands are column slices of wider (fused) buffers with NaN around them, the output has guards
    long=False,         # must run on attn_self16_kernel by the shipped rule (Nq, Nk >= 4096)
    mea=False,          # also through memory_efficient_attention on (B * heads, N, 64) tensors (it never prescales)
)
Case = collections.namedtuple("Case", list(_FIELDS))


def _case(id, **kw):
    f = dict(_FIELDS, id=id, **kw)
    assert set(f) == set(_FIELDS), set(f) - set(_FIELDS)
    return Case(**f)


def _cases():
    out = []
    # ---- one segment, Nq = Nk: 40 (one ragged tile, first and last), 64 | 65 (no ragged tile | a ragged tile of one key),
    # 448 (7 whole tiles: one unrolled trip + two remainder tiles, the last key fetched through the buffer descriptor),
    # 488 (the same + a ragged tile of 40)
    for n in (40, 64, 65, 448, 488):
        out.append(_case(f"self-N{n}", Nq=n, Nk=n, prescaled=(n in (65, 448)), mea=(n == 488)))
    out.append(_case("self-N488-prescaled", Nq=488, Nk=488, prescaled=True))
    out.append(_case("self-N448-B3h1", B=3, heads=1, Nq=448, Nk=448))  # batch stride != heads * head stride
    out.append(_case("self-Nq130-Nk488", Nq=130, Nk=488))               # a query tile with 2 valid rows
    out.append(_case("self-Nq300-Nk64", Nq=300, Nk=64, prescaled=True))
    out.append(_case("self-N488-fused", Nq=488, Nk=488, strided=True))  # q | k | v = column slices of [B, N, 3C]
    out.append(_case("self-N448-fused-prescaled", Nq=448, Nk=448, strided=True, prescaled=True))
    out.append(_case("self-N4136-long", B=1, heads=2, Nq=4136, Nk=4136, long=True, prescaled=True))  # 64 tiles + 40 keys
    # ---- two segments: 77 text keys shared by all batch elements (batch stride 0) + 16 image keys per batch element
    for nq in (160, 40):
        for w2 in (1.0, 0.5):
            out.append(_case(f"cross-Nq{nq}-w{w2}", kind="cross", B=4, heads=5, Nq=nq, Nk=77, Nk2=16, w2=w2,
                             prescaled=(nq == 40)))
    out.append(_case("cross-Nq160-w0.5-strided", kind="cross", B=4, heads=5, Nq=160, Nk=77, Nk2=16, w2=0.5, strided=True))
    # ---- temporal: keys are frames (<= 16, 4-bit labels); 8800 problems > 4 * 2048: the capped grid's second trip
    out.append(_case("temporal-F16-P37", kind="temporal", B=37, heads=5, Nq=16, Nk=16, L=4, strided=True))
    out.append(_case("temporal-Fq2-Fk16-P37", kind="temporal", B=37, heads=5, Nq=2, Nk=16, L=4, strided=True))
    out.append(_case("temporal-F5-P37", kind="temporal", B=37, heads=5, Nq=5, Nk=5, L=4, strided=True))
    out.append(_case("temporal-F16-P1100-h8", kind="temporal", B=1100, heads=8, Nq=16, Nk=16, L=4, strided=True))
    # ---- generic head dims
    out.append(_case("generic-D8-Nq70-Nk64", kind="generic", B=3, heads=2, D=8, L=8, Nq=70, Nk=64))
    out.append(_case("generic-D80-N257", kind="generic", B=2, heads=3, D=80, Nq=257, Nk=257))
    out.append(_case("generic-D128-Nq5-Nk1000", kind="generic", B=2, heads=3, D=128, Nq=5, Nk=1000))
    # ---- fp8: whole tiles | a ragged tile
    for n in (192, 232):
        out.append(_case(f"fp8-N{n}", kind="fp8", Nq=n, Nk=n))
    out.append(_case("fp8-N232-prescaled", kind="fp8", Nq=232, Nk=232, prescaled=True))
    ids = [c.id for c in out]
    assert len(set(ids)) == len(ids)
    return out


CASES = _cases()


# ---- geometry --------------------------------------------------------------------------------------------------------------------
def tiles(nk):
    """(number of 64-key tiles, number of whole tiles)"""
    nkt = (nk + KV_TILE - 1) // KV_TILE
    return nkt, (nkt if nk % KV_TILE == 0 else nkt - 1)


def tile_class(key, nk):
    """"first" (tile 0, careful), "fast" (a whole tile behind it) or "ragged" (the careful masked last tile)"""
    nkt, last_full = tiles(nk)
    t = key // KV_TILE
    return "first" if t == 0 else ("fast" if t < last_full else "ragged")


def seg_lengths(case):
    return [case.Nk] + ([case.Nk2] if case.kind == "cross" else [])


def scale_of(case):
    """the softmax scale as the op passes it to the C ABI"""
    if case.kind == "generic":
        return float(case.D) ** -0.5
    if case.prescaled:
        return float(np.log(2.0))
    return 64 ** -0.5


def scale_log2e_f32(case):
    """scale * log2 e as the launchers form it: an f32 product of the f32 scale"""
    return np.float32(np.float32(scale_of(case)) * np.float32(LOG2E))


def q_effective(case, q, dtype, rounded):
    """f64 tensor of what multiplies k in the kernel's base-2 score, made of the q tensor as the kernels do it:
      prescaled one-segment kernels: q itself;
      attn_self_kernel / attn_self16_kernel (rounded=True): round16(q * scale * log2 e), f32 product rounded to `dtype`;
      attn_kernel, tattn_kernel, attn_small_kernel (rounded=False): the f32 product, unrounded (they scale scores or q in f32);
      attn_fp8_pack_kernel: the f32 product rounded to e4m3."""
    if case.prescaled and case.kind in ("self", "fp8"):
        return q.double()
    prod = q.float() * torch.tensor(scale_log2e_f32(case))
    if case.kind == "fp8":
        return prod.to(torch.float8_e4m3fn).double()
    return prod.to(dtype).double() if rounded else prod.double()


def amplitudes(case):
    """(A, ak): |q| and |k| elements.  A = 4 where q is taken as prescaled, else 16 - except the fp8 kernel, whose pack pass
    rounds q * scale * log2 e to e4m3: there A = 22 (on the e4m3 grid: 1.375 * 2^4), because 22 * 0.125 * log2 e = 3.967
    rounds to the grid point 4.0 from 0.09 above the rounding boundary 3.875 and 0.28 below 4.25 - nowhere near either, so q'
    is exactly +-4.0 in every element whatever the last bit of the f32 product (asserted in `build`).  ak: the smallest power
    of two that makes the one-bit score gap 2 * (D / L) * q' * ak >= MIN_GAP (q' taken at its smallest over the treatments)."""
    A = 4.0 if case.prescaled and case.kind != "generic" else (22.0 if case.kind == "fp8" else 16.0)
    one = torch.tensor([A])
    qe = min(q_effective(case, one, dt, r).item() for dt in (torch.float16, torch.bfloat16) for r in (False, True))
    ak = 1.0
    while 2 * (case.D // case.L) * qe * ak < MIN_GAP:
        ak *= 2
    assert ak <= 64 and case.D % case.L == 0
    return A, ak


# ---- instances -------------------------------------------------------------------------------------------------------------------
def _forced_groups(rng, nk, idx):
    """the tie placements every instance of nk keys carries where its tiles allow them (keys drawn afresh per instance):
    first + fast tile; two fast tiles in different ring stages (t % 2 and t % 4 differ); fast + ragged tile; key nk - 1 tied with
    a key of tile 0 (even instances) or winning alone (odd instances); a lone winner in tile 0; four keys spread first to last"""
    nkt, last_full = tiles(nk)
    used = {nk - 1}

    def pick(t):
        lo, hi = t * KV_TILE, min(nk, (t + 1) * KV_TILE)
        free = [k for k in range(lo, hi) if k not in used]
        if not free:
            return None
        k = rng.choice(free)
        used.add(k)
        return k

    groups = []
    if nk >= 2 and idx % 2 == 0:
        groups.append((nk - 1, pick(0)))
    else:
        groups.append((nk - 1,))
    groups.append((pick(0),))
    if last_full >= 2:
        groups.append((pick(0), pick(rng.randrange(1, last_full))))
    if last_full >= 3:
        t1 = rng.randrange(1, last_full - 1)
        groups.append((pick(t1), pick(t1 + 1)))  # neighbours: stages differ for a ring of 2 and of 4
    if last_full >= 2 and last_full < nkt:
        groups.append((pick(rng.randrange(1, last_full)), pick(nkt - 1)))
    if nkt >= 4:
        groups.append((pick(0), pick(nkt // 2), pick(nkt // 2 + 1), pick(nkt - 1)))
    return [g for g in groups if None not in g]


def _partition(rng, nk, forced):
    """forced groups + the remaining keys, shuffled, in groups of 1, 2 or 4 -> list of key tuples"""
    used = {k for g in forced for k in g}
    rest = [k for k in range(nk) if k not in used]
    rng.shuffle(rest)
    groups, i = list(forced), 0
    while i < len(rest):
        m = rng.choice((1, 1, 2, 2, 4))
        while m > len(rest) - i:
            m //= 2
        groups.append(tuple(rest[i:i + m]))
        i += m
    return groups


def _queries(rng, nq, ngroups, nforced, last_gid, idx):
    """query -> group: the forced groups first (as many as there are rows, rotating with the instance), the rest at random,
    shuffled; then row nq - 1 selects the group of the last key and row 0 a forced group"""
    cover = [(idx + i) % nforced for i in range(min(nq, nforced))]
    sel = cover + [rng.randrange(ngroups) for _ in range(nq - len(cover))]
    rng.shuffle(sel)
    if nq > nforced:  # (fewer rows than forced groups: the rotation over instances covers them instead)
        j = sel.index(last_gid)
        sel[j], sel[nq - 1] = sel[nq - 1], sel[j]
        if nq > 1 and sel[0] >= nforced:
            j = next(i for i in range(nq - 1) if sel[i] < nforced)
            sel[j], sel[0] = sel[0], sel[j]
    return sel


@functools.lru_cache(maxsize=None)
def _structure(case):
    """dtype-free part of a case: per segment s  key_gid[s] int64 [Bs, H, Nk_s] (group of every key), key_label[s] (its label),
    sel[s] int64 [B, H, Nq] (the group of segment s every query selects), ngroups[s]; q_label [B, H, Nq]"""
    rng = random.Random(f"attn_exact/{case.id}")
    B, H, Nq = case.B, case.heads, case.Nq
    nlab = 2 ** case.L
    segs = seg_lengths(case)
    key_gid = [[] for _ in segs]
    key_label = [[] for _ in segs]
    sel = [[] for _ in segs]
    q_label = []
    shared = []  # cross: segment 0 is one instance per head, shared by the batch
    if case.kind == "cross":
        for h in range(H):
            forced = _forced_groups(rng, segs[0], h)
            groups = _partition(rng, segs[0], forced)
            labels = rng.sample(range(nlab), len(groups))
            shared.append((groups, labels, len(forced)))
            gid = [0] * segs[0]
            for g, keys in enumerate(groups):
                for k in keys:
                    gid[k] = g
            key_gid[0].append(gid)
            key_label[0].append([labels[g] for g in gid])
    for b in range(B):
        for h in range(H):
            idx = b * H + h
            s = len(segs) - 1  # the segment whose groups the queries pick from (cross: the per-batch image keys)
            forced = _forced_groups(rng, segs[s], idx)
            groups = _partition(rng, segs[s], forced)
            if case.kind == "cross":
                # every group of segment 1 borrows the label of a group of segment 0: the forced groups of segment 0 first
                g0, l0, nf0 = shared[h]
                first = list(range(nf0))
                rng.shuffle(first)
                others = list(range(nf0, len(g0)))
                rng.shuffle(others)
                partner = (first + others)[:len(groups)]
                rng.shuffle(partner)
                labels = [l0[p] for p in partner]
            else:
                labels = rng.sample(range(nlab), len(groups))
            gid = [0] * segs[s]
            for g, keys in enumerate(groups):
                for k in keys:
                    gid[k] = g
            # cross: all groups of the 16-key segment are "forced" (every one is selected, so every borrowed label is used)
            nforced = len(groups) if case.kind == "cross" else len(forced)
            qs = _queries(rng, Nq, len(groups), nforced, gid[segs[s] - 1], idx)
            key_gid[s].append(gid)
            key_label[s].append([labels[g] for g in gid])
            sel[s].append(qs)
            if case.kind == "cross":
                sel[0].append([partner[g] for g in qs])
            q_label.append([labels[g] for g in qs])
    T = lambda rows, bs, n: torch.tensor(rows, dtype=torch.int64).reshape(bs, H, n)
    st = dict(key_gid=[], key_label=[], sel=[], ngroups=[])
    for s, nk in enumerate(segs):
        bs = 1 if (case.kind == "cross" and s == 0) else B
        st["key_gid"].append(T(key_gid[s], bs, nk))
        st["key_label"].append(T(key_label[s], bs, nk))
        st["sel"].append(T(sel[s], B, Nq))
        st["ngroups"].append(int(st["key_gid"][-1].max().item()) + 1)
    st["q_label"] = T(q_label, B, Nq)
    return st


def _codes(case, label):
    """int64 labels [Bs, H, N] -> f32 [Bs, N, H * D] of +-1: channel d of a head holds bit d % L"""
    bits = (label[..., None] >> (torch.arange(case.D) % case.L)) & 1  # [Bs, H, N, D]
    return (2.0 * bits.float() - 1.0).permute(0, 2, 1, 3).reshape(label.shape[0], label.shape[2], case.heads * case.D)


def build(case, dtype, seed=0):
    """-> dict: q [B, Nq, C], k / v [B (cross: 1), Nk, C], k2 / v2 [B, Nk2, C] or None in `dtype` on the CPU, `st` (_structure).
    temporal cases use the same layout with B = pixels and Nq / Nk = frames (`frames_first` turns them for the op)."""
    st = _structure(case)
    A, ak = amplitudes(case)
    g = torch.Generator().manual_seed(2000 + seed)
    C = case.heads * case.D
    d = dict(st=st, k2=None, v2=None, A=A, ak=ak)
    d["q"] = (A * _codes(case, st["q_label"])).to(dtype)
    for s, nk in enumerate(seg_lengths(case)):
        k = (ak * _codes(case, st["key_label"][s])).to(dtype)
        v = torch.randint(-V_MAX, V_MAX + 1, (k.shape[0], nk, C), generator=g).float().to(dtype)
        d["k" if s == 0 else "k2"], d["v" if s == 0 else "v2"] = k, v
    if case.kind == "fp8" and not case.prescaled:
        assert q_effective(case, d["q"], dtype, True).abs().unique().tolist() == [4.0]  # (see `amplitudes`)
    return d


def frames_first(t):
    """[P, F, C] -> the temporal op's [F, P, C]"""
    return t.transpose(0, 1).contiguous()


def _group_means(case, st, s, v):
    """f64 [Bs, H, G, D]: mean of v over the keys of every group of segment s"""
    Bs, nk = v.shape[0], v.shape[1]
    H, D, G = case.heads, case.D, st["ngroups"][s]
    vh = v.double().reshape(Bs, nk, H, D).permute(0, 2, 1, 3)
    gid = st["key_gid"][s]
    sums = torch.zeros(Bs, H, G, D, dtype=torch.float64).scatter_add_(2, gid[..., None].expand(Bs, H, nk, D), vh)
    cnt = torch.zeros(Bs, H, G, dtype=torch.float64).scatter_add_(2, gid, torch.ones(Bs, H, nk, dtype=torch.float64))
    return sums / cnt.clamp_min(1.0)[..., None]


def want(case, d, dtype):
    """the closed form as the tensor the op must return, bit for bit: [B, Nq, C] `dtype`"""
    st, B, H, D = d["st"], case.B, case.heads, case.D
    y = torch.zeros(B, H, case.Nq, D, dtype=torch.float64)
    for s, (v, w) in enumerate(((d["v"], 1.0), (d["v2"], case.w2))):
        if v is None:
            continue
        means = _group_means(case, st, s, v).expand(B, H, -1, D)
        y += w * torch.gather(means, 2, st["sel"][s][..., None].expand(B, H, case.Nq, D))
    out = y.permute(0, 2, 1, 3).reshape(B, case.Nq, H * D)
    assert torch.equal(out.to(dtype).double(), out) and out.abs().max().item() <= 2 * V_MAX  # exact in the output type
    return out.to(dtype)


def winners(case, st, s, b, h, row):
    """the keys of segment s that query `row` of instance (b, h) averages"""
    bs = 0 if st["key_gid"][s].shape[0] == 1 else b
    return (st["key_gid"][s][bs, h] == st["sel"][s][b, h, row]).nonzero().flatten().tolist()


def _where(key, nk):
    t = key // KV_TILE
    return f"key {key} (tile {t} [{tile_class(key, nk)}], stage {t % 2} of 2 / {t % 4} of 4)"


def describe_mismatch(case, d, got, wanted):
    """The first wrong row, for the assertion message: batch, head, query row; the keys that should have been averaged; and
    what the row that came back IS - NaN, some key's V row, the mean of a subset of the right keys, the mean with the last key
    counted once per clamped row of a ragged tile (a missing key mask), another group's mean - with key, tile and ring stage."""
    st, H, D = d["st"], case.heads, case.D
    g3, w3 = got.float().reshape(case.B, case.Nq, H, D), wanted.float().reshape(case.B, case.Nq, H, D)
    bad = ((g3 != w3) | torch.isnan(g3)).any(-1).nonzero()
    if bad.numel() == 0:
        return "equal"
    b, row, h = bad[0].tolist()
    r = g3[b, row, h].double()
    msg = [f"{case.id}: {bad.shape[0]} wrong rows of {case.B * case.Nq * H}; first: batch {b} head {h} query row {row}"]
    segs = seg_lengths(case)
    vs = [d["v"], d["v2"]]
    for s, nk in enumerate(segs):
        msg.append(f"segment {s} should average " + ", ".join(_where(k, nk) for k in winners(case, st, s, b, h, row)))
    if torch.isnan(r).any():
        msg.append(f"got NaN in {int(torch.isnan(r).sum())} of {D} channels (a read outside the operands, or 0 / 0)")
        return "; ".join(msg)
    if len(segs) == 1:
        nk, v = segs[0], vs[0].double().reshape(-1, segs[0], H, D)
        win = winners(case, st, 0, b, h, row)
        found = False
        for bb in [b] + [x for x in range(v.shape[0]) if x != b]:
            for hh in [h] + [x for x in range(H) if x != h]:
                hit = (v[bb, :, hh] == r).all(-1).nonzero().flatten().tolist()
                if hit and not found:
                    found = True
                    msg.append(f"got = the V row of batch {bb} head {hh} " + ", ".join(_where(k, nk) for k in hit[:4]))
        for n in range(1, len(win)):
            sub = [c for c in _subsets(win, n) if torch.equal(v[b, list(c), h].mean(0), r)]
            if sub:
                found = True
                missing = sorted(set(win) - set(sub[0]))
                msg.append(f"got = the mean over {list(sub[0])} only: missing " + ", ".join(_where(k, nk) for k in missing))
        clamped = tiles(nk)[0] * KV_TILE - nk
        if clamped and nk - 1 in win:
            wsum = v[b, win, h].sum(0) + clamped * v[b, nk - 1, h]
            if torch.allclose(wsum / (len(win) + clamped), r, atol=0.07, rtol=0.02):
                found = True
                msg.append(f"got = the mean with key {nk - 1} counted {1 + clamped} times: the {clamped} clamped rows of the "
                           f"ragged tile {nk // KV_TILE} are not masked")
        means = _group_means(case, st, 0, vs[0])
        bs = 0 if means.shape[0] == 1 else b
        other = (means[bs, h] == r).all(-1).nonzero().flatten().tolist()
        if other and not found:
            found = True
            keys = (st["key_gid"][0][bs, h] == other[0]).nonzero().flatten().tolist()
            msg.append("got = the mean of another group: " + ", ".join(_where(k, nk) for k in keys))
        if not found:
            msg.append("got matches no V row, subset or group mean of this case")
    msg.append(f"got[:8] {g3[b, row, h, :8].tolist()} want[:8] {w3[b, row, h, :8].tolist()}")
    return "; ".join(msg)


def _subsets(keys, n):
    import itertools
    return list(itertools.combinations(keys, n))


PLACEMENTS = ("first+fast", "fast+fast in two ring stages", "fast+ragged", "last key + a key of tile 0", "last key alone",
              "tile 0 alone, later tiles far below", "row 0", "row Nq-1")


def placements(case, st, s=0):
    """which of PLACEMENTS occur among the rows of segment s of `case` (from the structure itself: the groups the queries select)"""
    nk = seg_lengths(case)[s]
    nkt, _ = tiles(nk)
    seen = set()
    gid_all, sel_all = st["key_gid"][s], st["sel"][s]
    for b in range(case.B):
        for h in range(case.heads):
            gid = gid_all[0 if gid_all.shape[0] == 1 else b, h].tolist()
            members = collections.defaultdict(list)
            for k, g in enumerate(gid):
                members[g].append(k)
            rows = sel_all[b, h].tolist()
            for row, g in enumerate(rows):
                keys = members[g]
                assert keys, (case.id, b, h, row)
                cls = [tile_class(k, nk) for k in keys]
                fast = sorted({k // KV_TILE for k, c in zip(keys, cls) if c == "fast"})
                if "first" in cls and fast:
                    seen.add(PLACEMENTS[0])
                if any(t1 % 2 != t2 % 2 and t1 % 4 != t2 % 4 for t1 in fast for t2 in fast):
                    seen.add(PLACEMENTS[1])
                if fast and "ragged" in cls:
                    seen.add(PLACEMENTS[2])
                if nk - 1 in keys and len(keys) > 1 and any(k < KV_TILE and k != nk - 1 for k in keys):
                    seen.add(PLACEMENTS[3])
                if keys == [nk - 1]:
                    seen.add(PLACEMENTS[4])
                if len(keys) == 1 and keys[0] < KV_TILE and nkt > 1:
                    seen.add(PLACEMENTS[5])
                if row == 0:
                    seen.add(PLACEMENTS[6])
                if row == case.Nq - 1:
                    seen.add(PLACEMENTS[7])
    return seen
