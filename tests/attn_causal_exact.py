"""Test infrastructure: causal-attention inputs whose result is exact in f16 and bf16, in the manner of oracle/attn_exact.py
(whose code, amplitude and exactness rules are reused), for pm_attention_causal - query row i sees key j iff j <= q_pos0 + i.

Per (batch element, head) instance the keys are partitioned into PAIRS (a < b) that share a 16-bit sign code and SINGLES with a
code of their own; all codes of an instance differ, so a query (A times a code) scores its matching keys at least MIN_GAP
base-2 units above every other key and the softmax is an exact selection.  Query row i, whose last visible key is
t = q_pos0 + i, takes
  * the code of a pair with a <= t < b wherever one exists: one VISIBLE match and one FUTURE match, whose v rows differ - a
    kernel that ignores the mask returns the mean of the two rows, the masked kernel the visible row;
  * on every third row, and where no pair straddles t, the code of a key whose only visible match is key t itself where the
    partition allows it (a pair with a == t, or the single t): the boundary j == q_pos0 + i;
  * else a visible single, or a pair with both keys visible (the mean of two integer rows: still exact).
`want` is index arithmetic: the mean of the v rows of the visible matches."""
import random

import torch

from oracle import attn_exact as ax

CASES = ((5, 5, 0), (64, 64, 0), (65, 65, 0), (77, 77, 0), (3, 70, 67))  # (Nq, Nk, q_pos0)
HEAD_DIMS = (64, 80)
B, HEADS, L = 2, 3, 16


def case_of(Nq, Nk, q_pos0, D):
    return ax._case(f"causal-Nq{Nq}-Nk{Nk}-p{q_pos0}-D{D}", kind="generic", B=B, heads=HEADS, Nq=Nq, Nk=Nk, D=D, L=L)


def _instance(rng, Nq, Nk, q_pos0):
    """-> (key_label [Nk], q_label [Nq], visible matches per row, future matches per row)"""
    # row 0's last visible key q_pos0 (at q_pos0 = 0 the only one it sees) gets a future twin: the boundary j == q_pos0 + i
    later = list(range(q_pos0 + 1, Nk))
    pairs = [(q_pos0, rng.choice(later))] if later else []
    keys = [k for k in range(Nk) if not pairs or k not in pairs[0]]
    rng.shuffle(keys)
    npairs = len(keys) // 3
    for _ in range(npairs):
        a, b = sorted((keys.pop(), keys.pop()))
        pairs.append((a, b))
    singles = sorted(keys)
    labels = rng.sample(range(2 ** L), len(pairs) + len(singles))
    key_label = [0] * Nk
    groups = [tuple(p) for p in pairs] + [(s,) for s in singles]
    for g, lab in zip(groups, labels):
        for k in g:
            key_label[k] = lab
    q_label, vis, fut = [], [], []
    for i in range(Nq):
        t = q_pos0 + i
        straddle = [g for g in groups if len(g) == 2 and g[0] <= t < g[1]]
        edge = [g for g in groups if g[0] == t and (len(g) == 1 or g[1] > t)]  # only visible match: key t itself
        edge.sort(key=len, reverse=True)  # (a pair first: the boundary row then has a future match as well)
        if edge and (i % 3 == 0 or not straddle):
            g = edge[0]
        elif straddle:
            g = rng.choice(straddle)
        else:
            g = rng.choice([g for g in groups if g[0] <= t])
        q_label.append(key_label[g[0]])
        vis.append([k for k in g if k <= t])
        fut.append([k for k in g if k > t])
    return key_label, q_label, vis, fut


def build(Nq, Nk, q_pos0, D, dtype):
    """-> dict: q [B, Nq, C], k / v [B, Nk, C] in `dtype` on the CPU, `want` [B, Nq, C] (the visible matches' mean),
    `unmasked` (the mean over visible AND future matches: what a kernel without the mask returns), vis / fut [b][h][row]."""
    case = case_of(Nq, Nk, q_pos0, D)
    A, ak = ax.amplitudes(case)
    rng = random.Random(case.id)
    C = HEADS * D
    kl, ql, vis, fut = [], [], [], []
    for _ in range(B * HEADS):
        a, b, c, d = _instance(rng, Nq, Nk, q_pos0)
        kl.append(a), ql.append(b), vis.append(c), fut.append(d)
    T = lambda rows, n: torch.tensor(rows, dtype=torch.int64).reshape(B, HEADS, n)
    g = torch.Generator().manual_seed(4000 + Nq + 7 * D)
    out = dict(case=case, q=(A * ax._codes(case, T(ql, Nq))).to(dtype), k=(ak * ax._codes(case, T(kl, Nk))).to(dtype),
               v=torch.randint(-ax.V_MAX, ax.V_MAX + 1, (B, Nk, C), generator=g).float().to(dtype))
    vh = out["v"].double().reshape(B, Nk, HEADS, D)
    want = torch.zeros(B, Nq, HEADS, D, dtype=torch.float64)
    unmasked = torch.zeros_like(want)
    for b in range(B):
        for h in range(HEADS):
            for i in range(Nq):
                v_, f_ = vis[b * HEADS + h][i], fut[b * HEADS + h][i]
                want[b, i, h] = vh[b, v_, h].mean(0)
                unmasked[b, i, h] = vh[b, v_ + f_, h].mean(0)
    for name, t in (("want", want), ("unmasked", unmasked)):
        t = t.reshape(B, Nq, C)
        assert torch.equal(t.to(dtype).double(), t)  # exact in the output type
        out[name] = t.to(dtype)
    out["vis"] = [[vis[b * HEADS + h] for h in range(HEADS)] for b in range(B)]
    out["fut"] = [[fut[b * HEADS + h] for h in range(HEADS)] for b in range(B)]
    return out


def coverage(d, Nq, q_pos0):
    """per instance: rows with one visible + one future match whose v rows differ; rows whose only match is key q_pos0 + i"""
    D = d["case"].D
    vh = d["v"].reshape(B, -1, HEADS, D)
    rows = []
    for b in range(B):
        for h in range(HEADS):
            both = sum(1 for i in range(Nq) if len(d["vis"][b][h][i]) == 1 and len(d["fut"][b][h][i]) == 1
                       and not torch.equal(vh[b, d["vis"][b][h][i][0], h], vh[b, d["fut"][b][h][i][0], h]))
            edge = sum(1 for i in range(Nq) if d["vis"][b][h][i] == [q_pos0 + i])
            rows.append((both, edge))
    return rows
