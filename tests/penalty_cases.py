"""Shared inputs and an fp64 oracle for the repetition / presence / frequency penalties
(tests/test_penalty_cases_cpu.py runs the CPU definition of ops/reference.py and a set of deliberately wrong
definitions through them, tests/test_penalties_gpu.py the HIP kernels of csrc/penalties.hip).

Semantics. A row's known tokens are prompt + output. c[v] = occurrences of v in the output, seen[v] = v occurs in
the prompt or the output. Per column v < vocab, in this order: x = logit; seen -> x = x > 0 ? x / r : x * r;
c > 0 -> x = x - (f * c + p); one rounding to the logits' dtype. Rows with slot -1 and columns >= vocab are copied.

The oracle recomputes seen and c from the token lists of the case and of every call made so far (numpy bincount) in
float64. It never reads a state word and shares no code with ops/reference.py.

Exact cases: logits are multiples of 1/8 with |x| < 32, r in {0.5, 1, 2, 4}, p and f multiples of 1/4, counts <= 8.
Every intermediate (x / r or x * r: a multiple of 1/32 below 128; f * c + p: a multiple of 1/4 below 20; the
difference) is exact in fp32, fused or not, so the expected output is the round-to-nearest-even of the exact value
and the comparison is bit for bit.

General cases (normal logits, r = 1.3, p = 0.7, f = 0.45): |got - want| <= ulp_out(want) + 4 * 2^-24 * M, M the
element's largest intermediate magnitude in the oracle: one output rounding whose tie may flip, and at most four fp32
roundings (the quotient or product, f * c, the sum with p, the difference).

Layout. A case owns a [B, ld] buffer whose columns [off, off + W) are the full-vocabulary logits row (column j =
token j; tokens >= vocab are head padding), so row bases and strides break 16-byte alignment unless the case is an
aligned one. Each state starts as another sequence's words in every row, is rebuilt by penalty_reset for the rows
that hold a slot, and then gets arbitrary words in the columns >= vocab. Calls are (state, lo, width, new tokens):
full-width ones, and pairs of vocabulary shards that each work on a state of their own, as two tensor-parallel ranks
do - the new token lies inside the shard on one and outside it on the other, and the following full-width call must
see it on both.
"""
from dataclasses import dataclass, field
from functools import lru_cache
from typing import List

import numpy as np
import torch

WIDTHS = (1, 7, 8, 9, 255, 256, 257, 4099)
GROUP_EDGE = 2048  # columns per apply workgroup (PEN_GROUPS * 8), csrc/penalties.hip
RESET_EDGE = 4096  # state words per reset workgroup (PEN_RESET_COLS)
R_GEN, P_GEN, F_GEN = np.float32(1.3), np.float32(0.7), np.float32(0.45)


@dataclass
class Case:
    name: str
    exact: bool
    dtype: torch.dtype
    B: int
    W: int  # logits columns (vocab + head padding)
    vocab: int
    ld: int
    off: int  # first logits column inside the [B, ld] buffer
    ooff: int  # the same for the output buffer
    state_cols: int
    S: int
    slots: np.ndarray  # [B] int32, -1: no penalties
    prompts: List[List[int]]
    outputs: List[List[int]]
    rep: np.ndarray
    pres: np.ndarray
    freq: np.ndarray
    base: torch.Tensor = field(repr=False)  # [B, ld]
    garbage: torch.Tensor = field(repr=False)  # [S, state_cols] int32: what the state holds before the reset
    steps: list = field(repr=False, default_factory=list)  # [[(state id, lo, width, new tokens [B]), ...], ...]
    nstates: int = 1


def _ulp_out(want, dtype):
    mant = 7 if dtype == torch.bfloat16 else 23
    a = np.abs(want)
    e = np.floor(np.log2(np.where(a > 0, a, 1.0)))
    e = np.maximum(e, -126.0)
    return 2.0 ** (e - mant)


def oracle(case: Case, b: int, registered: List[int], lo: int, width: int):
    """(want [width] fp64 before the output rounding, M [width], touched [width] bool) of row b's columns
    [lo, lo + width) after ``registered`` further output tokens. touched = the column is penalised at all."""
    x0 = case.base[b, case.off + lo:case.off + lo + width].double().numpy()
    want, M = x0.copy(), np.abs(x0)
    touched = np.zeros(width, dtype=bool)
    if case.slots[b] < 0:
        return want, M, touched
    V = case.vocab
    out = [t for t in case.outputs[b] + list(registered) if t >= 0]
    cnt = np.bincount(np.asarray(out, dtype=np.int64), minlength=V)[:V]
    seen = cnt + np.bincount(np.asarray(case.prompts[b], dtype=np.int64), minlength=V)[:V] > 0
    n = max(0, min(width, V - lo))
    cnt, seen = cnt[lo:lo + n].astype(np.float64), seen[lo:lo + n]
    r, p, f = float(case.rep[b]), float(case.pres[b]), float(case.freq[b])
    x = x0[:n]
    with np.errstate(invalid="ignore"):
        x1 = np.where(seen, np.where(x > 0, x / r, x * r), x)
        fc = f * cnt
        sub = fc + p
        x2 = np.where(cnt > 0, x1 - sub, x1)
    want[:n] = x2
    fin = lambda a: np.where(np.isfinite(a), np.abs(a), 0.0)  # noqa: E731
    M[:n] = np.maximum.reduce([fin(x), fin(x1), fin(fc) * (cnt > 0), fin(sub) * (cnt > 0), fin(x2)])
    touched[:n] = seen
    return want, M, touched


def _bits(t):
    return t.view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


def reset_lists(case: Case):
    """(cu [B + 1] int32, tokens int64, words int32): every row's distinct tokens and finished words."""
    cu, toks, words = [0], [], []
    for b in range(case.B):
        pset = set(case.prompts[b])
        for t in sorted(pset | set(case.outputs[b])):
            w = case.outputs[b].count(t) + ((1 << 31) if t in pset else 0)
            toks.append(t)
            words.append(w - (1 << 32) if w >= (1 << 31) else w)
        cu.append(len(toks))
    return (np.asarray(cu, dtype=np.int32), np.asarray(toks, dtype=np.int64).reshape(-1),
            np.asarray(words, dtype=np.int32).reshape(-1))


def run(case: Case, apply_fn, reset_fn, device="cpu"):
    """Run the case's reset and calls through ``apply_fn`` / ``reset_fn`` (the ops' signatures) and compare every
    output with the oracle. Returns the worst error as a fraction of the bound (0 for exact cases); raises
    AssertionError on the first mismatch."""
    dev = torch.device(device)
    B, W, V = case.B, case.W, case.vocab
    base = case.base.to(dev)
    keep = _bits(base).clone()
    cu, toks, words = (torch.from_numpy(a).to(dev) for a in reset_lists(case))
    slots = torch.from_numpy(case.slots).to(dev)
    rep, pres, freq = (torch.from_numpy(a).to(dev) for a in (case.rep, case.pres, case.freq))
    states = []
    for _ in range(case.nstates):
        st = case.garbage.clone().to(dev)
        reset_fn(st, slots, cu, toks, words)
        st[:, V:] = case.garbage[:, V:].to(dev)
        states.append(st)
    unused = [s for s in range(case.S) if s not in set(case.slots.tolist())]
    registered = [[[] for _ in range(B)] for _ in range(case.nstates)]
    sent = -7.5
    worst = 0.0
    for si, step in enumerate(case.steps):
        for sid, lo, width, new in step:
            lg = base[:, case.off + lo:case.off + lo + width]
            obase = torch.full((B, case.ld), sent, dtype=case.dtype, device=dev)
            out = obase[:, case.ooff + lo:case.ooff + lo + width]
            res = apply_fn(lg, states[sid], slots, torch.from_numpy(new).to(dev), rep, pres, freq, lo, V, out)
            assert res.data_ptr() == out.data_ptr() and res.shape == out.shape, "did not write into out"
            got_all = obase.cpu()
            mask = torch.ones(B, case.ld, dtype=torch.bool)
            mask[:, case.ooff + lo:case.ooff + lo + width] = False
            assert (got_all[mask].float() == sent).all(), f"{case.name}: wrote outside the output view"
            assert torch.equal(_bits(base), keep), f"{case.name}: the raw logits changed"
            got = got_all[:, case.ooff + lo:case.ooff + lo + width]
            for b in range(B):
                if case.slots[b] >= 0 and new[b] >= 0:
                    registered[sid][b].append(int(new[b]))
                want, M, touched = oracle(case, b, registered[sid][b], lo, width)
                src = case.base[b, case.off + lo:case.off + lo + width]
                where = f"{case.name} step {si} state {sid} lo {lo} row {b}"
                same = ~touched
                assert torch.equal(_bits(got[b])[torch.from_numpy(same)], _bits(src)[torch.from_numpy(same)]), \
                    f"{where}: a column that carries no penalty is not a bit-for-bit copy"
                if case.exact:
                    exp = torch.from_numpy(want).float().to(case.dtype)
                    bad = (_bits(exp) != _bits(got[b])).nonzero().flatten().tolist()
                    assert not bad, (f"{where}: columns {bad[:8]} differ: got {got[b][bad[:8]].tolist()}, "
                                     f"want {exp[bad[:8]].tolist()}")
                else:
                    g = got[b].double().numpy()
                    inf = ~np.isfinite(want)
                    assert np.array_equal(g[inf], want[inf]), f"{where}: non-finite values differ"
                    tol = _ulp_out(want[~inf], case.dtype) + 4 * 2.0 ** -24 * M[~inf]
                    err = np.abs(g[~inf] - want[~inf]) / tol
                    if err.size:
                        worst = max(worst, float(err.max()))
                    j = int(np.argmax(err)) if err.size else 0
                    assert not err.size or err.max() <= 1.0, \
                        f"{where}: error {err.max():.3f} x bound at finite column #{j}"
    for sid, st in enumerate(states):  # rows nobody holds keep what they held
        if unused:
            assert torch.equal(st.cpu()[unused], case.garbage[unused]), f"{case.name}: a row without a slot changed"
    return worst


def _words(g, n, V):
    """A sequence's words over n columns: about half the tokens carry a flag, a count or both."""
    w = torch.zeros(n, dtype=torch.int64)
    kind = torch.randint(0, 4, (n,), generator=g)
    cnt = torch.randint(1, 6, (n,), generator=g)
    w = torch.where(kind == 1, torch.full_like(w, 1 << 31), w)
    w = torch.where(kind == 2, cnt, w)
    w = torch.where(kind == 3, cnt + (1 << 31), w)
    w = torch.where(w >= (1 << 31), w - (1 << 32), w)
    return w.to(torch.int32)


def _make(name, exact, dtype, B, W, seed, aligned=False, mismatch=False, shard=None):
    g = torch.Generator().manual_seed(seed)
    pad = 3 if W >= 7 else 0
    V = W - pad
    if aligned:
        off = ooff = 0
        ld = -(-W // 8) * 8 + 8
        state_cols = -(-(V + 5) // 4) * 4
    else:
        off, ooff = 3, (5 if mismatch else 3)
        ld = W + 13 + (1 if (W + 13) % 8 == 0 else 0)
        state_cols = V + 5 + (1 if (V + 5) % 4 == 0 else 0)
    S = 2 * B + 2
    if exact:
        x = torch.randint(-255, 256, (B, ld), generator=g).float() / 8
    else:
        x = torch.randn(B, ld, generator=g) * 4
    x[torch.rand(B, ld, generator=g) < 0.06] = float("-inf")
    base = x.to(dtype)
    slots = np.array([S - 2 - 2 * b for b in range(B)], dtype=np.int32)  # descending, every other row
    if B >= 3:
        slots[1::4] = -1
    rs, ps, fs = (0.5, 2.0, 4.0), (-0.5, 0.25, 1.5, 2.0), (0.25, 0.5, -0.25, 1.0)
    rep, pres, freq = (np.zeros(B, dtype=np.float32) for _ in range(3))
    prompts, outputs, new1, new2 = [], [], np.full(B, -1, dtype=np.int64), np.full(B, -1, dtype=np.int64)
    for b in range(B):
        if exact:
            rep[b], pres[b], freq[b] = rs[b % 3], ps[b % 4], fs[(b // 2) % 4]
            if b % 7 == 6:
                rep[b], pres[b], freq[b] = 1.0, 0.0, 0.0  # a slot with the default values: a copy
        else:
            rep[b], pres[b], freq[b] = R_GEN, P_GEN, F_GEN
        npr = min(V, 2 + V // 5)
        pr = torch.randint(0, V, (npr,), generator=g).tolist()
        no = min(V, 1 + V // 6)
        distinct = torch.randint(0, V, (no,), generator=g).tolist()
        out = []
        for t in dict.fromkeys(distinct):
            out += [t] * int(torch.randint(1, 5, (1,), generator=g))
        for edge in (GROUP_EDGE, RESET_EDGE):  # tokens on both sides of the workgroup chunk edges
            for t in range(edge - 9, edge + 9):
                if t < V and (t + b) % 3 != 2:
                    (pr if (t + b) % 2 else out).append(t)
        fresh = [t for t in range(V) if t not in pr]
        if fresh and fresh[-1] not in out:
            out += [fresh[-1]] * 2  # an output token that the prompt does not hold
        order = torch.randperm(len(out), generator=g).tolist()
        out = [out[i] for i in order]
        out = [t for i, t in enumerate(out) if out[:i].count(t) < 6]  # two more calls may register it: c <= 8
        prompts.append(pr)
        outputs.append(out)
        choices = [0, V - 1, pr[0], -1, GROUP_EDGE - 1 if V > GROUP_EDGE else V // 2,
                   GROUP_EDGE if V > GROUP_EDGE else V // 3]
        new1[b] = choices[b % len(choices)]
        new2[b] = choices[(b + 1) % len(choices)] if b % 2 == 0 else -1
    if V > GROUP_EDGE + 16 and B >= 5:
        # new tokens on the apply workgroups' chunk edge: workgroup k of a row takes the columns
        # [head + 2048 k, head + 2048 (k + 1)), head = the columns before the row's first 16-byte boundary
        held = [b for b in range(B) if slots[b] >= 0]
        unit = 16 // base.element_size()
        for i, b in enumerate(held[:4]):
            e = GROUP_EDGE + ((-(b * ld + off)) % unit if i >= 2 else 0)
            new1[b], new2[b] = (e - 1, e) if i % 2 == 0 else (e, e - 1)
    garbage = torch.stack([_words(g, state_cols, V) for _ in range(S)])
    c = Case(name, exact, dtype, B, W, V, ld, off, ooff, state_cols, S, slots, prompts, outputs, rep, pres, freq,
             base, garbage)
    if shard is None:
        c.steps = [[(0, 0, W, new1)], [(0, 0, W, new2)]]
    else:
        none = np.full(B, -1, dtype=np.int64)
        c.nstates = 2
        c.steps = [[(0, 0, shard, new1), (1, shard, W - shard, new1)], [(0, 0, W, none), (1, 0, W, none)],
                   [(0, 0, shard, new2), (1, shard, W - shard, new2)], [(0, 0, W, none), (1, 0, W, none)]]
    return c


@lru_cache(maxsize=None)
def cases():
    out = {}
    seed = 0
    for exact in (True, False):
        for dtype, dn in ((torch.bfloat16, "bf16"), (torch.float32, "fp32")):
            kind = "exact" if exact else "general"
            specs = [(f"B3-W{W}", dict(B=3, W=W)) for W in WIDTHS]
            specs += [("B1-W257", dict(B=1, W=257)), ("B65-W257", dict(B=65, W=257)),
                      ("B3-W256-aligned", dict(B=3, W=256, aligned=True)),
                      ("B3-W4099-aligned", dict(B=3, W=4099, aligned=True)),
                      ("B3-W257-mismatch", dict(B=3, W=257, mismatch=True)),
                      ("B3-W257-shard13", dict(B=3, W=257, shard=13)),
                      ("B3-W256-aligned-shard128", dict(B=3, W=256, aligned=True, shard=128)),
                      # vocab 4128: reset lists on both sides of state column 4096, new tokens on the apply chunk edge
                      ("B6-W4131", dict(B=6, W=4131)), ("B6-W4131-aligned", dict(B=6, W=4131, aligned=True))]
            for nm, kw in specs:
                seed += 1
                name = f"{kind}-{dn}-{nm}"
                out[name] = _make(name, exact, dtype, seed=seed, **kw)
    return out


def edge_tokens(case: Case, b: int):
    """Where the apply kernel cuts row b between its first two workgroups: the first column of the second one."""
    unit = 16 // case.base.element_size()
    return GROUP_EDGE + (-(b * case.ld + case.off)) % unit


CASE_NAMES = tuple(cases())
EXACT_NAMES = tuple(n for n in CASE_NAMES if n.startswith("exact"))


def penalise_row(x, prompt, output, r, p, f, vocab=None):
    """The fp64 oracle over one full-vocabulary logits row ``x`` from a sequence's token lists (engine tests)."""
    x = np.asarray(x, dtype=np.float64).copy()
    V = x.size if vocab is None else vocab
    cnt = np.bincount(np.asarray(output, dtype=np.int64), minlength=V)[:V].astype(np.float64)
    seen = cnt + np.bincount(np.asarray(prompt, dtype=np.int64), minlength=V)[:V] > 0
    y = x[:V]
    with np.errstate(invalid="ignore"):
        y = np.where(seen, np.where(y > 0, y / float(r), y * float(r)), y)
        y = np.where(cnt > 0, y - (float(f) * cnt + float(p)), y)
    x[:V] = y
    return x
