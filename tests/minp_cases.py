"""The min-p floor on top of the fp64 sampler oracle of tests/sampler_cases.py, and the inputs the min-p tests share
(tests/test_minp_cases_cpu.py holds the oracle and ops/reference.py to each other; tests/test_minp_gpu.py runs the
same cases through the MINP variants of the HIP kernels in csrc/sampling.hip).

Definition. The kernels get ``ln_min_p``, one fp32 per row: -inf where the row has no floor, else fp32(ln(min_p)),
the logarithm taken in fp64 on the host and rounded once. A non-greedy row keeps
    {top-k set} & {top-p nucleus of the top-k set, computed WITHOUT the floor} & {x_i >= fp32(mx + ln_min_p)}
where x_i = fp32(logit_i) * fp32(1 / temperature) and mx is the maximum of x over the vocabulary (padding columns
excluded, -inf ignored). Greedy rows ignore the lane. The floor is one fp32 add and a comparison of fp32 numbers: it
is exact, so it adds no undecidable band of its own. A row is decidable exactly when it is in the oracle of
sampler_cases: the drawn token clears the strict top-p threshold and leads the runner-up by DELTA.

Case seeds. The cases mirror sampler_cases.ALL_CASES one for one (same shapes, dtypes, dispatches, temperatures,
top-k and top-p lists, B_ROWS rows) with seeds of their own, 300 above the original's: 401-411 (full rows), 501-503
(column shards), 601-602 (TP ranks). Per-row min_p comes from MIN_PS by a generator seeded with the case seed + 7000.
For these seeds the oracle alone has no undecidable row among the 48 of any case (test_minp_cases_cpu.py asserts
it), and the floor changes the drawn token of several rows per case, so the cases fail on a sampler without it.
Unlike the engine, which stages -inf for greedy rows, the cases put the finite fp32(ln(min_p)) in the lane of greedy
rows too: the kernels themselves must ignore it there.
"""
import math
from dataclasses import replace
from functools import lru_cache

import numpy as np
import torch

import sampler_cases as S
from sampler_cases import (B_ROWS, DELTA, EPS, MAX_UNDECIDABLE, Case, dispatch, gumbel, inputs, philox,  # noqa: F401
                           scaled, thresholds, uniform)

MIN_PS = [0.0, 0.02, 0.1, 0.5, 1.0]
SEED_SHIFT = 300
MINP_RNG_SHIFT = 7000


def _mirror(cases):
    return [replace(c, name="minp-" + c.name, seed=c.seed + SEED_SHIFT) for c in cases]


FULL_ROW_CASES = _mirror(S.FULL_ROW_CASES)  # seeds 401 .. 411
SHARD_CASES = _mirror(S.SHARD_CASES)        # seeds 501 .. 503
TP_CASES = _mirror(S.TP_CASES)              # seeds 601, 602
ALL_CASES = FULL_ROW_CASES + SHARD_CASES + TP_CASES


def ln_of(min_p) -> np.ndarray:
    """fp32(ln(min_p)) per entry, the logarithm in fp64; -inf for 0."""
    return np.array([-np.inf if m == 0 else np.float32(math.log(float(m))) for m in np.atleast_1d(min_p)],
                    dtype=np.float32)


@lru_cache(maxsize=None)
def min_ps(case: Case) -> np.ndarray:
    return np.random.default_rng(case.seed + MINP_RNG_SHIFT).choice(MIN_PS, B_ROWS)


def ln_min_p(case: Case) -> np.ndarray:
    """The case's lane [B] fp32 (finite on greedy rows too, see the module docstring)."""
    return ln_of(min_ps(case))


def floor_of(x32: np.ndarray, ln: float) -> np.float32:
    """fp32(mx + ln_min_p) of a row of fp32 scaled logits (columns past the vocabulary already cut)."""
    return np.float32(np.float32(x32.max()) + np.float32(ln))


def oracle_row(x32: np.ndarray, t: float, k: int, p: float, seed: int, eps_fn, ln: float):
    """sampler_cases.oracle_row with the floor: (token, decidable, lead)."""
    V = x32.size
    idx = np.flatnonzero(x32 > -np.inf)
    if idx.size == 0:
        return 0, True, np.inf
    x = x32[idx].astype(np.float64)
    if S.is_greedy(t, k):
        return int(idx[np.argmax(x)]), True, np.inf  # greedy rows ignore the floor
    _, thr_strict, thr_loose = thresholds(x, k, p, V, eps_fn)  # the nucleus of the distribution without the floor
    keep = (x >= thr_loose) & (x32[idx] >= floor_of(x32[idx], ln))  # fp32 >= fp32: exact
    x, idx = x[keep], idx[keep]
    v = x + gumbel(idx, seed)
    w = int(np.argmax(v))
    lead = np.inf if v.size == 1 else float(v[w] - np.max(np.delete(v, w)))
    return int(idx[w]), bool(x[w] >= thr_strict and lead >= DELTA), lead


@lru_cache(maxsize=None)
def oracle(case: Case, with_floor: bool = True):
    """(tokens [B] int64, decidable [B] bool) of a case; ``with_floor`` False: the same rows without min-p."""
    inp = inputs(case)
    rows = inp.logits[:, :case.V].float().numpy()
    lane = ln_min_p(case)
    toks, dec = [], []
    for b in range(rows.shape[0]):
        t, k, p = float(inp.temp[b]), int(inp.topk[b]), float(inp.topp[b])
        tok, ok, _ = oracle_row(scaled(rows[b], t, k), t, k, p, int(inp.seeds[b]), EPS[case.eps],
                                float(lane[b]) if with_floor else -np.inf)
        toks.append(tok)
        dec.append(ok)
    return np.array(toks, dtype=np.int64), np.array(dec, dtype=bool)


def check_tokens(got, case: Case):
    """``got`` equals the oracle on every decidable row, and at most MAX_UNDECIDABLE of the rows are not."""
    want, dec = oracle(case)
    got = np.asarray(got, dtype=np.int64)
    assert 1.0 - dec.mean() <= MAX_UNDECIDABLE, f"{case.name}: {(~dec).sum()} of {dec.size} rows undecidable"
    bad = np.flatnonzero(dec & (got != want))
    inp, mp = inputs(case), min_ps(case)
    assert bad.size == 0, (case.name, [(int(b), int(got[b]), int(want[b]), float(inp.temp[b]), int(inp.topk[b]),
                                        float(inp.topp[b]), float(mp[b]), int(inp.seeds[b])) for b in bad[:8]])


# ------------------------------------------------------------------------------------------ exact-boundary rows
# Temperature 1, top-k 0, top-p 1 (the path that builds no histogram), ln_min_p = -2.0 given directly. One token at
# the maximum, one exactly on the floor (kept), one at the next representable bf16 value below the floor (cut), every
# other token at -30. Two kinds: "exact" - maximum 3.0, floor 1.0, cut 1.0 - 2^-8; "zero" - maximum 2.0, floor +0.0,
# the kept token at -0.0 (equal to the floor as floats, below it as sign-magnitude keys), cut -2^-100.
# The seeds were searched on the CPU (the oracle alone): rows 0-5 draw the token on the floor, rows 6-11 the maximum,
# and in rows 12-17 the cut token would have won had it been kept. All rows are decidable.
BND_LN = -2.0
BND_TOK_MAX, BND_TOK_KEPT, BND_TOK_CUT = 17, 905, 5
BND_KINDS = {"exact": (3.0, 1.0, 1.0 - 2.0 ** -8), "zero": (2.0, -0.0, -2.0 ** -100)}
BND_SEEDS = {kind: [10, 12, 16, 17, 39, 44, 0, 1, 3, 4, 5, 6, 2, 14, 21, 25, 33, 51] for kind in BND_KINDS}


def boundary_rows(kind: str, V: int, dtype=torch.float32) -> torch.Tensor:
    mx, kept, cut = BND_KINDS[kind]
    x = torch.full((len(BND_SEEDS[kind]), V), -30.0, dtype=torch.float32)
    x[:, BND_TOK_MAX], x[:, BND_TOK_KEPT], x[:, BND_TOK_CUT] = mx, kept, cut
    x = x.to(dtype)
    assert x.float()[0, BND_TOK_CUT].item() == cut and x.float()[0, BND_TOK_MAX].item() + BND_LN == float(kept)
    assert math.copysign(1.0, x.float()[0, BND_TOK_KEPT].item()) == math.copysign(1.0, kept)
    return x


def boundary_scan(kind: str, seeds):
    """Per seed: (the oracle's token, decidable, the token that would win if the cut token were kept)."""
    mx, kept, cut = BND_KINDS[kind]
    row = np.full(1000, -30.0, dtype=np.float32)
    row[BND_TOK_MAX], row[BND_TOK_KEPT], row[BND_TOK_CUT] = mx, kept, cut
    out = []
    for s in seeds:
        tok, ok, _ = oracle_row(row, 1.0, 0, 1.0, int(s), S.eps_v3, BND_LN)
        three = np.array([BND_TOK_MAX, BND_TOK_KEPT, BND_TOK_CUT])
        v = row[three].astype(np.float64) + gumbel(three, int(s))
        out.append((tok, ok, int(three[np.argmax(v)])))
    return out


@lru_cache(maxsize=None)
def boundary_oracle(kind: str):
    """Tokens of the boundary rows (any vocabulary >= 1000: the -30 tokens are cut by the floor whatever their noise)."""
    scan = boundary_scan(kind, BND_SEEDS[kind])
    assert all(ok for _, ok, _ in scan)
    return np.array([t for t, _, _ in scan], dtype=np.int64)


# ------------------------------------------------------------------------------------------ tied maxima
TIE_V = 1000
TIE_TOKENS = [3, 250, 251, 999]  # the maxima, all at TIE_MAX; the next value is one bf16 step below
TIE_MAX = 2.5
TIE_N = 4096


def tie_row(dtype=torch.bfloat16) -> torch.Tensor:
    """TIE_TOKENS at 2.5, token 500 at the next bf16 below 2.5, the rest spread over [-6, 2]."""
    x = (torch.arange(TIE_V, dtype=torch.float32) % 65) * 0.125 - 6.0
    x[500] = TIE_MAX - 2.0 ** -6
    x[TIE_TOKENS] = TIE_MAX
    x = x.to(dtype)
    assert int((x.float() == TIE_MAX).sum()) == len(TIE_TOKENS) and float(x.float().max()) == TIE_MAX
    return x


@lru_cache(maxsize=None)
def tie_oracle():
    """min_p = 1 (ln 0.0), temperature 1, top-k 0, top-p 1, seeds 0 .. TIE_N - 1: (tokens, decidable)."""
    row = tie_row().float().numpy()
    res = [oracle_row(row, 1.0, 0, 1.0, s, S.eps_v3, 0.0) for s in range(TIE_N)]
    return np.array([r[0] for r in res], dtype=np.int64), np.array([r[1] for r in res], dtype=bool)


def tie_chi2(tokens) -> float:
    """Pearson's statistic of the counts against uniform over TIE_TOKENS; infinite if any other token was drawn."""
    tokens = np.asarray(tokens, dtype=np.int64)
    if not np.isin(tokens, TIE_TOKENS).all():
        return float("inf")
    counts = np.array([(tokens == t).sum() for t in TIE_TOKENS], dtype=np.float64)
    exp = tokens.size / len(TIE_TOKENS)
    return float(((counts - exp) ** 2 / exp).sum())


# ------------------------------------------------------------------------------------------ distribution
# (top-k, top-p, temperature, min_p) on sampler_cases.dist_row: the floor alone (23 tokens of 64 stay); inside a
# top-k of 10 (6 stay); and with top-p 0.95 at temperature 0.7, where the nucleus has 17 tokens and the floor keeps 13.
DIST_PARAMS = [(0, 1.0, 1.0, 0.06), (10, 1.0, 1.0, 0.5), (0, 0.95, 0.7, 0.1)]
DIST_GAP = 1e-3


@lru_cache(maxsize=None)
def dist_oracle(k: int, p: float, t: float, min_p: float, family: str):
    """sampler_cases.dist_oracle with the floor: (tokens, decidable, kept token ids, their exact probabilities)."""
    x32 = scaled(S.dist_row().float().numpy(), t, k)
    x = x32.astype(np.float64)
    _, strict, loose = thresholds(x, k, float(np.float32(p)), S.DIST_V, S.eps_v3)
    assert strict == loose, "the distribution row must have an unambiguous nucleus"
    ln = float(ln_of(min_p)[0])
    floor = floor_of(x32, ln)
    assert np.abs(x - (float(x32.max()) + ln)).min() > DIST_GAP, "a scaled value lies within 1e-3 of the floor"
    kept = np.flatnonzero((x >= loose) & (x32 >= floor))
    pr = np.exp(x[kept] - x[kept].max())
    pr /= pr.sum()
    seeds = S.dist_seeds(family)
    v = x[kept][None, :] + gumbel(kept[None, :], seeds[:, None])
    order = np.sort(v, axis=1)
    dec = (order[:, -1] - order[:, -2]) >= DELTA
    return kept[np.argmax(v, axis=1)], dec, kept, pr
