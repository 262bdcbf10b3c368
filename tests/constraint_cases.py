"""Shared inputs and an fp64 oracle for the token constraints - logit_bias, banned / allowed tokens, min_tokens
(tests/test_constraint_cases_cpu.py runs the CPU definition of ops/reference.py and a set of deliberately wrong
definitions through them, tests/test_constraints_gpu.py the HIP kernel of csrc/constraints.hip).

Semantics, per row with a request and ``nout`` tokens generated so far, for column j = global token v = lo + j:
v >= vocab -> copied; v banned, or an allowed set exists and v is not in it, or nout < min_tokens and v is in the stop
set ({eos} unless ignore_eos, and stop_token_ids) -> -inf; v in logit_bias -> float(x) + fp32(bias), one fp32 add and
one rounding to the logits' dtype; else copied. Rows with slot -1 are copied.

The oracle works from these request-level fields with numpy masks in float64 and never sees a resolved list: the sum
of an fp32-representable logit and an fp32 bias is formed in float64, rounded to fp32 (which is the correctly rounded
fp32 sum: 53 >= 2 * 24 + 2 bits make the double rounding innocuous for an addition) and then to the dtype. So every
comparison is bit for bit, over the whole output buffer including the bytes between the rows.

Layout. A case owns a [B, ld] input buffer whose columns [off, off + W) are the launch's logits (the columns
[lo, lo + W) of the vocabulary; tokens >= vocab are head padding and hold poison: NaN, +inf, huge values) and an output
buffer of the same shape full of a sentinel, written at column ``ooff``. With an odd ``ld`` the row bases take every
16-byte phase. The state holds another request's lists in every slot no row uses.
"""
from dataclasses import dataclass, field
from functools import lru_cache
from typing import Dict, List, Optional

import numpy as np
import torch

from llmss_amd.engine.sampling import MAX_TOKEN_EDITS, SamplingParams
from llmss_amd.ops.reference import pack_token_edits

E = MAX_TOKEN_EDITS
WIDTHS = (1, 7, 8, 9, 2047, 2048, 2049, 4099)
CHUNK = 2048  # columns per workgroup (CON_GROUPS * 8), csrc/constraints.hip
MIN_TOKENS = 3
SENTINEL = -7.5


@dataclass
class Case:
    name: str
    dtype: torch.dtype
    B: int
    W: int
    lo: int
    vocab: int  # the global vocabulary; columns with lo + j >= vocab are padding
    ld: int
    off: int
    ooff: int
    S: int
    slots: np.ndarray  # [B] int32, -1: no constraints
    nout: np.ndarray  # [B] int32
    reqs: Dict[int, SamplingParams]  # slot -> request
    eos: Dict[int, Optional[int]]  # slot -> the engine's EOS token for that request
    base: torch.Tensor = field(repr=False)  # [B, ld]
    garbage: Optional[tuple] = field(repr=False, default=None)  # (ids, vals, meta) of the slots nobody holds


def _bits(t):
    return t.view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


def chunk_edges(case: Case, b: int) -> List[int]:
    """Columns of row b on the kernel's seams: the loose head and tail and the first and last column of every
    workgroup's chunk (the input row's first 16-byte boundary shifts them)."""
    unit = 16 // case.base.element_size()
    head = min((-(b * case.ld + case.off)) % unit, case.W)
    ngroups = (case.W - head) // 8
    tail0 = head + ngroups * 8
    cols = set(range(head)) | set(range(tail0, case.W))
    for k in range(0, ngroups * 8, CHUNK):
        cols |= {head + k, head + min(k + CHUNK, ngroups * 8) - 1}
    return sorted(c for c in cols if 0 <= c < case.W)


def oracle_row(x: torch.Tensor, p: Optional[SamplingParams], eos, nout: int, lo: int, vocab: int) -> torch.Tensor:
    """The expected output row for the logits row ``x`` (columns = tokens lo ..) under request ``p``."""
    out = x.clone()
    if p is None:
        return out
    W = x.shape[0]
    v = lo + np.arange(W)
    inside = v < vocab
    member = lambda ids: np.isin(v, np.asarray(list(ids), dtype=np.int64))  # noqa: E731
    forbidden = member(p.banned_token_ids)
    if len(p.allowed_token_ids) > 0:
        forbidden |= ~member(p.allowed_token_ids)
    if nout < p.min_tokens:
        stop = set(p.stop_token_ids) | (set() if p.ignore_eos or eos is None else {eos})
        forbidden |= member(stop)
    a = np.zeros(W, dtype=np.float64)
    biased = np.zeros(W, dtype=bool)
    for t, val in p.logit_bias.items():
        if lo <= t < lo + W:
            a[t - lo] = np.float64(np.float32(val))
            biased[t - lo] = True
    with np.errstate(invalid="ignore", over="ignore"):
        s = (x.double().numpy() + a).astype(np.float32)
    summed = torch.from_numpy(s).to(x.dtype)
    ninf = torch.full_like(x, float("-inf"))
    f = torch.from_numpy(forbidden & inside)
    e = torch.from_numpy(biased & inside & ~forbidden)
    return torch.where(f, ninf, torch.where(e, summed, out))


def build_state(case: Case, resolve_fn):
    """(edit_ids [S, 2, E], edit_vals, edit_meta [S, 4]) for the case: held slots from ``resolve_fn``, the rest from
    the case's garbage."""
    ids, vals, meta = (torch.from_numpy(a.copy()) for a in case.garbage)
    for s, p in case.reqs.items():
        early, late, fill = resolve_fn(p, case.eos[s], case.vocab)
        i, v, m = pack_token_edits(early, late, fill, p.min_tokens, E)
        ids[s], vals[s], meta[s] = torch.from_numpy(i), torch.from_numpy(v), torch.from_numpy(m)
    return ids, vals, meta


@lru_cache(maxsize=None)
def expected(name: str) -> torch.Tensor:
    """The whole [B, ld] output buffer the case must leave, computed once and shared."""
    c = cases()[name]
    want = torch.full((c.B, c.ld), SENTINEL, dtype=c.dtype)
    for b in range(c.B):
        s = int(c.slots[b])
        want[b, c.ooff:c.ooff + c.W] = oracle_row(c.base[b, c.off:c.off + c.W], c.reqs.get(s), c.eos.get(s),
                                                  int(c.nout[b]), c.lo, c.vocab)
    return want


def run(case: Case, apply_fn, resolve_fn, device="cpu"):
    """Run the case through ``resolve_fn`` (engine.sampling.resolve_token_edits' signature) and ``apply_fn`` (the
    ops' signature) and compare the raw bits of the whole output buffer; raises AssertionError on a mismatch."""
    dev = torch.device(device)
    state = [t.to(dev) for t in build_state(case, resolve_fn)]
    keep_state = [t.clone() for t in state]
    base = case.base.to(dev)
    keep = _bits(base).clone()
    obuf = torch.full((case.B, case.ld), SENTINEL, dtype=case.dtype, device=dev)
    lg = base[:, case.off:case.off + case.W]
    out = obuf[:, case.ooff:case.ooff + case.W]
    res = apply_fn(lg, *state, torch.from_numpy(case.slots).to(dev), torch.from_numpy(case.nout).to(dev), case.lo,
                   case.vocab, out)
    assert res.data_ptr() == out.data_ptr() and res.shape == out.shape, "did not write into out"
    assert torch.equal(_bits(base), keep), f"{case.name}: the input logits changed"
    for t, k in zip(state, keep_state):
        assert torch.equal(t.view(torch.int32), k.view(torch.int32)), f"{case.name}: the state changed"
    got, want = _bits(obuf.cpu()), _bits(expected(case.name))
    if not torch.equal(got, want):
        bad = (got != want).nonzero()
        b, c = (int(i) for i in bad[0])
        raise AssertionError(f"{case.name}: {bad.shape[0]} elements differ, first at row {b} buffer column {c} (logits "
                             f"column {c - case.ooff}, token {case.lo + c - case.ooff}): got "
                             f"{obuf.cpu()[b, c].item()}, want {expected(case.name)[b, c].item()}, input "
                             f"{case.base[b, c - case.ooff + case.off].item() if 0 <= c - case.ooff < case.W else None}")


def _garbage(g, S, vocab):
    ids = torch.stack([torch.stack([torch.randperm(max(vocab, E), generator=g)[:E] for _ in range(2)])
                       for _ in range(S)]).to(torch.int32).numpy()
    vals = (torch.randn(S, 2, E, generator=g) * 8).numpy().astype(np.float32)
    meta = np.tile(np.array([E, E, 1, 2], dtype=np.int32), (S, 1))
    meta[::2, 2] = 0
    return ids, vals, meta


def _pick(g, pool, n):
    pool = sorted(pool)
    idx = torch.randperm(len(pool), generator=g)[:n].tolist()
    return [pool[i] for i in idx]


def _make(name, dtype, B, W, seed, aligned=False, mismatch=False, lo=0, vocab=None, long=False):
    g = torch.Generator().manual_seed(seed)
    pad = 3 if W >= 7 else 0
    vocab = lo + W - pad if vocab is None else vocab
    if aligned:
        off = ooff = 0
        ld = -(-W // 8) * 8 + 8
    else:
        off, ooff = 3, (5 if mismatch else 3)
        ld = W + 13 + (1 if (W + 13) % 2 == 0 else 0)  # odd: the row bases take every 16-byte phase
    x = torch.randn(B, ld, generator=g) * 4
    x[torch.rand(B, ld, generator=g) < 0.06] = float("-inf")
    base = x.to(dtype)
    poison = torch.tensor([float("nan"), float("inf"), 3.0e38, -1.0e30], dtype=dtype)
    for j in range(W):
        if lo + j >= vocab:
            base[:, off + j] = poison[j % 4]
    S = 2 * B + 2
    slots = np.array([S - 2 - 2 * b for b in range(B)], dtype=np.int32)  # descending, every other slot
    if B >= 3:
        slots[1::4] = -1
    nout = np.array([MIN_TOKENS - 1 + (b + seed) % 3 for b in range(B)], dtype=np.int32)  # early, at the edge, late
    case = Case(name, dtype, B, W, lo, vocab, ld, off, ooff, S, slots, nout, {}, {}, base)
    local = [v for v in range(lo, lo + W) if v < vocab]  # this launch's tokens
    far = [v for v in (0, 1, lo - 1, lo + W, lo + W + 1, vocab - 1, vocab - 2) if 0 <= v < vocab
           and not lo <= v < lo + W]  # listed tokens of other shards: before and after this one
    held = 0
    for b in range(B):
        s = int(slots[b])
        if s < 0:
            continue
        kind = (0, 2, 1, 3, 4, 5)[held % 6]
        held += 1
        edges = [lo + c for c in chunk_edges(case, b) if lo + c < vocab] + ([vocab - 1] if vocab - 1 in local else [])
        edges = list(dict.fromkeys(edges))
        n_rand = (E if long else 24)
        pool = set(local) - set(edges)
        eos = local[len(local) // 2] if local else (far[0] if far else None)
        stop = ([edges[0]] if edges else []) + _pick(g, pool, 2)
        kw = dict(max_new_tokens=16, min_tokens=MIN_TOKENS, stop_token_ids=list(dict.fromkeys(stop)))
        bias_of = lambda toks: {t: float(np.float32(torch.empty(1).uniform_(-100, 100, generator=g).item()))  # noqa: E731
                                for t in toks}
        if kind == 0:  # biases only, as many as a list holds when the case is a long one
            toks = list(dict.fromkeys(edges + far + _pick(g, pool, n_rand)))[:E]
            extra = set(kw["stop_token_ids"]) | {eos}
            while len(set(toks) | extra) > E:  # the early list - these and the stop set - fills a long case's slot
                toks.pop()
            kw.update(logit_bias=bias_of(toks))
        elif kind == 1:  # banned tokens and biases that overlap them
            ban = list(dict.fromkeys(edges[::2] + _pick(g, pool, 5) + far[:1]))
            toks = list(dict.fromkeys(edges + far[1:] + (_pick(g, pool, E) if long else [])))
            while len(set(toks) | set(ban)) > E:
                toks.pop()
            kw.update(banned_token_ids=ban, logit_bias=bias_of(toks))
            if long:  # nothing to stop on: the early and the late list both hold E entries
                kw.update(ignore_eos=True, stop_token_ids=[])
        elif kind == 2:  # an allowed set with biases, a banned member, EOS allowed and in the stop set
            allow = list(dict.fromkeys(edges + far + _pick(g, pool, n_rand) + ([eos] if eos is not None else [])))
            allow = allow[:E]
            kw.update(allowed_token_ids=allow, banned_token_ids=list(dict.fromkeys(allow[1:2] + _pick(g, pool, 1))),
                      logit_bias=bias_of(allow[::2] + _pick(g, pool, 2)))
            kw["stop_token_ids"] = list(dict.fromkeys(kw["stop_token_ids"] + allow[3:4]))
            if not set(allow) - set(kw["banned_token_ids"]) - set(kw["stop_token_ids"]) - {eos}:
                kw.update(banned_token_ids=[], stop_token_ids=[], ignore_eos=True)  # a row of one or two columns
        elif kind == 3:  # an allowed set alone
            allow = list(dict.fromkeys(_pick(g, pool, 6) + edges[1::2] + far[:1]))
            kw.update(allowed_token_ids=allow or [0], stop_token_ids=[])
            if len(allow) < 2:  # nothing would be left before min_tokens
                eos = None
        elif kind == 4:  # one banned token, EOS ignored: the early list is the late one plus the stop tokens
            kw.update(banned_token_ids=(edges[-1:] or [0]), ignore_eos=True)
        else:  # min_tokens with nothing to stop on: both lists empty
            kw.update(ignore_eos=True, stop_token_ids=[])
        p = SamplingParams(**kw).validate()
        case.reqs[s], case.eos[s] = p, eos
        # a finite bias over a -inf logit stays -inf
        for t in list(p.logit_bias)[:2]:
            if lo <= t < lo + W:
                base[b, off + t - lo] = float("-inf")
    case.garbage = _garbage(g, S, vocab)
    return case


def _rounding(name, dtype):
    """Sums that need the rounding. bf16 (8 significant bits): 256 + 0.75 -> 256, 256 + 1 (a tie) -> 256 (even),
    258 + 1 (a tie) -> 260, 256 + 1.25 -> 258, 256 + (1 + 2^-10) -> 258 though the bias rounds to 1 in bf16,
    1 + (2^-8 + 2^-20) -> 1 + 2^-7 though the sum rounds to the tie 1 + 2^-8 at 11 significant bits, and the negated
    ones. fp32 (24 bits): the same with 2^16 in place of 2^0 steps."""
    W, vocab, B = 16, 16, 2
    sh = 1.0 if dtype == torch.bfloat16 else 2.0 ** -16
    x = [256.0, 256.0, 258.0, 256.0, 256.0, 1.0, -256.0, -258.0, -1.0, 0.0, float("-inf"), 3.0, 100.0, -100.0, 0.5, 7.0]
    a = [0.75 * sh, 1.0 * sh, 1.0 * sh, 1.25 * sh, (1 + 2.0 ** -10) * sh, (2.0 ** -8 + 2.0 ** -20) * sh, -1.0 * sh,
         -1.0 * sh, -(2.0 ** -8 + 2.0 ** -20) * sh, 0.1, 5.0, -100.0, 100.0, 100.0, 1e-3, -7.0]
    base = torch.tensor([x, x], dtype=torch.float32).to(dtype)
    assert torch.equal(base.float(), torch.tensor([x, x]))
    p = SamplingParams(max_new_tokens=4, logit_bias={i: v for i, v in enumerate(a)}).validate()
    q = SamplingParams(max_new_tokens=4, logit_bias={i: v for i, v in enumerate(a)},
                       allowed_token_ids=list(range(0, 16, 1))).validate()
    c = Case(name, dtype, B, W, 0, vocab, W, 0, 0, 3, np.array([2, 0], dtype=np.int32), np.zeros(B, dtype=np.int32),
             {2: p, 0: q}, {2: None, 0: None}, base)
    c.garbage = _garbage(torch.Generator().manual_seed(99), 3, vocab)
    return c


@lru_cache(maxsize=None)
def cases():
    out = {}
    seed = 100
    for dtype, dn in ((torch.bfloat16, "bf16"), (torch.float32, "fp32")):
        specs = [(f"B3-W{W}", dict(B=3, W=W)) for W in WIDTHS]
        specs += [("B1-W2049", dict(B=1, W=2049)), ("B65-W2049", dict(B=65, W=2049)),
                  ("B8-W4099-long", dict(B=8, W=4099, long=True)),  # every row phase; 512-entry lists
                  ("B3-W2048-aligned", dict(B=3, W=2048, aligned=True)),
                  ("B7-W4099-aligned-long", dict(B=7, W=4099, aligned=True, long=True)),
                  ("B3-W2049-mismatch", dict(B=3, W=2049, mismatch=True)),
                  ("B7-W4099-mismatch", dict(B=7, W=4099, mismatch=True)),
                  # vocabulary shards: listed tokens before, inside and after [lo, lo + W)
                  ("B7-W2049-shard-mid", dict(B=7, W=2049, lo=2000, vocab=6000)),
                  ("B7-W2100-shard-last", dict(B=7, W=2100, lo=4000, vocab=6090)),  # the padded last shard
                  ("B3-W0-shard", dict(B=3, W=0, lo=6000, vocab=6000))]
        for nm, kw in specs:
            seed += 1
            name = f"{dn}-{nm}"
            out[name] = _make(name, dtype, seed=seed, **kw)
        out[f"{dn}-rounding"] = _rounding(f"{dn}-rounding", dtype)
    return out


CASE_NAMES = tuple(cases())


def constrain_row(x, p: SamplingParams, eos, nout: int, vocab=None):
    """The oracle over one full-vocabulary fp64 logits row from a request's fields (engine tests): forbidden tokens
    -inf, biased ones x + fp32(bias)."""
    x = np.asarray(x, dtype=np.float64).copy()
    V = x.size if vocab is None else vocab
    v = np.arange(V)
    forbidden = np.isin(v, np.asarray(p.banned_token_ids, dtype=np.int64))
    if len(p.allowed_token_ids) > 0:
        forbidden |= ~np.isin(v, np.asarray(p.allowed_token_ids, dtype=np.int64))
    if nout < p.min_tokens:
        stop = set(p.stop_token_ids) | (set() if p.ignore_eos or eos is None else {eos})
        forbidden |= np.isin(v, np.asarray(sorted(stop), dtype=np.int64))
    for t, a in p.logit_bias.items():
        if t < V:
            x[t] += float(np.float32(a))
    x[:V][forbidden] = -np.inf
    return x
