"""An fp64 oracle of per-token log-probabilities and the inputs the log-probability tests share
(tests/test_logprob_cases_cpu.py checks the CPU definition of ops/reference.py against it, tests/test_logprobs_gpu.py
the HIP kernels of csrc/logprobs.hip).

The oracle is numpy float64: ``x - logsumexp(x)`` over the first V columns of a row, and the top list by
``np.lexsort((ids, -x))`` - raw logit descending, ties by ascending token id. It shares no code with
ops/reference.py.

Value bound
-----------
For a row of V finite logits and a token whose logit lies d = max - x[token] below the row maximum:

    tol(V, d) = 1e-6 + (ceil(V / 256) + 16) * 2^-24 + 4 * 2^-24 * (d + ln V + 1)

* 1e-6: the relative error of the fp32 exponential in the mass sum exp(x - max) (the figure sampler_cases.py uses);
  the logarithm turns a relative error of the sum into an absolute one of the result.
* (ceil(V / 256) + 16) * 2^-24: an fp32 sum whose longest chain of additions is a per-thread serial run of at most
  ceil(V / 256) terms plus a reduction tree of at most 16 levels; each addition rounds by at most 2^-24 of a partial
  sum that is at most the total. The kernel's longest chain is ceil(V / 2048) + 11 (csrc/logprobs.hip: an 8-element
  tree per 16-B chunk, 256 threads serial over their chunks, a 6-level shuffle tree, 4 wave partials as a 2-level
  tree), and ceil(V / 256) on rows it reads element by element - inside this shape either way.
* 4 * 2^-24 * (d + ln V + 1): the final subtraction and logarithm, a few ulps of numbers of magnitude d + ln V.

Top-list ids are compared exactly on every row: selection compares stored values, there is no undecidable class.
"""
import math
from dataclasses import dataclass, field
from functools import lru_cache

import numpy as np
import torch

MAX_N = 20
N_VALUES = (0, 1, 5, 20)
PAD = 1e30  # fills the head's padding columns [V, ld): must never reach the maximum, the sum or the top list


def tol(V, d):
    d = np.asarray(d, dtype=np.float64)
    return 1e-6 + (math.ceil(V / 256) + 16) * 2.0 ** -24 + 4 * 2.0 ** -24 * (d + math.log(V) + 1)


@dataclass
class Case:
    name: str
    V: int
    ld: int
    logits: torch.Tensor  # [B, ld], bf16 or fp32, CPU
    tokens: torch.Tensor  # [B] int64
    lsm: np.ndarray = field(repr=False, default=None)  # [B, V] fp64 oracle log-softmax
    order: np.ndarray = field(repr=False, default=None)  # [B, min(MAX_N, V)] oracle top ids
    dist: np.ndarray = field(repr=False, default=None)  # [B, V] max - x

    @property
    def B(self):
        return self.logits.shape[0]


def oracle(x: np.ndarray):
    """(log-softmax [B, V] fp64, top ids [B, min(MAX_N, V)], max - x [B, V]) of fp64 logits x [B, V]."""
    x = np.asarray(x, dtype=np.float64)
    m = x.max(axis=1, keepdims=True)
    lse = m + np.log(np.exp(x - m).sum(axis=1, keepdims=True))
    ids = np.arange(x.shape[1])
    order = np.stack([np.lexsort((ids, -row))[:MAX_N] for row in x])
    return x - lse, order, m - x


def _finish(name, V, ld, x, tokens, dtype):
    lg = torch.full((x.shape[0], ld), PAD, dtype=torch.float32)
    lg[:, :V] = x
    lg = lg.to(dtype)
    c = Case(name, V, ld, lg, tokens.to(torch.int64))
    c.lsm, c.order, c.dist = oracle(lg[:, :V].double().numpy())
    return c


def _random(name, B, V, ld, dtype, scale, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, V, generator=g) * scale
    tokens = torch.randint(0, V, (B,), generator=g)
    tokens[0] = V - 1  # the last vocabulary column, next to the padding
    return _finish(name, V, ld, x, tokens, dtype)


def _special(name, V, ld, dtype, seed):
    """Row 0: all equal. Row 1: two values, 3 high, every other column tied at the N-th place. Row 2: random with 3
    high values and min(300, V // 3) columns tied at one value above the rest (hundreds of ties at the N-th place
    among few survivors). Row 3: one dominant token, the chosen token about 60 below it. Row 4: the ties of row 2 at
    the END of the row (ascending-id order decides, late). Row 5: the last min(2500, V // 2) columns tied below 2
    high values: more ties than the kernel ranks in LDS, the first of them late in the row."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(6, V, generator=g)
    tokens = torch.randint(0, V, (6,), generator=g)
    x[0] = 1.5
    x[1] = -2.0
    x[1, torch.randperm(V, generator=g)[:3]] = 3.0
    nt = min(300, V // 3)
    for r, cols in ((2, torch.randperm(V, generator=g)[:nt + 3]), (4, torch.arange(V - nt - 3, V))):
        x[r] = x[r].clamp(max=4.0)
        x[r, cols[3:]] = 6.0
        x[r, cols[:3]] = torch.tensor([9.0, 8.0, 9.0])
    x[5] = x[5].clamp(max=4.0)
    x[5, V - min(2500, V // 2):] = 6.0
    x[5, :2] = 9.0
    x[3] = torch.randn(V, generator=g) * 0.5 - 60.0
    x[3, V // 2] = 0.0
    tokens[3] = V // 2 + 1
    return _finish(name, V, ld, x, tokens, dtype)


bf16, f32 = torch.bfloat16, torch.float32


@lru_cache(maxsize=None)
def cases():
    """Every case, built once per process: the smallest shapes at which the kernel takes each of its paths."""
    return {c.name: c for c in (
        _random("v13-f32-unaligned", 3, 13, 13, f32, 1.0, 1),
        _random("v13-bf16-unaligned", 3, 13, 13, bf16, 12.0, 2),
        _random("v101-pad112-bf16", 3, 101, 112, bf16, 1.0, 3),
        _random("v101-pad112-f32", 1, 101, 112, f32, 12.0, 4),
        _random("v32000-bf16-b64", 64, 32000, 32000, bf16, 1.0, 5),
        _random("v32000-bf16-s12", 3, 32000, 32000, bf16, 12.0, 6),
        _random("v32000-f32", 1, 32000, 32000, f32, 12.0, 7),
        _random("v50257-pad50304-bf16", 3, 50257, 50304, bf16, 12.0, 8),
        _random("v50257-pad50304-f32", 1, 50257, 50304, f32, 1.0, 9),
        _random("v128256-bf16", 1, 128256, 128256, bf16, 1.0, 10),
        _random("v128256-bf16-s12", 3, 128256, 128256, bf16, 12.0, 11),
        _special("special-v101-pad112-bf16", 101, 112, bf16, 12),
        _special("special-v13-f32", 13, 13, f32, 13),
        _special("special-v32000-bf16", 32000, 32000, bf16, 14),
        _special("special-v50257-pad50304-f32", 50257, 50304, f32, 15),
    )}


CASE_NAMES = ("v13-f32-unaligned", "v13-bf16-unaligned", "v101-pad112-bf16", "v101-pad112-f32", "v32000-bf16-b64",
              "v32000-bf16-s12", "v32000-f32", "v50257-pad50304-bf16", "v50257-pad50304-f32", "v128256-bf16",
              "v128256-bf16-s12", "special-v101-pad112-bf16", "special-v13-f32", "special-v32000-bf16",
              "special-v50257-pad50304-f32")
SHARDABLE = tuple(n for n in CASE_NAMES if "v13" not in n)  # at least one column per shard at 8 shards


def check(case: Case, N: int, lp, top_lp, top_ids, what=""):
    """Assert (lp [B], top_lp [B, N], top_ids [B, N]) against the oracle: values within tol, ids exactly, -inf / -1
    past the vocabulary. Returns the largest error as a fraction of its bound."""
    B, V = case.B, case.V
    lp = lp.detach().cpu().double().numpy()
    top_lp = top_lp.detach().cpu().double().numpy()
    top_ids = top_ids.detach().cpu().numpy()
    assert lp.shape == (B,) and top_lp.shape == (B, N) and top_ids.shape == (B, N), (what, lp.shape, top_lp.shape)
    rows = np.arange(B)
    tok = case.tokens.numpy()
    err = np.abs(lp - case.lsm[rows, tok]) / tol(V, case.dist[rows, tok])
    worst = float(err.max())
    assert np.isfinite(lp).all() and worst <= 1.0, \
        f"{what} {case.name}: token log-probability off by {worst:.3g} x tol at row {int(err.argmax())}"
    k = min(N, V)
    want = case.order[:, :k]
    bad = np.flatnonzero((top_ids[:, :k] != want).any(axis=1))
    assert bad.size == 0, f"{what} {case.name} N={N}: top ids differ on rows {bad[:8].tolist()}: got " \
                          f"{top_ids[bad[0], :k].tolist()}, want {want[bad[0]].tolist()}"
    assert (top_ids[:, k:] == -1).all() and np.isneginf(top_lp[:, k:]).all(), f"{what} {case.name}: entries past V"
    if k:
        r2 = rows[:, None]
        e2 = np.abs(top_lp[:, :k] - case.lsm[r2, want]) / tol(V, case.dist[r2, want])
        assert np.isfinite(top_lp[:, :k]).all() and e2.max() <= 1.0, \
            f"{what} {case.name} N={N}: top value off by {e2.max():.3g} x tol"
        worst = max(worst, float(e2.max()))
    return worst
