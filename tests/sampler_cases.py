"""An fp64 oracle of the token sampler and the inputs the sampler tests share (tests/test_sampler_oracle_cpu.py
checks the oracle and the CPU definition ops/reference.py against each other; tests/test_sampler_oracle_gpu.py
runs the same cases through the HIP kernels of csrc/sampling.hip).

The oracle is an independent definition of temperature -> top-k -> top-p -> Gumbel-max: its own Philox, its own
integer definition of the uniform mapping, fp64 masses and fp64 logarithms. It shares no selection code with
ops/reference.py. Per row it returns the token AND whether that token is DECIDABLE: whether every evaluation of
the same definition within the stated rounding bounds draws the same token. A test compares tokens on decidable
rows only, and asserts that at most MAX_UNDECIDABLE of the rows of a case are not.

Rounding bounds
---------------
top-p, v3 and candidate kernels (eps_v3).  The kernels sum each kept token's mass exp(x - max) as a truncated
    2^-32 fixed-point integer of an fp32 __expf. Against the exact masses, whose sum z is >= 1 (the maximum
    itself has mass 1 = 2^32 units): truncation loses at most one unit per token, n * 2^-32 relative to z; the fp32
    difference x - max, the fp32 product with log2(e) inside __expf and the hardware exp2 are each good to about an
    ulp of a number of magnitude <= 16 on the tokens that carry mass, about 1e-6 relative in the mass. That bounds
    the error of one cumulative sum by (n * 2^-32 + 1e-6) z. The comparison `cum >= p * z` has such an error on
    either side (cum and z), hence the factor 2:  eps = 2 (n 2^-32 + 1e-6).
top-p, fallback sample_kernel (eps_fallback).  This kernel adds fp32 masses with LDS float atomics in no fixed
    order. A sum of n fp32 terms accumulated in any order is within n * 2^-24 (n - 1 roundings of half an ulp,
    each of a partial sum <= z, 2^-24 z each, to first order) of the exact sum:  eps = n 2^-24. For every n of a
    few dozen or more this also covers the 1e-6 of the exponential above; it is far wider than eps_v3 at
    vocabulary size (3e-3 at n = 50000) because fp32 accumulation is that much worse than 2^-32 fixed point.
    n is the number of top-k survivors in both formulas.
Gumbel noise (DELTA).  The kernels and the CPU definition take both logarithms in fp32, the oracle in fp64 from
    the same fp32 u. G_FP32_MAX_ERR is the largest |g_fp32 - g_fp64| over ALL 2^24 values of u with numpy's
    fp32 log (measured on the CPU against the fp64 value, never against a kernel). DELTA is 1000 times that: the
    margin for a fast device log that is a few ulps worse, amplified by the second log. A row is decidable only
    if the winner leads the runner-up by at least DELTA.
"""
from dataclasses import dataclass
from functools import lru_cache
from typing import Optional

import numpy as np
import torch

G_FP32_MAX_ERR = 5.944e-7  # max |g_fp32 - g_fp64| over all 2^24 u (numpy fp32 logs); at r >> 8 = 16775735
DELTA = 1000 * G_FP32_MAX_ERR  # 5.944e-4
MAX_UNDECIDABLE = 0.02
B_ROWS = 48

_M32 = np.uint64(0xFFFFFFFF)


# ------------------------------------------------------------------------------------------ noise
def philox(idx, seed) -> np.ndarray:
    """First output word of Philox-4x32-10 for counter (idx, 0, 0, 0) and key (seed low word, seed high word).
    ``idx`` and ``seed`` broadcast against each other; seeds are taken modulo 2^64 (int64 views allowed)."""
    c0 = np.asarray(idx).astype(np.uint64) & _M32
    seed = np.asarray(seed)
    seed = seed.astype(np.int64).view(np.uint64) if seed.dtype.kind == "i" else seed.astype(np.uint64)
    c0, seed = np.broadcast_arrays(c0, seed)
    k0, k1 = seed & _M32, seed >> np.uint64(32)
    c1 = np.zeros_like(c0)
    c2 = np.zeros_like(c0)
    c3 = np.zeros_like(c0)
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c0, np.uint64(0xCD9E8D57) * c2
        c0, c1, c2, c3 = (p1 >> np.uint64(32)) ^ c1 ^ k0, p1 & _M32, (p0 >> np.uint64(32)) ^ c3 ^ k1, p0 & _M32
        k0, k1 = (k0 + np.uint64(0x9E3779B9)) & _M32, (k1 + np.uint64(0xBB67AE85)) & _M32
    return c0


def uniform(m) -> np.ndarray:
    """The sampler's u for m = r >> 8, as an exact fp64 number, defined with integers: fp32 (m + 0.5) * 2^-24 is
    (2m + 1) / 2^25 while that is representable (m < 2^23) and m + 0.5 rounded to even above; the result is clamped
    to the largest fp32 below 1, (2^24 - 1) / 2^24."""
    m = np.asarray(m).astype(np.int64)
    num = np.where(m < (1 << 23), 2 * m + 1, 2 * (m + (m & 1)))  # numerator over 2^25
    return np.minimum(num, 2 * ((1 << 24) - 1)).astype(np.float64) / float(1 << 25)


def gumbel(idx, seed) -> np.ndarray:
    """fp64 Gumbel noise of token ``idx`` under row seed ``seed``."""
    return -np.log(-np.log(uniform(philox(idx, seed) >> np.uint64(8))))


# ------------------------------------------------------------------------------------------ selection
def eps_v3(n: int) -> float:
    return 2.0 * (n * 2.0 ** -32 + 1e-6)


def eps_fallback(n: int) -> float:
    return n * 2.0 ** -24


EPS = {"v3": eps_v3, "fallback": eps_fallback}


def is_greedy(t: float, k: int) -> bool:
    return not t > 0 or k == 1


def scaled(row: np.ndarray, t: float, k: int) -> np.ndarray:
    """fp32 scaled logits as the kernels form them: logit * fp32(1 / temperature), one fp32 rounding each."""
    sc = np.float32(1.0) if is_greedy(t, k) else np.float32(1.0) / np.float32(t)
    return row.astype(np.float32) * sc


def thresholds(x: np.ndarray, k: int, p: float, V: int, eps_fn):
    """(thr_k, thr_strict, thr_loose) of the finite fp64 values ``x``: the top-k boundary value (ties kept), and the
    top-p boundary values when the cumulative mass is read eps too low / eps too high. thr_strict >= thr_loose;
    every admissible kernel keeps exactly the tokens >= some thr with thr_loose <= thr <= thr_strict (and
    >= thr_k)."""
    thr_k = -np.inf
    if 0 < k < V and k <= x.size:
        thr_k = np.partition(x, x.size - k)[x.size - k]
    if not p < 1.0:
        return thr_k, thr_k, thr_k
    xs = np.sort(x[x >= thr_k])[::-1]  # the boundary is a value: the order inside a tie does not matter
    cum = np.cumsum(np.exp(xs - xs[0]))
    z = cum[-1]
    target, e = float(p) * z, eps_fn(xs.size) * z
    last = xs.size - 1
    strict = xs[min(int(np.searchsorted(cum, target - e, side="left")), last)]
    loose = xs[min(int(np.searchsorted(cum, target + e, side="left")), last)]
    return thr_k, max(thr_k, strict), max(thr_k, loose)


def oracle_row(x32: np.ndarray, t: float, k: int, p: float, seed: int, eps_fn):
    """One row of fp32 scaled logits over the vocabulary (columns past it already cut). Returns (token,
    decidable, lead): lead = fp64 gap between the winner and the runner-up (inf where there is none)."""
    V = x32.size
    idx = np.flatnonzero(x32 > -np.inf)
    if idx.size == 0:
        return 0, True, np.inf
    x = x32[idx].astype(np.float64)
    if is_greedy(t, k):
        return int(idx[np.argmax(x)]), True, np.inf  # argmax: the first (lowest index) of the maxima
    thr_k, thr_strict, thr_loose = thresholds(x, k, p, V, eps_fn)
    keep = x >= thr_loose
    x, idx = x[keep], idx[keep]
    v = x + gumbel(idx, seed)
    w = int(np.argmax(v))
    lead = np.inf if v.size == 1 else float(v[w] - np.max(np.delete(v, w)))
    return int(idx[w]), bool(x[w] >= thr_strict and lead >= DELTA), lead


# ------------------------------------------------------------------------------------------ cases
@dataclass(frozen=True)
class Case:
    name: str
    V: int
    width: int        # row width (stride); columns [V, width) are padding that must be masked
    dtype: str        # "bf16" | "fp32"
    kernel: str       # the launch_sample dispatch this shape and dtype reach (see dispatch())
    eps: str          # "v3" | "fallback"
    seed: int
    cand: bool = False  # candidate path: only greedy rows and rows with 1 <= top_k <= 64
    shards: int = 0     # candidate path: column shards of one launch, or TP ranks


def dispatch(V: int, width: int, dtype: str) -> str:
    """Which kernel launch_sample (csrc/sampling.hip) picks for a contiguous, 16-byte aligned [B, width] tensor."""
    chunks = (V + 7) // 8
    if dtype == "bf16" and width % 8 == 0 and chunks <= 7168:  # SV3_LROW_CHUNKS
        return "v3<2,false>" if chunks <= 2048 else "v3<4,false>" if chunks <= 4096 else "v3<8,true>"
    return "sample_kernel<float>" if dtype == "fp32" else "sample_kernel<bf16>"


FULL_ROW_CASES = [
    Case("v3c2-V1000", 1000, 1000, "bf16", "v3<2,false>", "v3", 101),
    Case("v3c2-V16384", 16384, 16384, "bf16", "v3<2,false>", "v3", 102),
    Case("v3c2-V8200-in-8208", 8200, 8208, "bf16", "v3<2,false>", "v3", 103),
    Case("v3c4-V32000", 32000, 32000, "bf16", "v3<4,false>", "v3", 104),
    Case("v3c4-V32768", 32768, 32768, "bf16", "v3<4,false>", "v3", 105),
    Case("v3c8lds-V50257-in-50304", 50257, 50304, "bf16", "v3<8,true>", "v3", 106),
    Case("v3c8lds-V57344", 57344, 57344, "bf16", "v3<8,true>", "v3", 107),
    Case("fallback-bf16-V50257-odd-stride", 50257, 50257, "bf16", "sample_kernel<bf16>", "fallback", 108),
    Case("fallback-bf16-V60000", 60000, 60000, "bf16", "sample_kernel<bf16>", "fallback", 109),
    Case("fallback-fp32-V1000", 1000, 1000, "fp32", "sample_kernel<float>", "fallback", 110),
    Case("fallback-fp32-V32000", 32000, 32000, "fp32", "sample_kernel<float>", "fallback", 111),
]
SHARD_CASES = [  # H.cand_topk(shards=s) + H.sample_cand on one GPU
    Case("cand-s8-V32000", 32000, 32000, "bf16", "cand", "v3", 201, cand=True, shards=8),
    Case("cand-s4-V50257-in-50304", 50257, 50304, "bf16", "cand", "v3", 202, cand=True, shards=4),
    Case("cand-s3-V1000-in-1008", 1000, 1008, "bf16", "cand", "v3", 203, cand=True, shards=3),
]
TP_CASES = [  # ops.sample_distributed over per-rank packs
    Case("cand-tp2-V32000", 32000, 32000, "bf16", "cand", "v3", 301, cand=True, shards=2),
    Case("cand-tp8-V50257-in-50304", 50257, 50304, "bf16", "cand", "v3", 302, cand=True, shards=8),
]
ALL_CASES = FULL_ROW_CASES + SHARD_CASES + TP_CASES

TEMPS = [0.0, 0.7, 1.0, 1.3]
TOP_KS = [0, 1, 5, 40, 64, 2000]
TOP_PS = [1.0, 0.95, 0.9, 0.5]
PAD_LOGIT = 7.0  # padding columns hold +7: they would win if a kernel did not mask them


@dataclass
class Inputs:
    logits: torch.Tensor  # [B, width] bf16 or fp32, CPU
    temp: np.ndarray      # [B] float32
    topk: np.ndarray      # [B] int32
    topp: np.ndarray      # [B] float32
    seeds: np.ndarray     # [B] int64

    def params(self, device):
        return tuple(torch.from_numpy(a).to(device) for a in (self.temp, self.topk, self.topp, self.seeds))


@lru_cache(maxsize=None)
def inputs(case: Case) -> Inputs:
    """B_ROWS rows of randn * 2.5 rounded to bf16 (real ties), three -inf entries per row, the last row all -inf;
    fp32 cases keep the even rows at full fp32 precision. Per-row temperature / top-k / top-p from the lists above,
    seeds over the whole signed 64-bit range."""
    B = B_ROWS
    g = torch.Generator().manual_seed(case.seed)
    rng = np.random.default_rng(case.seed)
    x = torch.randn(B, case.V, generator=g) * 2.5
    xb = x.to(torch.bfloat16)
    if case.dtype == "fp32":
        x[1::2] = xb[1::2].float()
    else:
        x = xb
    for b in range(B):
        x[b, torch.from_numpy(rng.choice(case.V, 3, replace=False))] = float("-inf")
    x[B - 1] = float("-inf")
    logits = torch.full((B, case.width), PAD_LOGIT, dtype=x.dtype)
    logits[:, :case.V] = x
    temp = rng.choice(TEMPS, B).astype(np.float32)
    topk = rng.choice([k for k in TOP_KS if 1 <= k <= 64] if case.cand else TOP_KS, B).astype(np.int32)
    topp = rng.choice(TOP_PS, B).astype(np.float32)
    seeds = rng.integers(-2 ** 63, 2 ** 63, B, dtype=np.int64)
    seeds[0], seeds[1] = -1, -2 ** 63  # all key bits set; only the top key bit set
    return Inputs(logits, temp, topk, topp, seeds)


@lru_cache(maxsize=None)
def oracle(case: Case):
    """(tokens [B] int64, decidable [B] bool) of a case; computed once per process."""
    inp = inputs(case)
    rows = inp.logits[:, :case.V].float().numpy()
    toks, dec = [], []
    for b in range(rows.shape[0]):
        t, k, p = float(inp.temp[b]), int(inp.topk[b]), float(inp.topp[b])
        tok, ok, _ = oracle_row(scaled(rows[b], t, k), t, k, p, int(inp.seeds[b]), EPS[case.eps])
        toks.append(tok)
        dec.append(ok)
    return np.array(toks, dtype=np.int64), np.array(dec, dtype=bool)


def check_tokens(got, case: Case):
    """``got`` equals the oracle on every decidable row, and at most MAX_UNDECIDABLE of the rows are not."""
    want, dec = oracle(case)
    got = np.asarray(got, dtype=np.int64)
    assert 1.0 - dec.mean() <= MAX_UNDECIDABLE, f"{case.name}: {(~dec).sum()} of {dec.size} rows undecidable"
    bad = np.flatnonzero(dec & (got != want))
    inp = inputs(case)
    assert bad.size == 0, (case.name, [(int(b), int(got[b]), int(want[b]), float(inp.temp[b]), int(inp.topk[b]),
                                        float(inp.topp[b]), int(inp.seeds[b])) for b in bad[:8]])


# ------------------------------------------------------------------------------------------ u == 1 rows
U1_V = 32000
U1_PAIRS = [(247, 31399), (404, 28925), (554, 19468), (591, 21025)]  # (seed, token) with r >> 8 == 0xFFFFFF


def u1_rows(finite: Optional[int] = None) -> torch.Tensor:
    """One fp32 row per pair: token 0 at +5, the pair's token at -30, every other token at 0. ``finite`` = n keeps
    only n tokens finite (token 0, the pair's token and the lowest other indices), the rest -inf."""
    x = torch.zeros(len(U1_PAIRS), U1_V)
    for b, (_, tok) in enumerate(U1_PAIRS):
        if finite is not None:
            x[b, finite - 1:] = float("-inf")  # tokens 0 .. finite - 2 and the pair's token stay finite
        x[b, 0] = 5.0
        x[b, tok] = -30.0
    return x


@lru_cache(maxsize=None)
def u1_oracle(finite: Optional[int] = None, topk: int = 0):
    """(tokens, decidable, lead of the winner over the pair's token) of u1_rows at temperature 1, no top-p."""
    rows = u1_rows(finite).numpy()
    toks, dec, lead = [], [], []
    for b, (seed, tok) in enumerate(U1_PAIRS):
        t, ok, _ = oracle_row(rows[b], 1.0, topk, 1.0, seed, eps_v3)
        toks.append(t)
        dec.append(ok)
        lead.append(float(rows[b, t] + gumbel(t, seed) - (rows[b, tok] + gumbel(tok, seed))))
    return np.array(toks), np.array(dec), np.array(lead)


# ------------------------------------------------------------------------------------------ distribution
DIST_V = 64
DIST_N = 8192
DIST_PARAMS = [(0, 1.0, 1.0), (10, 1.0, 0.8), (0, 0.7, 1.0), (20, 0.9, 1.3)]  # (top-k, top-p, temperature)
DIST_FAMILIES = ["consecutive", "upper-word", "step-seeds"]


def dist_row() -> torch.Tensor:
    """+3 down to -4.875 in steps of 0.125: every value exact in bf16."""
    return (3.0 - 0.125 * torch.arange(DIST_V, dtype=torch.float32)).to(torch.bfloat16)


def dist_seeds(family: str) -> np.ndarray:
    i = np.arange(DIST_N, dtype=np.int64)
    if family == "consecutive":
        return i
    if family == "upper-word":
        return i << 32  # only the upper key word varies
    from llmss_amd.engine.sampling import step_seeds

    return step_seeds(np.full(DIST_N, 1234, dtype=np.uint64), i)


def chi2_bound(dof: int, q: float = 1e-6) -> float:
    """Chi-square quantile at 1 - q."""
    try:
        from scipy.stats import chi2

        return float(chi2.ppf(1.0 - q, dof))
    except ImportError:  # Wilson-Hilferty
        from statistics import NormalDist

        z = NormalDist().inv_cdf(1.0 - q)
        return dof * (1.0 - 2.0 / (9.0 * dof) + z * (2.0 / (9.0 * dof)) ** 0.5) ** 3


@lru_cache(maxsize=None)
def dist_oracle(k: int, p: float, t: float, family: str):
    """The DIST_N draws of dist_row under one parameter set and seed family: (tokens, decidable, kept token ids,
    their exact renormalised fp64 probabilities). The kept set itself must be beyond doubt."""
    x32 = scaled(dist_row().float().numpy(), t, k)
    x = x32.astype(np.float64)
    _, strict, loose = thresholds(x, k, float(np.float32(p)), DIST_V, eps_v3)  # p as the kernel's fp32 holds it
    assert strict == loose, "the distribution row must have an unambiguous kept set"
    kept = np.flatnonzero(x >= loose)
    pr = np.exp(x[kept] - x[kept].max())
    pr /= pr.sum()
    seeds = dist_seeds(family)
    v = x[kept][None, :] + gumbel(kept[None, :], seeds[:, None])
    order = np.sort(v, axis=1)
    dec = (order[:, -1] - order[:, -2]) >= DELTA
    return kept[np.argmax(v, axis=1)], dec, kept, pr


def chi2_stat(tokens, kept: np.ndarray, pr: np.ndarray) -> float:
    """Pearson's statistic of the token counts against the exact probabilities; a token outside the kept set makes
    it infinite."""
    counts = np.bincount(np.asarray(tokens, dtype=np.int64), minlength=DIST_V).astype(np.float64)
    if counts.sum() != counts[kept].sum():
        return float("inf")
    exp = pr * counts.sum()
    return float(((counts[kept] - exp) ** 2 / exp).sum())
