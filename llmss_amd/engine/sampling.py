"""Per-request sampling parameters (mirrors the reference CLI/HTTP fields, generate.py:21-40,
producer_server.py:9-15) plus the deterministic per-step seed used identically on every rank.

Filter order. The reference builds HF warpers in the order TopP -> TopK -> Temperature
(generate.py:111-119) but then inverts its own test (``if not list_of_warpers``), so the warpers
are never applied: its effective sampler is plain multinomial sampling from softmax(logits) at
temperature 1 whatever the flags say. Here the flags are honoured in the order HF ``generate()``
applies them - temperature, then top-k, then top-p on the temperature-scaled distribution
(csrc/sampling.hip, ops/reference.sample) - because that is what a caller of these flags expects
and it keeps top-p's nucleus consistent with the distribution actually sampled. The reference's
*stated* order would compute the nucleus at temperature 1 and rescale afterwards; the two agree
whenever temperature == 1 (the reference's default) or when top-p == 1. The reference's *effective*
behaviour is ``temperature=1.0, top_k=0, top_p=1.0`` (unfiltered multinomial sampling), which these
parameters reproduce exactly.
"""
from __future__ import annotations

import itertools
import math
import numbers
import os
from dataclasses import dataclass, field
from typing import Dict, List, Optional, Tuple

import numpy as np

_seed_counter = itertools.count(int.from_bytes(os.urandom(4), "little"))
MASK64 = (1 << 64) - 1
MAX_TOP_LOGPROBS = 20  # most alternatives per generated position a request may ask for (csrc/logprobs.hip)
MAX_TOKEN_EDITS = 512  # most listed tokens of a request's early or late constraint list (csrc/constraints.hip)


def _is_number(v) -> bool:
    return isinstance(v, numbers.Real) and not isinstance(v, bool)


def _is_int(v) -> bool:
    return isinstance(v, numbers.Integral) and not isinstance(v, bool)


@dataclass
class SamplingParams:
    max_new_tokens: int = 20
    is_greedy: bool = False
    temperature: float = 1.0
    top_p: float = 0.95
    top_k: int = 50
    seed: Optional[int] = None
    stop_token_ids: List[int] = field(default_factory=list)
    ignore_eos: bool = False
    # log-probabilities of the raw model distribution log_softmax(logits[:vocab]) - temperature, top-k and top-p are
    # not applied. None: none returned; 0: each generated token's; n in 1..MAX_TOP_LOGPROBS: additionally the n most
    # likely tokens at each generated position (logit descending, ties by ascending id). Needs an engine launched
    # with max_logprobs >= n.
    logprobs: Optional[int] = None
    # repetition control, applied to the logits before temperature, top-k and top-p (csrc/penalties.hip). A token seen
    # in the prompt or the output has its logit x replaced by x / repetition_penalty (x > 0) or x * repetition_penalty
    # (Hugging Face); a token that occurs c > 0 times in the output then loses frequency_penalty * c +
    # presence_penalty (OpenAI). Anything but the defaults needs an engine launched with penalties=True.
    repetition_penalty: float = 1.0
    presence_penalty: float = 0.0
    frequency_penalty: float = 0.0
    # token constraints, a sparse edit of the logits row after the penalties and before temperature, top-k and top-p
    # (csrc/constraints.hip; resolve_token_edits below is the definition). logit_bias adds a value in [-100, 100] to a
    # token's logit; a banned token's logit becomes -inf; a non-empty allowed_token_ids makes every other token's
    # -inf; while a sequence has generated fewer than min_tokens tokens, EOS (unless ignore_eos) and the
    # stop_token_ids are -inf. Anything but the defaults needs an engine launched with constraints=True.
    logit_bias: Dict[int, float] = field(default_factory=dict)
    banned_token_ids: List[int] = field(default_factory=list)
    allowed_token_ids: List[int] = field(default_factory=list)
    min_tokens: int = 0
    # min-p: after temperature, top-k and top-p, keep only the tokens whose probability is at least min_p times the most
    # likely token's (csrc/sampling.hip MINP variants; ops/reference.py _select is the definition). 0 = off; 1 keeps
    # exactly the most likely token(s). Greedy requests ignore it. Anything but 0 needs an engine launched with
    # min_p=True.
    min_p: float = 0.0

    @property
    def has_min_p(self) -> bool:
        return not (_is_number(self.min_p) and self.min_p == 0.0)

    @property
    def has_penalties(self) -> bool:
        return not (self.repetition_penalty == 1.0 and self.presence_penalty == 0.0 and self.frequency_penalty == 0.0)

    @property
    def has_constraints(self) -> bool:
        return bool(self.logit_bias or self.banned_token_ids or self.allowed_token_ids or self.min_tokens != 0)

    def validate(self) -> "SamplingParams":
        """Reference validation (generate.py:37-40)."""
        if not self.max_new_tokens > 0:
            raise ValueError("Value of max_new_tokens should be over than 0.")
        if not (0.0 < self.temperature <= 1.0):
            raise ValueError("Value of temperature is not valid.")
        if not (0.0 < self.top_p <= 1.0):
            raise ValueError("Value of top_p is not valid.")
        if not self.top_k >= 0:
            raise ValueError("Value of top_k is not valid.")
        lp = self.logprobs
        if lp is not None and not (isinstance(lp, int) and not isinstance(lp, bool) and 0 <= lp <= MAX_TOP_LOGPROBS):
            raise ValueError(f"Value of logprobs should be None or an integer in 0..{MAX_TOP_LOGPROBS}.")
        r = self.repetition_penalty
        if not (_is_number(r) and math.isfinite(r) and r > 0):
            raise ValueError("Value of repetition_penalty should be a finite number above 0.")
        for name in ("presence_penalty", "frequency_penalty"):
            v = getattr(self, name)
            if not (_is_number(v) and math.isfinite(v) and -2.0 <= v <= 2.0):
                raise ValueError(f"Value of {name} should be a finite number in [-2, 2].")
        if not isinstance(self.logit_bias, dict):
            raise ValueError("Value of logit_bias should be a dict of token id -> bias.")
        for name, ids in (("logit_bias", list(self.logit_bias)), ("banned_token_ids", self.banned_token_ids),
                          ("allowed_token_ids", self.allowed_token_ids)):
            if not isinstance(ids, (list, tuple)) or not all(_is_int(t) and t >= 0 for t in ids):
                raise ValueError(f"Token ids of {name} should be integers >= 0.")
            if len(set(ids)) != len(ids):
                raise ValueError(f"Token ids of {name} should be distinct.")
        for v in self.logit_bias.values():
            if not (_is_number(v) and math.isfinite(v) and -100.0 <= v <= 100.0):
                raise ValueError("Values of logit_bias should be finite numbers in [-100, 100].")
        if not (_is_int(self.min_tokens) and 0 <= self.min_tokens <= self.max_new_tokens):
            raise ValueError("Value of min_tokens should be an integer in 0..max_new_tokens.")
        if not (_is_number(self.min_p) and math.isfinite(self.min_p) and 0.0 <= self.min_p <= 1.0):
            raise ValueError("Value of min_p should be a finite number in [0, 1].")
        return self

    def resolved_seed(self) -> int:
        if self.seed is None:
            self.seed = next(_seed_counter)
        return self.seed & MASK64

    # kernel-facing values
    @property
    def k_temperature(self) -> float:
        return 0.0 if self.is_greedy else float(self.temperature)

    @property
    def k_top_k(self) -> int:
        return 1 if self.is_greedy else int(self.top_k)

    @property
    def k_top_p(self) -> float:
        return float(self.top_p)

    @property
    def k_ln_min_p(self) -> float:
        """fp32 ln(min_p), computed in fp64 and rounded once; -inf (no floor) for min_p == 0 or a greedy request. The
        kernels add it to the row's maximum scaled logit and never take a logarithm themselves."""
        if self.is_greedy or not self.min_p > 0.0:
            return float("-inf")
        return float(np.float32(math.log(float(self.min_p))))


def resolve_token_edits(params: SamplingParams, eos: Optional[int], vocab: int
                        ) -> Tuple[List[Tuple[int, float]], List[Tuple[int, float]], bool]:
    """A request's token constraints as (early list, late list, fill): two lists of distinct (token, value) pairs in
    ascending token order, value -inf (forbidden) or a finite bias added to the logit; ``fill``: every token that is
    not listed is forbidden too. The late list is in force once the sequence has generated min_tokens tokens, the
    early one before that (empty and unused when min_tokens == 0).

    late, with a non-empty allowed_token_ids: fill, and every allowed token that is not banned with its bias (0.0
    without one); otherwise no fill, and every token of logit_bias or banned_token_ids: -inf if banned, else its bias.
    early: the late list with the stop set S = {eos unless ignore_eos or eos is None} | stop_token_ids forced out -
    removed from a filled list, added or overwritten with -inf otherwise.

    ValueError: a token id at or past ``vocab``, a filled list that leaves no token, more than MAX_TOKEN_EDITS entries."""
    bias, banned, allowed = params.logit_bias, set(params.banned_token_ids), params.allowed_token_ids
    for name, ids in (("logit_bias", bias), ("banned_token_ids", banned), ("allowed_token_ids", allowed)):
        bad = [t for t in ids if not 0 <= t < vocab]
        if bad:
            raise ValueError(f"{name}: token ids {sorted(bad)[:8]} are outside the vocabulary of {vocab}")
    fill = len(allowed) > 0
    if fill:
        late = {int(v): float(bias.get(v, 0.0)) for v in allowed if v not in banned}
    else:
        late = {int(v): float("-inf") if v in banned else float(bias[v]) for v in set(bias) | banned}
    early = {}
    if params.min_tokens > 0:
        stop = {int(t) for t in params.stop_token_ids}
        if eos is not None and not params.ignore_eos:
            stop.add(int(eos))
        if fill:
            early = {v: a for v, a in late.items() if v not in stop}
        else:
            early = {**late, **{t: float("-inf") for t in stop if 0 <= t < vocab}}
    for name, lst, used in (("early", early, params.min_tokens > 0), ("late", late, True)):
        if used and fill and not lst:
            raise ValueError(f"the token constraints leave no token to sample "
                             f"{'before min_tokens' if name == 'early' else 'at all'}")
        if len(lst) > MAX_TOKEN_EDITS:
            raise ValueError(f"the token constraints list {len(lst)} tokens ({name}), more than MAX_TOKEN_EDITS = "
                             f"{MAX_TOKEN_EDITS}")
    return sorted(early.items()), sorted(late.items()), fill


def step_seed(seed: int, step: int) -> int:
    """splitmix64(seed + step): a fresh 64-bit Philox key per (request, generated position)."""
    z = (seed + 0x9E3779B97F4A7C15 * (step + 1)) & MASK64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & MASK64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & MASK64
    z = z ^ (z >> 31)
    return z - (1 << 64) if z >= (1 << 63) else z  # as signed int64


_M = [np.uint64(v) for v in (0x9E3779B97F4A7C15, 0xBF58476D1CE4E5B9, 0x94D049BB133111EB, 1, 30, 27, 31)]


def step_seeds(seeds: np.ndarray, steps: np.ndarray) -> np.ndarray:
    """Vectorised :func:`step_seed` (uint64 seeds, int steps) -> int64 Philox keys, bit-identical."""
    golden, m1, m2, one, s30, s27, s31 = _M
    with np.errstate(over="ignore"):
        z = seeds.astype(np.uint64) + golden * (steps.astype(np.uint64) + one)
        z = (z ^ (z >> s30)) * m1
        z = (z ^ (z >> s27)) * m2
        z = z ^ (z >> s31)
    return z.view(np.int64)
