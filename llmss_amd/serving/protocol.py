"""Wire formats (API-compatible with the reference PoC).

HTTP/Redis request JSON = ``{"prompt", "max_new_tokens", "is_greedy", "temperature", "top_p",
"top_k"}`` (producer_server.py:9-15), optionally ``"request_id"``; response JSON =
``{"prompt", "continuation"}`` written with ``ensure_ascii=False`` (consumer_server.py:170-173),
plus ``"request_id"`` and metrics when the request carried an id. Unknown keys are ignored, so a
reference producer/consumer interoperates with ours.
"""
from __future__ import annotations

import json
import uuid
from typing import Any, Dict, List, Optional

from pydantic import BaseModel, Field

from ..engine.sampling import SamplingParams


class Request(BaseModel):
    prompt: str
    max_new_tokens: int = 20
    is_greedy: bool = False
    temperature: float = 1.0
    top_p: float = 0.95
    top_k: int = 50
    request_id: Optional[str] = None
    seed: Optional[int] = None
    # extensions (absent from reference requests; a reference consumer ignores them)
    ignore_eos: bool = False
    stream: bool = False  # reply per engine step on squeue:<request_id>, then a final "finished" message
    prompt_token_ids: Optional[List[int]] = None  # pre-tokenized prompt (prompt text ignored)
    deadline_s: Optional[float] = None  # seconds the caller waits for the reply: the consumer stops generating then
    # log-probabilities of the raw model distribution: None none, 0 each generated token's, n also the n most likely
    # tokens per position (SamplingParams.logprobs; the serving engine needs --max-logprobs >= n)
    logprobs: Optional[int] = None
    # repetition control (SamplingParams; the serving engine needs --penalties, else the reply is an error)
    repetition_penalty: float = 1.0
    presence_penalty: float = 0.0
    frequency_penalty: float = 0.0
    # token constraints (SamplingParams; the serving engine needs --constraints, else the reply is an error).
    # logit_bias maps token ids to biases in [-100, 100]; JSON object keys are strings, read back as ints here
    logit_bias: Dict[int, float] = Field(default_factory=dict)
    banned_token_ids: List[int] = Field(default_factory=list)
    allowed_token_ids: List[int] = Field(default_factory=list)
    min_tokens: int = 0
    # min-p in [0, 1], 0 = off (SamplingParams; the serving engine needs --min-p, else the reply is an error)
    min_p: float = 0.0


class Response(BaseModel):
    prompt: str
    continuation: str
    request_id: Optional[str] = None
    output_tokens: Optional[int] = None
    ttft_s: Optional[float] = None
    e2e_s: Optional[float] = None
    finish_reason: Optional[str] = None
    # requests with logprobs only (final reply; the broker reply omits them otherwise, like every None): one entry
    # per generated token, the alternatives as [token id, log-probability] pairs, logit descending and ties by
    # ascending id
    token_logprobs: Optional[List[float]] = None
    top_logprobs: Optional[List[List[List[float]]]] = None


def new_request_id() -> str:
    return uuid.uuid4().hex


def parse_request(msg: str) -> Request:
    d = json.loads(msg)
    known = {k: d[k] for k in Request.model_fields if k in d}
    return Request(**known)


def to_sampling(req: Request) -> SamplingParams:
    return SamplingParams(max_new_tokens=req.max_new_tokens, is_greedy=req.is_greedy, temperature=req.temperature,
                          top_p=req.top_p, top_k=req.top_k, seed=req.seed, ignore_eos=req.ignore_eos,
                          logprobs=req.logprobs, repetition_penalty=req.repetition_penalty,
                          presence_penalty=req.presence_penalty, frequency_penalty=req.frequency_penalty,
                          logit_bias=dict(req.logit_bias), banned_token_ids=list(req.banned_token_ids),
                          allowed_token_ids=list(req.allowed_token_ids), min_tokens=req.min_tokens,
                          min_p=req.min_p).validate()


def dump_response(resp: Dict[str, Any]) -> str:
    return json.dumps({k: v for k, v in resp.items() if v is not None}, ensure_ascii=False)
