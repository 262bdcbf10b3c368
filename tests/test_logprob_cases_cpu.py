"""The CPU definition of per-token log-probabilities (ops/reference.py) against the fp64 oracle of
tests/logprob_cases.py; that the oracle's checks can fail; and that the vocab-parallel partial + combine
definitions equal the full-row one."""
import numpy as np
import pytest
import torch

import logprob_cases as L
from llmss_amd import ops
from llmss_amd.ops import reference as R


@pytest.mark.parametrize("name", L.CASE_NAMES)
def test_reference_meets_oracle(name):
    c = L.cases()[name]
    for N in L.N_VALUES:
        worst = L.check(c, N, *ops.token_logprobs(c.logits, c.V, c.tokens, N), what="reference")
        print(f"{name} N={N}: worst error {worst:.3f} x tol")


def test_tol_is_below_the_loss_tolerance():
    for V in (13, 101, 4096, 32000, 50257, 128256):
        assert L.tol(V, 0.0) < 1e-4


def test_all_equal_row_values():
    c = L.cases()["special-v32000-bf16"]
    lp, top, ids = ops.token_logprobs(c.logits[:1], c.V, c.tokens[:1], 20)
    assert ids[0].tolist() == list(range(20))
    assert np.abs(top[0].double().numpy() + np.log(c.V)).max() <= L.tol(c.V, 0.0)


# ------------------------------------------------------------------ the oracle can fail
def _with_pad(c, N):
    return R.token_logprobs(c.logits, c.ld, c.tokens, N)


def _with_temperature(c, N):
    return R.token_logprobs(c.logits.float() / 0.7, c.V, c.tokens, N)


def _ties_descending_id(c, N):
    lp, top, ids = R.token_logprobs(c.logits[:, :c.V].flip(1), c.V, c.V - 1 - c.tokens, N)
    return lp, top, torch.where(ids >= 0, c.V - 1 - ids, ids)


def _off_by_one(c, N):
    lp, top, ids = R.token_logprobs(c.logits, c.V, c.tokens, N + 1)
    return lp, top[:, 1:], ids[:, 1:]


@pytest.mark.parametrize("broken,name", [(_with_pad, "v101-pad112-bf16"), (_with_pad, "v50257-pad50304-bf16"),
                                         (_with_temperature, "v32000-bf16-s12"),
                                         (_ties_descending_id, "special-v32000-bf16"),
                                         (_off_by_one, "v32000-bf16-s12")])
def test_oracle_rejects_a_broken_definition(broken, name):
    c = L.cases()[name]
    with pytest.raises(AssertionError):
        L.check(c, 5, *broken(c, 5), what=broken.__name__)


# ------------------------------------------------------------------ vocab-parallel definitions
class _Gather:
    """A tensor-parallel group of one: the packs of `shards` column shards already sit side by side."""

    def all_gather_last_dim(self, t):
        return t


@pytest.mark.parametrize("shards", [2, 4, 8])
@pytest.mark.parametrize("name", L.SHARDABLE)
def test_partial_combine_equals_full_row(name, shards):
    c = L.cases()[name]
    local = c.logits[:, :c.V] if c.V % shards else c.logits  # a shard may also carry the padding columns
    for N in L.N_VALUES:
        got = ops.token_logprobs_distributed(local, _Gather(), 0, c.V, c.tokens, N, shards=shards)
        L.check(c, N, *got, what=f"{shards} shards")
        full = ops.token_logprobs(c.logits, c.V, c.tokens, N)
        assert torch.equal(got[2], full[2])


def test_partial_packs_of_real_ranks():
    """Two ranks' own shards (lo > 0), gathered rank-major, give the full row's result."""
    c = L.cases()["v101-pad112-bf16"]
    half = c.ld // 2
    packs = [R.token_logprobs_partial(c.logits[:, r * half:(r + 1) * half], r * half, c.V, c.tokens, 5) for r in (0, 1)]
    L.check(c, 5, *R.token_logprobs_combine(torch.cat(packs, dim=1), 5), what="2 ranks")


def test_n_range_is_validated():
    c = L.cases()["v13-f32-unaligned"]
    for bad in (-1, 21, 2.0):
        with pytest.raises(ValueError):
            ops.token_logprobs(c.logits, c.V, c.tokens, bad)
