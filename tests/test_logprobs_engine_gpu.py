"""Per-token log-probabilities through the GPU engine: the graph-captured, pipelined decode against the same engine
decoding eagerly (bit-identical), structural properties of every reported list, and the values against an fp64
log-softmax of a one-shot prefill on the same model."""
import math
import struct

import pytest
import torch

from llmss_amd.engine import LLMEngine, SamplingParams
from llmss_amd.models.config import get_preset
from llmss_amd.models.decoder import DecoderLM, StepInput
from llmss_amd.models.weights import random_weights

pytestmark = pytest.mark.gpu
N = 5
NEW = 24


def _bits(x):
    return struct.pack("<f", x)


def run(eng, prompts, sps):
    rids = [eng.add_request(p, sp) for p, sp in zip(prompts, sps)]
    events, done = [], {}
    while eng.has_unfinished():
        events += eng.step()
        for r in eng.pop_finished():
            done[r.id] = r
    return [done[i] for i in rids], events


def _sps(stop=None):
    """Rows 0-2 greedy, rows 3-4 sampled with fixed seeds; ``stop``: row 0 stops on that token."""
    out = [SamplingParams(max_new_tokens=NEW, is_greedy=True, ignore_eos=True, logprobs=N) for _ in range(3)]
    out += [SamplingParams(max_new_tokens=NEW, temperature=0.8, top_k=20, top_p=0.9, seed=11 + i, ignore_eos=True,
                           logprobs=N) for i in range(2)]
    if stop is not None:
        out[0] = SamplingParams(max_new_tokens=NEW, is_greedy=True, ignore_eos=True, logprobs=N, stop_token_ids=[stop])
    return out


@pytest.fixture(scope="module")
def setup():
    cfg = get_preset("tiny-llama", hidden_size=256, num_heads=4, num_kv_heads=2, head_dim=64, rotary_dim=64,
                     intermediate_size=512, max_position_embeddings=256)
    w = random_weights(cfg, device="cuda", dtype=torch.bfloat16, seed=3, std=0.05)
    m = DecoderLM(cfg, w)
    g = torch.Generator().manual_seed(0)
    prompts = [[int(x) for x in torch.randint(0, cfg.vocab_size, (n,), generator=g)] for n in (5, 17, 33, 2, 60)]
    eng = LLMEngine(m, max_num_seqs=8, block_size=16, use_graphs=True, max_logprobs=N)
    return cfg, m, prompts, eng


def _snapshot(reqs):
    return [(r.output_ids, [_bits(v) for v in r.output_logprobs],
             [[(i, _bits(v)) for i, v in top] for top in r.output_top_logprobs]) for r in reqs]


def test_graphs_equal_eager_and_lists_are_well_formed(setup):
    cfg, m, prompts, eng = setup
    assert eng.use_graphs and eng.graphs and eng.async_decode
    reqs, events = run(eng, prompts, _sps())
    assert eng.stats["decode_steps"] > 0
    eng.use_graphs = False
    try:
        eager, _ = run(eng, prompts, _sps())
    finally:
        eng.use_graphs = True
    # the same kernels on the same plans, captured or launched one by one: identical bits
    assert _snapshot(reqs) == _snapshot(eager)
    V = cfg.vocab_size
    by_req = {}
    for e in events:
        by_req.setdefault(e.req_id, []).append(e)
    for k, r in enumerate(reqs):
        assert len(r.output_ids) == NEW == len(r.output_logprobs) == len(r.output_top_logprobs)
        assert len(r.prompt_ids) + NEW > 16  # every sequence crosses a KV block boundary (or starts past one)
        assert [(e.token, e.logprob, e.top_logprobs) for e in by_req[r.id]] == \
            list(zip(r.output_ids, r.output_logprobs, r.output_top_logprobs))
        for tok, lp, top in zip(r.output_ids, r.output_logprobs, r.output_top_logprobs):
            ids, vals = [i for i, _ in top], [v for _, v in top]
            assert len(top) == N and len(set(ids)) == N and all(0 <= i < V for i in ids)
            assert vals == sorted(vals, reverse=True) and all(v <= 0 for v in vals) and lp <= 0
            assert all(a[1] > b[1] or a[0] < b[0] for a, b in zip(top, top[1:]))  # equal values: ascending id
            assert sum(math.exp(v) for v in vals) <= 1 + 1e-5
            if tok in ids:
                assert _bits(vals[ids.index(tok)]) == _bits(lp)
            else:
                assert lp <= vals[-1]
            if k < 3:  # greedy rows: the chosen token leads the list, with the same bits
                assert top[0][0] == tok and _bits(top[0][1]) == _bits(lp)
    # values: an fp64 log-softmax of a one-shot prefill of prompt + output on the same model; row
    # len(prompt) - 1 + t is the distribution of output[t]. 0.1: a 0.05 per-logit difference between kernel
    # routes is bf16 noise (test_engine_gpu._near_tie), and the token's logit and the log-sum-exp each move by
    # at most that much
    for r in reqs:
        ids = r.prompt_ids + r.output_ids
        T, P = len(ids), len(r.prompt_ids)
        x = torch.tensor(ids, device="cuda")
        lg = m(StepInput("prefill", x, torch.arange(T, device="cuda"), torch.full((T,), -1, device="cuda"),
                         cu_seqlens=torch.tensor([0, T], dtype=torch.int32, device="cuda"), max_seqlen=T,
                         last_idx=torch.arange(P - 1, T - 1, device="cuda")), m.allocate_kv_cache(8, 16))
        want = torch.log_softmax(lg[:, :V].double(), dim=-1).cpu()
        for t, (tok, lp, top) in enumerate(zip(r.output_ids, r.output_logprobs, r.output_top_logprobs)):
            assert abs(lp - want[t, tok].item()) <= 0.1, (r.id, t, lp, want[t, tok].item())
            for i, v in top:
                assert abs(v - want[t, i].item()) <= 0.1


def test_stop_token_mid_pipeline_keeps_lengths(setup):
    cfg, m, prompts, eng = setup
    base, _ = run(eng, prompts, _sps())
    stop = base[0].output_ids[9]
    cut = base[0].output_ids.index(stop) + 1
    reqs, events = run(eng, prompts, _sps(stop=stop))
    assert reqs[0].finish_reason == "stop" and reqs[0].output_ids == base[0].output_ids[:cut]
    for r, b in zip(reqs, base):
        assert len(r.output_logprobs) == len(r.output_ids) == len(r.output_top_logprobs)
        n = len(r.output_ids)
        assert _snapshot([r])[0][0] == b.output_ids[:n]
    assert sum(1 for e in events if e.req_id == reqs[0].id) == cut  # the speculated extra token was dropped whole
    assert all(e.logprob is not None for e in events)


def test_disabled_engine_is_unchanged(setup):
    cfg, m, prompts, eng = setup
    off = LLMEngine(m, max_num_seqs=8, block_size=16, use_graphs=True)
    assert off.max_logprobs == 0 and not hasattr(off.buf, "lp_f") and off.buf.lp_out(8) is None
    assert sorted(off.graphs) == sorted(eng.graphs)
    fa, fb = off.fingerprint(), eng.fingerprint()
    assert fa.pop("max_logprobs") == 0 and fb.pop("max_logprobs") == N and fa == fb
    with pytest.raises(ValueError):
        off.add_request([1, 2, 3], SamplingParams(max_new_tokens=2, logprobs=0))
    plain = [SamplingParams(max_new_tokens=NEW, is_greedy=True, ignore_eos=True) for _ in prompts]
    assert off.generate(prompts, plain) == eng.generate(prompts, plain)
