"""Repetition / presence / frequency penalties through the GPU engine: graph-captured, pipelined decode against the
same engine decoding eagerly, greedy tokens against the fp64 oracle over a one-shot prefill's logits, a stop token
mid-pipeline, default requests and a penalties=False engine unchanged, log-probabilities still those of the raw
distribution."""
import struct

import pytest
import torch

import penalty_cases as P
from llmss_amd.engine import LLMEngine, SamplingParams
from llmss_amd.models.config import get_preset
from llmss_amd.models.decoder import DecoderLM, StepInput
from llmss_amd.models.weights import random_weights

pytestmark = pytest.mark.gpu
N = 5
NEW = 24
NEAR_TIE = 0.1  # test_engine_gpu._near_tie: a 0.05 per-logit difference between kernel routes is bf16 noise


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


def _sps(pens, stop=None, logprobs=None):
    """Rows 0-2 greedy, rows 3-4 sampled with fixed seeds, row i with penalties pens[i]; ``stop``: row 0 stops on it."""
    out = []
    for i, (r, p, f) in enumerate(pens):
        kw = dict(max_new_tokens=NEW, ignore_eos=True, repetition_penalty=r, presence_penalty=p, frequency_penalty=f,
                  logprobs=logprobs)
        if i < 3:
            kw.update(is_greedy=True)
        else:
            kw.update(temperature=0.8, top_k=20, top_p=0.9, seed=11 + i)
        if i == 0 and stop is not None:
            kw.update(stop_token_ids=[stop])
        out.append(SamplingParams(**kw))
    return out


NONE = [(1.0, 0.0, 0.0)] * 5
MIXED = [(1.3, 0.0, 0.0), (1.0, 2.0, 1.0), (1.5, 0.7, 0.45), (1.2, 0.5, 0.25), (1.0, 1.0, 0.5)]
STRONG = [(1.0, 2.0, 1.0)] * 5  # a missing or stale count moves a logit by at least 2


@pytest.fixture(scope="module")
def setup():
    cfg = get_preset("tiny-llama", hidden_size=256, num_heads=4, num_kv_heads=2, head_dim=64, rotary_dim=64,
                     intermediate_size=512, max_position_embeddings=256)
    w = random_weights(cfg, device="cuda", dtype=torch.bfloat16, seed=3, std=0.05)
    m = DecoderLM(cfg, w)
    g = torch.Generator().manual_seed(0)
    prompts = [[int(x) for x in torch.randint(0, cfg.vocab_size, (n,), generator=g)] for n in (5, 17, 33, 2, 60)]
    on = LLMEngine(m, max_num_seqs=8, block_size=16, use_graphs=True, max_logprobs=N, penalties=True)
    off = LLMEngine(m, max_num_seqs=8, block_size=16, use_graphs=True, max_logprobs=N)
    return cfg, m, prompts, on, off


def idle(eng):
    return not eng._pen_slot and sorted(eng._pen_free) == list(range(eng.max_num_seqs))


def _raw_logits(m, r):
    """[len(output), width] logits of a one-shot prefill of prompt + output: row t is the distribution of output[t]."""
    ids = r.prompt_ids + r.output_ids
    T, Pn = len(ids), len(r.prompt_ids)
    x = torch.tensor(ids, device="cuda")
    return m(StepInput("prefill", x, torch.arange(T, device="cuda"), torch.full((T,), -1, device="cuda"),
                       cu_seqlens=torch.tensor([0, T], dtype=torch.int32, device="cuda"), max_seqlen=T,
                       last_idx=torch.arange(Pn - 1, T - 1, device="cuda")), m.allocate_kv_cache(8, 16))


def test_graphs_equal_eager(setup):
    cfg, m, prompts, on, off = setup
    assert on.use_graphs and on.graphs and on.async_decode
    assert on.stats["penalty_state_bytes"] == 8 * cfg.vocab_size * 4
    d0 = on.stats["decode_steps"]
    reqs, _ = run(on, prompts, _sps(MIXED))
    assert on.stats["decode_steps"] > d0 and idle(on)
    on.use_graphs = False
    try:
        eager, _ = run(on, prompts, _sps(MIXED))
    finally:
        on.use_graphs = True
    for r, e in zip(reqs, eager):
        assert len(r.output_ids) == NEW and len(r.prompt_ids) + NEW > 16  # crosses a KV block edge (or starts past one)
        assert r.output_ids == e.output_ids
    plain, _ = run(on, prompts, _sps(NONE))
    assert [r.output_ids for r in plain] != [r.output_ids for r in reqs]


def test_teacher_forced_greedy_tokens(setup):
    cfg, m, prompts, on, off = setup
    V = cfg.vocab_size
    plain, _ = run(on, prompts, _sps(NONE))
    assert all(len(set(r.output_ids)) < NEW for r in plain[:3]), "the unpenalised greedy rows do not repeat tokens"
    reqs, _ = run(on, prompts, _sps(STRONG))
    worst = 0.0
    for r in reqs[:3]:
        lg = _raw_logits(m, r)[:, :V].double().cpu().numpy()
        for t, tok in enumerate(r.output_ids):
            pen = P.penalise_row(lg[t], r.prompt_ids, r.output_ids[:t], 1.0, 2.0, 1.0)
            gap = float(pen.max() - pen[tok])
            worst = max(worst, gap)
            assert gap <= NEAR_TIE, (r.id, t, tok, int(pen.argmax()), gap)
    print(f"largest gap to the penalised maximum: {worst:.4f}")
    assert idle(on)


def test_stop_token_mid_pipeline_frees_the_slot(setup):
    cfg, m, prompts, on, off = setup
    base, _ = run(on, prompts, _sps(MIXED))
    stop = base[0].output_ids[9]
    cut = base[0].output_ids.index(stop) + 1
    reqs, events = run(on, prompts, _sps(MIXED, stop=stop))
    assert reqs[0].finish_reason == "stop" and reqs[0].output_ids == base[0].output_ids[:cut]
    for r, b in zip(reqs[1:], base[1:]):
        assert r.output_ids == b.output_ids
    assert sum(1 for e in events if e.req_id == reqs[0].id) == cut  # the speculated extra token was dropped
    assert idle(on)
    # the freed row serves the next holder: rebuilt whole, whatever the dropped step registered in it
    again, _ = run(on, prompts, _sps(MIXED))
    assert [r.output_ids for r in again] == [r.output_ids for r in base]


def test_default_requests_and_disabled_engine_unchanged(setup):
    cfg, m, prompts, on, off = setup
    a, _ = run(on, prompts, _sps(NONE, logprobs=N))
    b, _ = run(off, prompts, _sps(NONE, logprobs=N))
    snap = lambda rs: [(r.output_ids, [_bits(v) for v in r.output_logprobs],  # noqa: E731
                        [[(i, _bits(v)) for i, v in top] for top in r.output_top_logprobs]) for r in rs]
    assert snap(a) == snap(b)
    # off: graph keys, buffers and fingerprint as without the feature
    assert off.penalties is False and off.pen_state is None and "penalty_state_bytes" not in off.stats
    assert sorted(off.graphs) == sorted(on.graphs)
    buf, B, MB = off.buf, off.buf.max_b, off.buf.max_blocks
    assert not hasattr(buf, "pslot") and not hasattr(buf, "rep") and not hasattr(buf, "_logits_out")
    assert buf.o32 == 32 * B and buf.of32 == buf.o32 + (2 * B + B * MB) * 4 and buf.d.numel() == buf.of32 + 8 * B
    assert buf.topp.data_ptr() + 4 * B == buf.d.data_ptr() + buf.d.numel()
    assert on.buf.d.numel() == buf.d.numel() + 16 * B and on.buf.pslot.numel() == B == on.buf.freq.numel()
    fa, fb = off.fingerprint(), on.fingerprint()
    assert fa.pop("penalties") is False and fb.pop("penalties") is True and fa == fb
    with pytest.raises(ValueError):
        off.add_request([1, 2, 3], SamplingParams(max_new_tokens=2, presence_penalty=0.5))
    assert not off.has_unfinished() and not off.requests


def test_logprobs_stay_raw(setup):
    cfg, m, prompts, on, off = setup
    V = cfg.vocab_size
    reqs, _ = run(on, prompts, _sps(STRONG, logprobs=N))
    plain, _ = run(on, prompts, _sps(NONE, logprobs=N))
    assert [r.output_ids for r in reqs] != [r.output_ids for r in plain]
    for r in reqs:
        want = torch.log_softmax(_raw_logits(m, r)[:, :V].double(), dim=-1).cpu()
        assert len(r.output_logprobs) == NEW
        for t, (tok, lp, top) in enumerate(zip(r.output_ids, r.output_logprobs, r.output_top_logprobs)):
            assert abs(lp - want[t, tok].item()) <= 0.1, (r.id, t, lp, want[t, tok].item())
            for i, v in top:
                assert abs(v - want[t, i].item()) <= 0.1


def test_last_chunk_of_one_token_takes_its_row_in_a_decode_step(setup):
    """Chunked prefill (chunks of 4) with prompts of 5, 9 and 13 tokens: the scheduler hands the last chunk, one token,
    out as a decode row. That row takes its state row there, and the step runs eagerly with its own tokens to
    register instead of replaying the graph. Tokens equal the engine decoding eagerly throughout, and every greedy
    token sits at the oracle-penalised maximum of a one-shot prefill (p = 2: a prompt token counted as output, or a
    missing count, moves a logit by at least 2)."""
    cfg, m, prompts, on, off = setup
    V = cfg.vocab_size
    g = torch.Generator().manual_seed(1)
    ps = [[int(x) for x in torch.randint(0, V, (n,), generator=g)] for n in (5, 9, 13, 6, 17)]
    eng = LLMEngine(m, max_num_seqs=8, block_size=16, use_graphs=True, penalties=True, prefill_chunk=4)
    assert eng.use_graphs and eng.graphs
    calls = {"own": 0, "graph_bypassed": 0}
    inner = eng._decode_forward

    def counted(b, buf, dist=False, pnew=None):
        if pnew is not None:
            calls["own"] += 1
            calls["graph_bypassed"] += int(eng.use_graphs and (b, bool(dist)) in eng.graphs)
            assert (pnew[:b] == -1).any()
        return inner(b, buf, dist=dist, pnew=pnew)
    eng._decode_forward = counted
    reqs, _ = run(eng, ps, _sps(STRONG))
    assert calls["own"] > 0 and calls["graph_bypassed"] == calls["own"], calls
    assert idle(eng)
    eng.use_graphs = False
    try:
        eager, _ = run(eng, ps, _sps(STRONG))
    finally:
        eng.use_graphs = True
    assert [r.output_ids for r in reqs] == [r.output_ids for r in eager]
    for r in reqs[:3]:
        assert len(r.output_ids) == NEW
        lg = _raw_logits(m, r)[:, :V].double().cpu().numpy()
        for t, tok in enumerate(r.output_ids):
            pen = P.penalise_row(lg[t], r.prompt_ids, r.output_ids[:t], 1.0, 2.0, 1.0)
            assert float(pen.max() - pen[tok]) <= NEAR_TIE, (r.id, t, tok, int(pen.argmax()))
