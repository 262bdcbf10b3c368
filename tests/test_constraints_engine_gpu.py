"""Token constraints through the GPU engine: graph-captured, pipelined decode against the same engine decoding eagerly
across a bucket change, greedy tokens against the fp64 oracle over a one-shot prefill's logits, default requests and a
constraints=False engine unchanged, log-probabilities still those of the raw distribution, and a slot taken in a
decode step that replays its graph."""
import struct

import pytest
import torch

import constraint_cases as C
import penalty_cases as P
from llmss_amd.engine import LLMEngine, SamplingParams
from llmss_amd.engine.sampling import MAX_TOKEN_EDITS
from llmss_amd.models.config import get_preset
from llmss_amd.models.decoder import DecoderLM, StepInput
from llmss_amd.models.weights import random_weights

pytestmark = pytest.mark.gpu
N = 5
NEW = 24
# rows 1 and 3 leave early; the pipelined decode keeps their rows as padding until the scheduler runs again, which the
# late arrival of a sixth request forces: the batch then falls from the 8-row bucket into the 4-row one
LENS = (24, 6, 24, 10, 24)
LATE = 14  # engine steps before the sixth request arrives
NEAR_TIE = 0.1  # test_engine_gpu._near_tie: a 0.05 per-logit difference between kernel routes is bf16 noise


def _bits(x):
    return struct.pack("<f", x)


def run(eng, prompts, sps, late=None):
    """``late``: (prompt, params) of one more request that arrives after LATE engine steps."""
    rids = [eng.add_request(p, sp) for p, sp in zip(prompts, sps)]
    events, done, steps = [], {}, 0
    while eng.has_unfinished():
        events += eng.step()
        steps += 1
        if late is not None and steps == LATE:
            rids.append(eng.add_request(*late))
        for r in eng.pop_finished():
            done[r.id] = r
    return [done[i] for i in rids], events


def _sps(cons, lens=(NEW,) * 5, logprobs=None):
    """Rows 0-2 greedy, rows 3-4 sampled with fixed seeds, row i with the constraint fields cons[i]."""
    out = []
    for i, con in enumerate(cons):
        kw = dict(max_new_tokens=lens[i], ignore_eos=True, logprobs=logprobs, **con)
        if i < 3:
            kw.update(is_greedy=True)
        else:
            kw.update(temperature=0.8, top_k=20, top_p=0.9, seed=11 + i)
        out.append(SamplingParams(**kw))
    return out


NONE = [{}] * 5


@pytest.fixture(scope="module")
def setup():
    cfg = get_preset("tiny-llama", hidden_size=256, num_heads=4, num_kv_heads=2, head_dim=64, rotary_dim=64,
                     intermediate_size=512, max_position_embeddings=256)
    w = random_weights(cfg, device="cuda", dtype=torch.bfloat16, seed=3, std=0.05)
    m = DecoderLM(cfg, w)
    g = torch.Generator().manual_seed(0)
    prompts = [[int(x) for x in torch.randint(0, cfg.vocab_size, (n,), generator=g)] for n in (5, 17, 33, 2, 60)]
    on = LLMEngine(m, max_num_seqs=8, block_size=16, use_graphs=True, max_logprobs=N, penalties=True, constraints=True)
    off = LLMEngine(m, max_num_seqs=8, block_size=16, use_graphs=True, max_logprobs=N)
    plain, _ = run(on, prompts, _sps(NONE))
    return cfg, m, prompts, on, off, plain


def derive(plain, V):
    """Five rows' constraints, each violated by the unconstrained output of its row."""
    outs = [r.output_ids for r in plain]
    absent = lambda i, n: [t for t in range(V) if t not in outs[i]][7:7 + n]  # noqa: E731
    return [dict(banned_token_ids=list(dict.fromkeys(outs[0]))[:3], logit_bias={absent(0, 1)[0]: 1.0}),
            dict(allowed_token_ids=absent(1, 40), logit_bias={absent(1, 1)[0]: -2.0}),
            dict(logit_bias={absent(2, 1)[0]: 100.0}, repetition_penalty=1.3, presence_penalty=0.5),
            dict(banned_token_ids=list(dict.fromkeys(outs[3]))[:MAX_TOKEN_EDITS]),
            dict(stop_token_ids=[outs[4][1]], min_tokens=5, allowed_token_ids=sorted(set(outs[4]) | set(absent(4, 30))))]


def idle(eng):
    return (not eng._con_slot and sorted(eng._con_free) == list(range(eng.max_num_seqs))
            and not eng._pen_slot and sorted(eng._pen_free) == list(range(eng.max_num_seqs)))


def satisfied(reqs, cons):
    for r, con in zip(reqs, cons):
        o = r.output_ids
        assert not set(con.get("banned_token_ids", [])) & set(o)
        assert not con.get("allowed_token_ids") or set(o) <= set(con["allowed_token_ids"])
        if con.get("min_tokens"):
            assert len(o) >= min(con["min_tokens"], r.params.max_new_tokens)
            assert not set(o[:con["min_tokens"] - 1]) & set(con["stop_token_ids"])


def _raw_logits(m, r):
    """[len(output), width] logits of a one-shot prefill of prompt + output: row t is the distribution of output[t]."""
    ids = r.prompt_ids + r.output_ids
    T, Pn = len(ids), len(r.prompt_ids)
    x = torch.tensor(ids, device="cuda")
    return m(StepInput("prefill", x, torch.arange(T, device="cuda"), torch.full((T,), -1, device="cuda"),
                       cu_seqlens=torch.tensor([0, T], dtype=torch.int32, device="cuda"), max_seqlen=T,
                       last_idx=torch.arange(Pn - 1, T - 1, device="cuda")), m.allocate_kv_cache(8, 16))


def test_graphs_equal_eager_across_a_bucket_change(setup):
    cfg, m, prompts, on, off, plain = setup
    assert on.use_graphs and on.graphs and on.async_decode
    assert on.stats["constraint_state_bytes"] == 8 * (4 * MAX_TOKEN_EDITS + 4) * 4
    cons = derive(plain, cfg.vocab_size)
    late = (prompts[1][:9], SamplingParams(max_new_tokens=12, ignore_eos=True, is_greedy=True, **cons[0]))
    buckets = []
    inner = on.buf.fill
    on.buf.fill = lambda k, b_pad, *a, **kw: (buckets.append(b_pad), inner(k, b_pad, *a, **kw))[1]
    try:
        reqs, _ = run(on, prompts, _sps(cons, LENS), late=late)
    finally:
        on.buf.fill = inner
    assert len(set(buckets)) >= 2 and all((b, False) in on.graphs for b in set(buckets)), sorted(set(buckets))
    assert idle(on)
    on.use_graphs = False
    try:
        eager, _ = run(on, prompts, _sps(cons, LENS), late=late)
    finally:
        on.use_graphs = True
    assert len(reqs) == 6 and reqs[5].output_ids == eager[5].output_ids and len(reqs[5].output_ids) == 12
    assert not set(cons[0]["banned_token_ids"]) & set(reqs[5].output_ids)
    for r, e, n, p in zip(reqs, eager, LENS, plain):
        assert r.output_ids == e.output_ids
        assert len(r.output_ids) == n or r.params.stop_token_ids
        assert r.output_ids != p.output_ids[:len(r.output_ids)]  # the unconstrained run violates the constraint
    satisfied(reqs, cons)
    # the stop token ends the unconstrained row 4 after at most two tokens, min_tokens = 5 holds it back
    short, _ = run(on, prompts[4:], [SamplingParams(max_new_tokens=NEW, ignore_eos=True, temperature=0.8, top_k=20,
                                                    top_p=0.9, seed=15, stop_token_ids=cons[4]["stop_token_ids"])])
    assert short[0].finish_reason == "stop" and len(short[0].output_ids) <= 2 and len(reqs[4].output_ids) >= 5


def test_teacher_forced_greedy_tokens(setup):
    cfg, m, prompts, on, off, plain = setup
    V = cfg.vocab_size
    cons = derive(plain, V)
    reqs, _ = run(on, prompts, _sps(cons))
    satisfied(reqs, cons)
    worst = 0.0
    for r in reqs[:3]:
        q = r.params
        lg = _raw_logits(m, r)[:, :V].double().cpu().numpy()
        for t, tok in enumerate(r.output_ids):
            row = lg[t]
            if q.has_penalties:
                row = P.penalise_row(row, r.prompt_ids, r.output_ids[:t], q.repetition_penalty, q.presence_penalty,
                                     q.frequency_penalty)
            row = C.constrain_row(row, q, on.eos, t)
            gap = float(row.max() - row[tok])
            worst = max(worst, gap)
            assert gap <= NEAR_TIE, (r.id, t, tok, int(row.argmax()), gap)
    print(f"largest gap to the constrained maximum: {worst:.4f}")
    assert set(reqs[2].output_ids) == set(cons[2]["logit_bias"])  # + 100 forces the token at every step
    assert idle(on)


def test_default_requests_and_disabled_engine_unchanged(setup):
    cfg, m, prompts, on, off, plain = setup
    a, _ = run(on, prompts, _sps(NONE, logprobs=N))
    b, _ = run(off, prompts, _sps(NONE, logprobs=N))
    snap = lambda rs: [(r.output_ids, [_bits(v) for v in r.output_logprobs],  # noqa: E731
                        [[(i, _bits(v)) for i, v in top] for top in r.output_top_logprobs]) for r in rs]
    assert snap(a) == snap(b)
    # off: graph keys, buffers and fingerprint as without the feature
    assert off.constraints is False and off.con_state is None and "constraint_state_bytes" not in off.stats
    assert sorted(off.graphs) == sorted(on.graphs)
    buf, B, MB = off.buf, off.buf.max_b, off.buf.max_blocks
    assert not hasattr(buf, "cslot") and not hasattr(buf, "cnout") and not hasattr(buf, "_logits_out")
    assert not hasattr(buf, "pslot") and not hasattr(buf, "rep")
    assert buf.o32 == 32 * B and buf.of32 == buf.o32 + (2 * B + B * MB) * 4 and buf.d.numel() == buf.of32 + 8 * B
    assert buf.topp.data_ptr() + 4 * B == buf.d.data_ptr() + buf.d.numel()
    # on (penalties and constraints): pslot, then cslot and cnout, end the int32 part; rep / pres / freq the fp32 one
    ob = on.buf
    assert ob.d.numel() == buf.d.numel() + 16 * B + 8 * B and ob.pslot.numel() == ob.cslot.numel() == ob.cnout.numel() == B
    assert ob.cslot.data_ptr() == ob.pslot.data_ptr() + 4 * B and ob.cnout.data_ptr() == ob.cslot.data_ptr() + 4 * B
    assert ob.cnout.data_ptr() + 4 * B == ob.temp.data_ptr() == ob.d.data_ptr() + ob.of32
    fa, fb = off.fingerprint(), on.fingerprint()
    assert fa.pop("constraints") is False and fb.pop("constraints") is True
    assert fa.pop("penalties") is False and fb.pop("penalties") is True and fa == fb
    with pytest.raises(ValueError, match="constraints=True"):
        off.add_request([1, 2, 3], SamplingParams(max_new_tokens=2, banned_token_ids=[5]))
    assert not off.has_unfinished() and not off.requests


def test_logprobs_stay_raw(setup):
    cfg, m, prompts, on, off, plain = setup
    V = cfg.vocab_size
    absent = [t for t in range(V) if all(t not in r.output_ids for r in plain)]
    cons = [dict(logit_bias={absent[i]: 100.0}) for i in range(5)]
    reqs, _ = run(on, prompts, _sps(cons, logprobs=N))
    for r, con in zip(reqs[:3], cons):
        assert set(r.output_ids) == set(con["logit_bias"])  # forced
    for r in reqs:
        want = torch.log_softmax(_raw_logits(m, r)[:, :V].double(), dim=-1).cpu()
        assert len(r.output_logprobs) == NEW
        for t, (tok, lp, top) in enumerate(zip(r.output_ids, r.output_logprobs, r.output_top_logprobs)):
            assert abs(lp - want[t, tok].item()) <= 0.1, (r.id, t, lp, want[t, tok].item())
            for i, v in top:
                assert abs(v - want[t, i].item()) <= 0.1
    # under the constrained distribution a forced token's log-probability would be about 0
    for r in reqs[:3]:
        assert max(r.output_logprobs) < -0.5


def test_slot_taken_in_a_decode_step_replays_the_graph(setup):
    """Chunked prefill (chunks of 4) with prompts of 5, 9 and 13 tokens: the scheduler hands the last chunk, one token,
    out as a decode row, which takes its constraint slot there. The slot is written ahead of the launch and nothing
    else about the step changes, so it replays its graph. Tokens equal the engine decoding eagerly throughout."""
    cfg, m, prompts, on, off, plain = setup
    V = cfg.vocab_size
    g = torch.Generator().manual_seed(1)
    ps = [[int(x) for x in torch.randint(0, V, (n,), generator=g)] for n in (5, 9, 13, 6, 17)]
    eng = LLMEngine(m, max_num_seqs=8, block_size=16, use_graphs=True, constraints=True, prefill_chunk=4)
    assert eng.use_graphs and eng.graphs
    base, _ = run(eng, ps, _sps(NONE))
    cons = derive(base, V)
    cons[2] = {k: v for k, v in cons[2].items() if "penalty" not in k}  # this engine has no penalties
    calls = {"took_in_decode": 0, "eager_decode": 0}
    acquire, forward = eng._con_acquire, eng._decode_forward
    state = {"in_record": False}
    record = eng._record_from_batch

    def counted_record(*a, **kw):
        state["in_record"] = True
        try:
            return record(*a, **kw)
        finally:
            state["in_record"] = False

    def counted_acquire(reqs):
        took = acquire(reqs)
        calls["took_in_decode"] += int(took and state["in_record"])
        return took

    def counted_forward(*a, **kw):
        calls["eager_decode"] += 1
        return forward(*a, **kw)
    eng._record_from_batch, eng._con_acquire, eng._decode_forward = counted_record, counted_acquire, counted_forward
    reqs, _ = run(eng, ps, _sps(cons))
    eng._record_from_batch, eng._con_acquire, eng._decode_forward = record, acquire, forward
    assert calls["took_in_decode"] > 0 and calls["eager_decode"] == 0, calls
    assert not eng._con_slot and sorted(eng._con_free) == list(range(8))
    satisfied(reqs, cons)
    eng.use_graphs = False
    try:
        eager, _ = run(eng, ps, _sps(cons))
    finally:
        eng.use_graphs = True
    assert [r.output_ids for r in reqs] == [r.output_ids for r in eager]
    assert [r.output_ids for r in reqs] != [r.output_ids for r in base]
