"""Sliding-window attention through the engine on the GPU: the `tiny-mistral` preset (head dim 64, window 32, 16-token
pages), prompts of 5, 40 and 100 tokens and 80 new tokens each, greedy, with HIP graphs and the pipelined decode both
on and both off."""
import dataclasses

import pytest
import torch

from llmss_amd.engine import LLMEngine, SamplingParams
from llmss_amd.models.config import get_preset
from llmss_amd.models.decoder import DecoderLM, StepInput
from llmss_amd.models.weights import random_weights
from test_engine_gpu import _to_gpu

pytestmark = pytest.mark.gpu

MODES = [pytest.param(True, True, id="graphs-pipelined"), pytest.param(False, False, id="eager-serial")]
SP = SamplingParams(max_new_tokens=80, is_greedy=True, ignore_eos=True)


@pytest.fixture(scope="module")
def setup():
    cfg = get_preset("tiny-mistral")
    assert (cfg.head_dim, cfg.sliding_window) == (64, 32)
    wc = random_weights(cfg, device="cpu", dtype=torch.float32, seed=4, std=0.05)
    g = torch.Generator().manual_seed(7)
    prompts = [[int(x) for x in torch.randint(0, cfg.vocab_size, (n,), generator=g)] for n in (5, 40, 100)]
    return cfg, wc, _to_gpu(wc), prompts


def engine(cfg, w, graphs, pipelined, num_blocks=256):
    eng = LLMEngine(DecoderLM(cfg, w), max_num_seqs=4, block_size=16, num_blocks=num_blocks, use_graphs=graphs,
                    autotune=False)
    eng.async_decode = pipelined
    return eng


@pytest.mark.parametrize("graphs,pipelined", MODES)
def test_a_window_no_sequence_reaches_changes_no_token(setup, graphs, pipelined):
    """Window 200 >= every sequence length (180): the windowed kernels run (the window is below the model length) and
    mask nothing, so the tokens are those of the unwindowed engine."""
    cfg, _, wg, prompts = setup
    wide = dataclasses.replace(cfg, sliding_window=200)
    plain = dataclasses.replace(cfg, sliding_window=0)
    e_w, e_p = engine(wide, wg, graphs, pipelined), engine(plain, wg, graphs, pipelined)
    assert e_w.window == 200 and e_p.window == 0
    assert e_w.generate(prompts, SP) == e_p.generate(prompts, SP)


@pytest.mark.parametrize("graphs,pipelined", MODES)
def test_a_pool_smaller_than_the_sequences(setup, graphs, pipelined):
    """The three sequences end at 85, 120 and 180 tokens: 26 pages unwindowed. With window 32 a sequence holds at
    most 6 pages, so a pool of 20 serves them - with the tokens of a large pool, and every block free at the end."""
    cfg, _, wg, prompts = setup
    small, big = engine(cfg, wg, graphs, pipelined, 20), engine(cfg, wg, graphs, pipelined, 256)
    out = small.generate(prompts, SP)
    assert out == big.generate(prompts, SP)
    assert small.sched.num_free_blocks() == 20 and big.sched.num_free_blocks() == 256
    assert small.stats["preemptions"] == 0 and 0 < small.stats["peak_live_kv_blocks"] <= 18
    if not graphs:  # the same pool without the window has to preempt
        plain = engine(dataclasses.replace(cfg, sliding_window=0), wg, False, False, 20)
        plain.generate(prompts, SP)
        assert plain.stats["preemptions"] > 0 and plain.stats["peak_live_kv_blocks"] > 18


def fp32_logits(m, seq):
    """Next-token logits after ``seq`` from the windowed CPU model, fed in chunks of at most the window."""
    cfg, W, bs = m.cfg, m.cfg.sliding_window, 16
    nb = -(-len(seq) // bs)
    kv = m.allocate_kv_cache(nb, bs)
    table = torch.arange(nb, dtype=torch.int32)[None]
    ids = torch.tensor(seq)
    for a in range(0, len(seq), W):
        e = min(len(seq), a + W)
        pos = torch.arange(a, e)
        out = m(StepInput("prefill" if a == 0 else "extend", ids[a:e], pos, pos.clone(),
                          cu_seqlens=torch.tensor([0, e - a], dtype=torch.int32), max_seqlen=e - a, block_tables=table,
                          ctx_lens=torch.tensor([e], dtype=torch.int32), max_ctx=nb * bs, has_prefix=a > 0, window=W,
                          last_idx=torch.tensor([e - a - 1])), kv)
    return out[0, : cfg.vocab_size]


@pytest.mark.parametrize("graphs,pipelined", MODES)
def test_against_the_fp32_engine(setup, graphs, pipelined):
    """The rule of test_gpu_chunked_engine_matches_whole_prompt: a greedy pick may differ from the CPU fp32 engine's
    only where the fp32 top-2 margin is below 0.1, and the comparison of that sequence stops there."""
    cfg, wc, wg, prompts = setup
    m_cpu = DecoderLM(cfg, wc)
    ref = LLMEngine(m_cpu, max_num_seqs=4, block_size=16, num_blocks=64).generate(prompts, SP)
    got = engine(cfg, wg, graphs, pipelined).generate(prompts, SP)
    compared = 0
    for p, g, r in zip(prompts, got, ref):
        assert len(g) == len(r) == 80
        for k, (a, b) in enumerate(zip(g, r)):
            if a == b:
                compared += 1
                continue
            top2 = fp32_logits(m_cpu, p + r[:k]).topk(2).values
            assert float(top2[0] - top2[1]) < 0.1, ("GPU and fp32 engines differ at a clear margin", k, top2.tolist())
            break
    assert compared >= 0.6 * sum(len(x) for x in ref), (compared, got, ref)
