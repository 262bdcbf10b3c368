"""Sliding-window attention end to end on the CPU (fp32): config parsing, the windowed reference ops, a tiny Mistral
against Hugging Face's eager attention (teacher-forced logits at every position, greedy engine output), preemption,
and TP=2 over gloo."""
import pytest
import torch

from llmss_amd import _native
from llmss_amd.engine import LLMEngine, SamplingParams
from llmss_amd.models.config import ModelConfig, get_preset
from llmss_amd.models.decoder import DecoderLM, StepInput
from llmss_amd.models.weights import load_hf_weights
from llmss_amd.ops import reference as R
from llmss_amd.utils.checkpoint import CheckpointReader, weight_files

W, BS, VOCAB = 8, 4, 101


def mistral_dict(**over):
    d = dict(model_type="mistral", hidden_size=64, num_hidden_layers=2, num_attention_heads=4, num_key_value_heads=2,
             intermediate_size=160, vocab_size=VOCAB, max_position_embeddings=64, sliding_window=W)
    d.update(over)
    return d


# ------------------------------------------------------------------------------------------- config
def test_config_parses_the_window():
    assert ModelConfig.from_hf_dict(mistral_dict()).sliding_window == 8
    assert ModelConfig.from_hf_dict(mistral_dict(sliding_window=None)).sliding_window == 0
    assert ModelConfig.from_hf_dict(mistral_dict(sliding_window=64)).sliding_window == 0   # == max positions
    assert ModelConfig.from_hf_dict(mistral_dict(sliding_window=4096)).sliding_window == 0
    no_key = mistral_dict()
    del no_key["sliding_window"]
    assert ModelConfig.from_hf_dict(no_key).sliding_window == 0
    # a Llama config is untouched, whatever it carries; an unwindowed Mistral is the Llama config
    llama = ModelConfig.from_hf_dict(mistral_dict(model_type="llama"))
    assert llama.sliding_window == 0
    assert ModelConfig.from_hf_dict(mistral_dict(sliding_window=None)) == llama
    m7 = get_preset("mistral-7b")
    assert (m7.hidden_size, m7.num_layers, m7.num_heads, m7.num_kv_heads, m7.head_dim, m7.intermediate_size,
            m7.vocab_size, m7.max_position_embeddings, m7.sliding_window) == (4096, 32, 32, 8, 128, 14336, 32000,
                                                                             32768, 4096)
    tiny = get_preset("tiny-mistral")
    assert tiny.head_dim == 64 and 0 < tiny.sliding_window < tiny.max_position_embeddings


# ------------------------------------------------------------------------------------ reference ops
def dense_window(q, k, v, scale, window, kv_start=0):
    """q [n, nh, D], k / v [n, nkv, D] of one sequence -> [n, nh*D]: row p attends max(kv_start, p-window+1)..p."""
    n, nh, D = q.shape
    g = nh // k.shape[1]
    kk, vv = k.repeat_interleave(g, 1).transpose(0, 1), v.repeat_interleave(g, 1).transpose(0, 1)
    s = torch.matmul(q.transpose(0, 1), kk.transpose(1, 2)) * scale
    i, j = torch.arange(n)[:, None], torch.arange(n)[None, :]
    dead = (j > i) | (j < kv_start)
    if window > 0:
        dead = dead | (j < i - window + 1)
    p = torch.softmax(s.masked_fill(dead, float("-inf")), -1).nan_to_num(0.0)
    return torch.matmul(p, vv).transpose(0, 1).reshape(n, nh * D)


@pytest.mark.parametrize("window,kv_start", [(8, 0), (5, 0), (0, 6), (8, 13), (64, 0)])
def test_reference_ops_match_dense_windowed_attention(window, kv_start):
    torch.manual_seed(0)
    nh, nkv, D, n, chunk = 4, 2, 16, 37, 11
    q, k, v = torch.randn(n, nh, D), torch.randn(n, nkv, D), torch.randn(n, nkv, D)
    nb = (n + BS - 1) // BS
    perm = torch.randperm(nb + 3)
    table = perm[:nb].to(torch.int32)[None]
    krows, vrows = torch.full(((nb + 3) * BS, nkv, D), 1e4), torch.full(((nb + 3) * BS, nkv, D), 1e4)
    slot = table[0].long()[torch.arange(n) // BS] * BS + torch.arange(n) % BS
    krows[slot], vrows[slot] = k, v
    kc, vc = (x.view(nb + 3, BS, nkv, D).permute(0, 2, 1, 3).contiguous() for x in (krows, vrows))
    # the entries below the lowest row's first key belong to released pages: point them at the spare pages
    lo_chunk = max(kv_start, n - chunk - window + 1 if window else 0, 0)
    lo_dec = max(kv_start, n - window if window else 0, 0)
    ks = torch.tensor([kv_start], dtype=torch.int32) if kv_start else None
    want = dense_window(q, k, v, 0.25, window, kv_start)
    scale = 0.25
    t = table.clone()
    t[0, : lo_chunk // BS] = perm[nb]
    got = R.attn_extend(q[n - chunk:].reshape(chunk, -1), kc, vc, t, torch.tensor([0, chunk]), torch.tensor([n]), nh,
                        nkv, D, scale, window=window, kv_starts=ks)
    assert torch.allclose(got, want[n - chunk:], atol=1e-5)
    t = table.clone()
    t[0, : lo_dec // BS] = perm[nb]
    got = R.attn_decode(q[n - 1:].reshape(1, -1), kc, vc, t, torch.tensor([n]), nh, nkv, D, scale, window=window,
                        kv_starts=ks)
    assert torch.allclose(got, want[n - 1:], atol=1e-5)


# --------------------------------------------------------------------------------------- HF parity
@pytest.fixture(scope="module")
def mistral(tmp_path_factory):
    from transformers import MistralConfig, MistralForCausalLM

    torch.manual_seed(0)
    d = {k: v for k, v in mistral_dict().items() if k != "model_type"}
    hf = MistralForCausalLM(MistralConfig(**d, attn_implementation="eager", bos_token_id=VOCAB - 1,
                                          eos_token_id=VOCAB - 1)).eval()
    path = str(tmp_path_factory.mktemp("mistral"))
    hf.save_pretrained(path, safe_serialization=True)
    cfg = ModelConfig.from_pretrained(path)
    assert cfg.sliding_window == W
    w = load_hf_weights(cfg, CheckpointReader(weight_files(path)), 1, 0, device="cpu", dtype=torch.float32)
    return path, hf, cfg, w


def test_teacher_forced_logits_match_hf(mistral):
    """A 24-token prompt in chunks of at most 8, then 16 decode steps, through the scheduler (which releases the
    blocks below the window: the pool holds 7 of the 10 blocks the sequence would need unwindowed). Logits at every
    position against HF's full forward with eager attention; 1e-4 is the project's fp32 bound."""
    _, hf, cfg, w = mistral
    m = DecoderLM(cfg, w)
    torch.manual_seed(3)
    seq = torch.randint(0, VOCAB - 1, (40,))
    with torch.no_grad():
        ref = hf(seq[None]).logits[0]
        full = hf.__class__(hf.config.__class__(**{**hf.config.to_dict(), "sliding_window": None})).eval()
        full.load_state_dict(hf.state_dict())
        unwindowed = full(seq[None]).logits[0]
    # the window matters from position W on (so a model that ignores it misses the bound below by far)
    assert float((ref[:W] - unwindowed[:W]).abs().max()) < 1e-5 < 1e-2 < float((ref[W:] - unwindowed[W:]).abs().max())
    pool = 7
    sched = _native().Scheduler(pool, BS, 2, 64, 64, 0, W)
    sched.add(0, 24, 17)  # the prompt's last row samples token 24, 16 decode steps compute positions 24 .. 39
    kv = m.allocate_kv_cache(pool, BS)
    got = torch.zeros(40, cfg.vocab_size)
    seen = 0
    while sched.has_work():
        b = sched.schedule()
        q, c = int(b.query_lens[0]), int(b.ctx_lens[0])
        assert q <= W
        pos = torch.from_numpy(b.positions)
        kind = "decode" if b.kind == 2 else ("prefill" if c == q else "extend")
        inp = StepInput(kind, seq[pos], pos, torch.from_numpy(b.slots), cu_seqlens=torch.tensor([0, q], dtype=torch.int32),
                        max_seqlen=q, block_tables=torch.from_numpy(b.block_table).to(torch.int32),
                        ctx_lens=torch.tensor([c], dtype=torch.int32), max_ctx=64, has_prefix=c > q, window=W)
        got[c - q:c] = m(inp, kv)[:, : cfg.vocab_size]
        seen = c
        if b.sample[0]:
            sched.on_token(0, False)
    assert seen == 40 and sched.num_free_blocks() == pool
    err = (got - ref).abs().amax(-1)
    print("max |logit error| at positions 0, 8, 12, 23, 39:", [float(err[i]) for i in (0, 8, 12, 23, 39)])
    assert float(err.max()) < 1e-4


def test_prompt_longer_than_the_window_fails_loudly(mistral):
    _, _, cfg, w = mistral
    m = DecoderLM(cfg, w)
    kv = m.allocate_kv_cache(8, BS)
    n = W + 1
    inp = StepInput("prefill", torch.zeros(n, dtype=torch.long), torch.arange(n), torch.arange(n),
                    cu_seqlens=torch.tensor([0, n], dtype=torch.int32), max_seqlen=n, window=W)
    with pytest.raises(ValueError, match="window"):
        m(inp, kv)


def hf_greedy(hf, prompt, n):
    with torch.no_grad():
        return hf.generate(torch.tensor(prompt)[None], max_new_tokens=n, do_sample=False, pad_token_id=0,
                           eos_token_id=None)[0, len(prompt):].tolist()


def test_greedy_engine_matches_hf(mistral):
    _, hf, cfg, w = mistral
    eng = LLMEngine(DecoderLM(cfg, w), max_num_seqs=4, block_size=BS, num_blocks=64)
    assert eng.window == W
    torch.manual_seed(2)
    prompts = [torch.randint(0, VOCAB - 1, (n,)).tolist() for n in (3, 9, 30)]
    outs = eng.generate(prompts, SamplingParams(max_new_tokens=25, is_greedy=True, ignore_eos=True))
    for p, o in zip(prompts, outs):
        assert o == hf_greedy(hf, p, 25)
    assert eng.sched.num_free_blocks() == 64
    # three sequences of up to 55 tokens would hold 28 blocks; the window keeps every one of them at 5 or fewer
    assert 0 < eng.stats["peak_live_kv_blocks"] <= 3 * 5


def test_preemption_keeps_results(mistral):
    _, _, cfg, w = mistral
    m = DecoderLM(cfg, w)
    prompts = [[(7 * i + j) % 100 for j in range(10 + 3 * i)] for i in range(6)]
    sp = SamplingParams(max_new_tokens=20, is_greedy=True, ignore_eos=True)
    big = LLMEngine(m, max_num_seqs=8, block_size=BS, num_blocks=200).generate(prompts, sp)
    small_eng = LLMEngine(m, max_num_seqs=8, block_size=BS, num_blocks=14)  # forces preemption
    small = small_eng.generate(prompts, sp)
    assert small == big
    assert small_eng.stats["preemptions"] > 0
    assert small_eng.sched.num_free_blocks() == 14


def test_tp2_gloo_matches_tp1(mistral):
    from test_tp_gloo import _run

    path, _, cfg, w = mistral
    prompts = [[(5 * i + 3 * j) % 100 for j in range(n)] for i, n in enumerate((12, 20, 3))]  # two pass the window
    eng = LLMEngine(DecoderLM(cfg, w), max_num_seqs=4, block_size=4, num_blocks=64)
    ref_g = eng.generate(prompts, SamplingParams(max_new_tokens=8, is_greedy=True, ignore_eos=True))
    ref_s = eng.generate(prompts, [SamplingParams(max_new_tokens=8, temperature=0.9, top_k=20, top_p=0.9, seed=5 + i,
                                                  ignore_eos=True) for i in range(len(prompts))])
    g, s = _run(2, path, prompts)
    assert g == ref_g
    assert s == ref_s
