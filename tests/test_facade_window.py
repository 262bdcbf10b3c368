"""The reference caller's KV window on the façade (models/registry.py): ``PagedPast.truncate`` keeps the last k keys at
any token boundary, returns wholly dropped blocks to the pool and continues at position = kept length, as the
reference loop does with its torch.cat cache (generate.py:99-145: ``past[..., -(n_positions - 1):, :]``); positions
past the wpe / RoPE table raise; a windowed model (Mistral) applies its window through the façade too."""
import pytest
import torch
from transformers import AutoConfig

from helpers import save_hf_model


def _load(d, block_size=4, max_blocks=64):
    from llmss.server.models.custom_modeling import MODEL_REGISTRY
    from llmss.server.models.utils.hub import weight_files
    from llmss.server.models.utils.weights import Weights

    config = AutoConfig.from_pretrained(d)
    w = Weights(weight_files(d), torch.device("cpu"), torch.float32, None)
    return MODEL_REGISTRY[config.model_type](config, w, max_blocks=max_blocks, block_size=block_size)


@pytest.fixture(scope="module")
def gptj(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("gptj"))
    hf = save_hf_model("gptj", d)  # n_positions = 64
    return d, hf


def test_truncate_that_drops_nothing_changes_nothing(gptj):
    d, _ = gptj
    ids = torch.randint(0, 100, (2, 11))
    outs = []
    for cut in (False, True):
        model = _load(d)
        past = model(ids[:, :7], use_cache=True).past_key_values
        free = len(model._free)
        if cut:
            assert past.truncate(7) is past and past.truncate(100) is past
            assert len(model._free) == free and past.offs == [0, 0] and past.lens == [7, 7]
        outs.append(model(ids[:, 7:], past_key_values=past, use_cache=True).logits)
    assert torch.equal(outs[0], outs[1])


def test_truncate_returns_blocks_and_continues_at_the_kept_length(gptj):
    d, hf = gptj
    model = _load(d)  # pages of 4 tokens
    ids = torch.randint(0, 100, (1, 23))
    past = model(ids[:, :22], use_cache=True).past_key_values
    free = len(model._free)
    held = list(past.blocks[0])
    past.truncate(9)  # keys 13 .. 21: pages 0 - 2 go back whole, page 3 is cut after its first key
    assert past.lens == [9] and past.offs == [1] and past.blocks[0] == held[3:]
    assert len(model._free) == free + 3 and set(held[:3]) <= set(model._free)
    out = model(ids[:, 22:], past_key_values=past, use_cache=True)
    # HF with its cache sliced the same way: the new token sits at position 9 (the kept length)
    from transformers import DynamicCache

    with torch.no_grad():
        c = hf(ids[:, :22], use_cache=True).past_key_values
        kv = [(layer.keys[:, :, -9:], layer.values[:, :, -9:]) for layer in c.layers]
        ref = hf(ids[:, 22:], past_key_values=DynamicCache(kv), use_cache=True).logits
    assert float((out.logits - ref).abs().max()) < 1e-4
    # ... which is what explicit position ids say as well
    model2 = _load(d)
    past2 = model2(ids[:, :22], use_cache=True).past_key_values.truncate(9)
    explicit = model2(ids[:, 22:], past_key_values=past2, use_cache=True, position_ids=torch.tensor([[9]])).logits
    assert torch.equal(explicit, out.logits)
    model.release(out.past_key_values)
    assert len(model._free) == 64
    # truncate(0) forgets the row
    model3 = _load(d)
    past3 = model3(ids[:, :10], use_cache=True).past_key_values.truncate(0)
    assert past3.lens == [0] and past3.blocks == [[]] and len(model3._free) == 64


def test_positions_outside_the_table_raise(gptj):
    d, _ = gptj
    model = _load(d)
    ids = torch.randint(0, 100, (1, 64))
    past = model(ids, use_cache=True).past_key_values  # positions 0 .. 63: the whole table
    free = len(model._free)
    with pytest.raises(ValueError, match="position 64"):
        model(ids[:, :1], past_key_values=past, use_cache=True)
    with pytest.raises(ValueError, match="position"):
        model(ids[:, :1], past_key_values=past, use_cache=True, position_ids=torch.tensor([[-1]]))
    assert len(model._free) == free and past.lens == [64]  # nothing allocated, nothing cached
    with pytest.raises(ValueError, match="position 70"):
        model(ids[:, :3], position_ids=torch.tensor([[0, 1, 70]]))
    past.truncate(63)
    model(ids[:, :1], past_key_values=past, use_cache=True)  # position 63
    gpt2_d = d + "-gpt2"
    save_hf_model("gpt2", gpt2_d)  # learned positions: the wpe table, 64 rows
    m2 = _load(gpt2_d)
    with pytest.raises(ValueError, match="position 64"):
        m2(torch.randint(0, 100, (1, 65)))


def test_reference_loop_with_a_kv_window(gptj):
    """The reference loop's shape (generate.py:99-145) for 80 steps on tiny GPT-J (n_positions = 64): once the cache
    holds n_positions entries it is cut to the last n_positions - 1. Oracle: HF GPT-J stepped the same way, its
    per-layer K / V sliced to the last 63 entries and handed back as a DynamicCache. Tokens are teacher-forced so
    every step's logits compare; 1e-4 is the project's fp32 bound. The page size 4 does not divide 63: the cut
    falls inside a page on most steps."""
    from transformers import DynamicCache

    d, hf = gptj
    n_pos = 64
    model = _load(d, block_size=4, max_blocks=20)  # 17 blocks hold 64 keys + the cut page: nothing may leak
    torch.manual_seed(5)
    prompt = torch.randint(0, 100, (1, 5))
    stream = torch.randint(0, 100, (80,))
    ids, past, hf_past, worst = prompt, None, None, 0.0
    for step in range(80):
        out = model(ids, past_key_values=past, use_cache=True)
        with torch.no_grad():
            ref = hf(ids, past_key_values=hf_past, use_cache=True)
        worst = max(worst, float((out.logits[:, -1] - ref.logits[:, -1]).abs().max()))
        past, hf_past = out.past_key_values, ref.past_key_values
        if past.lens[0] > n_pos - 1:
            past.truncate(n_pos - 1)
            hf_past = DynamicCache([(layer.keys[:, :, -(n_pos - 1):], layer.values[:, :, -(n_pos - 1):])
                                    for layer in hf_past.layers])
        assert past.lens[0] == hf_past.get_seq_length() <= n_pos - 1
        assert len(past.blocks[0]) <= 17 and len(model._free) + len(past.blocks[0]) == 20
        ids = stream[step].view(1, 1)
    assert past.lens[0] == n_pos - 1 and past.offs[0] != 0
    print(f"80 steps, worst |logit error| {worst:.3g}")
    assert worst < 1e-4


def test_windowed_model_through_the_facade(tmp_path):
    """A Mistral checkpoint (sliding_window = 8) through MODEL_REGISTRY: a prompt in calls of at most 8 tokens, then
    single tokens, against HF's eager attention; a longer call fails loudly."""
    from transformers import MistralConfig, MistralForCausalLM

    torch.manual_seed(0)
    hf = MistralForCausalLM(MistralConfig(hidden_size=64, num_hidden_layers=2, num_attention_heads=4,
                                          num_key_value_heads=2, intermediate_size=160, vocab_size=101,
                                          max_position_embeddings=64, sliding_window=8,
                                          attn_implementation="eager")).eval()
    d = str(tmp_path / "mistral")
    hf.save_pretrained(d, safe_serialization=True)
    model = _load(d)
    assert type(model).__name__ == "MistralForCausalLM" and model.config.sliding_window == 8
    ids = torch.randint(0, 100, (2, 30))
    with torch.no_grad():
        ref = hf(ids).logits
    past, got = None, []
    for a, e in ((0, 8), (8, 13), (13, 21), (21, 22), (22, 23), (23, 30)):
        out = model(ids[:, a:e], past_key_values=past, use_cache=True)
        past = out.past_key_values
        got.append(out.logits)
    assert float((torch.cat(got, 1) - ref).abs().max()) < 1e-4
    with pytest.raises(ValueError, match="window"):
        model(ids[:, :9])
