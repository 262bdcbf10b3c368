"""The engine on packed decode plans: a tiny Llama (head dim 64) with the plans of qkv (plain and fused-epilogue), o,
gate/up, down and the head forced through gemm_tuned_set, once with the packed bit and once on the row-major siblings.
Greedy tokens must be equal, eagerly and from HIP graphs. 8 requests on 4 sequence slots: the second four are prefilled
after decode steps of the first four, on the row-major weights."""
import pytest
import torch

from llmss_amd.engine import LLMEngine, SamplingParams
from llmss_amd.models.config import get_preset
from llmss_amd.models.decoder import DecoderLM
from llmss_amd.models.weights import random_weights
from llmss_amd.ops import hip as H

pytestmark = pytest.mark.gpu

DEC, PK = 1024, H.PACKED_HINT
# projection -> (kind, nt_hint, split): gemm_dec and gemm_mid tiles, unsplit, fp32 slabs for rope / add_norm, SwiGLU
PLANS = {
    "qkv": [(0, (2 | 32 | DEC) << 8, 2), (3, (4 | 32 | DEC) << 8, 1)],
    "o": [(0, (15 | 16) << 8, 2)],
    "up": [(0, (14 | 32) << 8, 1)],
    "down": [(0, (3 | 32 | DEC) << 8, 2)],
    "head": [(0, (7 | 32) << 8, 1)],
}
SP = SamplingParams(max_new_tokens=16, is_greedy=True, ignore_eos=True)


@pytest.fixture(scope="module")
def setup():
    cfg = get_preset("tiny-llama", hidden_size=256, num_heads=4, num_kv_heads=2, head_dim=64, rotary_dim=64,
                     intermediate_size=512, max_position_embeddings=256)
    w = random_weights(cfg, device="cuda", dtype=torch.bfloat16, seed=3, std=0.05)
    g = torch.Generator().manual_seed(11)
    prompts = [[int(x) for x in torch.randint(0, cfg.vocab_size, (n,), generator=g)] for n in (5, 40, 33, 21, 60, 2, 17, 30)]
    return cfg, w, prompts


def _linears(w):
    L = w.layers[0]
    return {"qkv": L.qkv, "o": L.o, "up": L.up, "down": L.down, "head": w.head}


def _force(w, packed):
    """Install the plans for every row count up to 8; returns what to pass to _restore."""
    lib = H.lib()
    saved = []
    for name, lin in _linears(w).items():
        for kind, nt, s in PLANS[name]:
            for M in range(1, 9):
                key = (M, lin.N, lin.K, bool(lin.glu), kind)
                saved.append((key, lib.gemm_tuned_get(*key)))
                lib.gemm_tuned_set(*key, nt | (PK if packed else 0), s)
    return saved


def _restore(saved):
    for key, prev in saved:
        H.lib().gemm_tuned_set(*key, *(prev or (0, 0)))


def _tokens(cfg, w, prompts, packed, graphs):
    saved = _force(w, packed)
    try:
        eng = LLMEngine(DecoderLM(cfg, w), max_num_seqs=4, block_size=16, num_blocks=64, use_graphs=graphs,
                        autotune=False)
        assert bool(eng.graphs) == graphs
        out = eng.generate(prompts, SP)
        return out, eng.stats
    finally:
        _restore(saved)


@pytest.mark.parametrize("graphs", [False, True], ids=["eager", "graphs"])
def test_packed_plans_give_the_row_major_tokens(setup, graphs):
    cfg, w, prompts = setup
    for lin in [l for L in w.layers for l in (L.qkv, L.o, L.up, L.down)] + [w.head]:
        lin.w_packed = None
    want, st0 = _tokens(cfg, w, prompts, False, graphs)
    assert st0["packed_weight_bytes"] == 0 and all(l.w_packed is None for l in _linears(w).values())
    got, st1 = _tokens(cfg, w, prompts, True, graphs)
    lins = [l for L in w.layers for l in (L.qkv, L.o, L.up, L.down)] + [w.head]
    assert all(l.w_packed is not None for l in lins)
    assert st1["packed_weight_bytes"] == sum(l.w_packed.numel() * 2 for l in lins) > 0
    assert st1["prefill_steps"] >= 2 and st1["decode_steps"] > 16  # the second four were prefilled between decodes
    assert all(len(o) == 16 for o in got)
    assert got == want
