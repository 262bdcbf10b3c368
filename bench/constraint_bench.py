"""apply_token_edits kernel time per call at batch 64 x 32,000 bf16 columns - no constrained rows, every row with an
8-entry list, every row with a 512-entry list, every row filled (an allowed set of 512) - next to ``Tensor.copy_`` of
the same [B, V], in one process. Every launch reads and writes the rows once, as the copy does; a constrained row also
reads its meta and list (at most 4 KiB). ``--tpot`` instead measures Llama-2-7B (random weights, bf16) batch-64 decode
TPOT with constraints off, on with default requests and on with every request constrained (the method of
bench/penalty_bench.py). One JSON line per measurement."""
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from llmss_amd.engine.sampling import MAX_TOKEN_EDITS, SamplingParams, resolve_token_edits  # noqa: E402
from llmss_amd.ops import hip as H  # noqa: E402
from llmss_amd.ops import reference as R  # noqa: E402

REPS = 20
B, V = 64, 32000
E = MAX_TOKEN_EDITS


def timed(f):
    """us per call: REPS calls captured in one HIP graph, minimum of 5 replays."""
    for _ in range(3):
        f()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, capture_error_mode="thread_local"):
        for _ in range(REPS):
            f()
    g.replay()
    torch.cuda.synchronize()
    best = float("inf")
    for _ in range(5):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        g.replay()
        e.record()
        e.synchronize()
        best = min(best, s.elapsed_time(e) / REPS * 1e3)
    return round(best, 2)


def _state(dev, params):
    """One slot per row, every row with the same request (tokens spread over the vocabulary)."""
    early, late, fill = resolve_token_edits(params, None, V)
    i, v, m = R.pack_token_edits(early, late, fill, params.min_tokens, E)
    rep = lambda a: torch.from_numpy(np.ascontiguousarray(np.broadcast_to(a, (B,) + a.shape))).to(dev)  # noqa: E731
    return rep(i), rep(v), rep(m)


def kernel():
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    logits = torch.randn(B, V, device=dev).to(torch.bfloat16)
    out = torch.empty_like(logits)
    nout = torch.zeros(B, dtype=torch.int32, device=dev)
    copy_us = timed(lambda: out.copy_(logits))
    print(json.dumps({"what": "copy_", "us": copy_us, "bytes": B * V * 4}), flush=True)
    spread = lambda n: [int(t) for t in np.linspace(0, V - 1, n).astype(np.int64)]  # noqa: E731
    cases = (("no_constrained_rows", SamplingParams(logit_bias={1: 1.0}), False),
             ("all_rows_8_entries", SamplingParams(logit_bias={t: -1.5 for t in spread(8)}), True),
             ("all_rows_512_entries", SamplingParams(logit_bias={t: -1.5 for t in spread(E)}), True),
             ("all_rows_filled_512_allowed", SamplingParams(allowed_token_ids=spread(E)), True))
    for name, params, held in cases:
        ids, vals, meta = _state(dev, params.validate())
        slots = torch.arange(B, dtype=torch.int32, device=dev) if held else \
            torch.full((B,), -1, dtype=torch.int32, device=dev)
        us = timed(lambda: H.apply_token_edits(logits, ids, vals, meta, slots, nout, 0, V, out))
        print(json.dumps({"what": f"apply_token_edits_{name}", "us": us, "vs_copy": round(us / copy_us, 2)}),
              flush=True)


def tpot():
    from llmss_amd.engine import LLMEngine
    from llmss_amd.models.config import get_preset
    from llmss_amd.models.decoder import DecoderLM
    from llmss_amd.models.weights import random_weights

    PROMPT, GEN = 128, 128
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    cfg = get_preset("llama2-7b")
    model = DecoderLM(cfg, random_weights(cfg, device=dev, dtype=torch.bfloat16, seed=0))
    g = torch.Generator().manual_seed(0)
    prompts = [torch.randint(0, cfg.vocab_size, (PROMPT,), generator=g).tolist() for _ in range(B)]

    def run(eng, con):
        for i, p in enumerate(prompts):
            eng.add_request(p, SamplingParams(max_new_tokens=GEN, temperature=1.0, top_p=0.95, top_k=50,
                                              ignore_eos=True, seed=7 + i, **con))
        done = []
        t0 = time.perf_counter()
        while eng.has_unfinished():
            eng.step()
            done += eng.pop_finished()
        wall = time.perf_counter() - t0
        assert all(len(r.output_ids) == GEN for r in done)
        return {"tok_s": round(B * GEN / wall, 1),
                "p50_tpot_ms": round(statistics.median(r.metrics()["tpot_s"] for r in done) * 1e3, 3)}

    real = dict(logit_bias={t: -1.5 for t in range(0, 32000, 500)}, banned_token_ids=list(range(7, 32000, 250)),
                min_tokens=16)  # 64 biases and 128 banned tokens per request; EOS is ignored, so every run is GEN long
    for name, on, con in (("off", False, {}), ("on_default_requests", True, {}), ("on_all_constrained", True, real)):
        eng = LLMEngine(model, max_num_seqs=B, use_graphs=True, constraints=on)
        run(eng, con)  # warm-up
        for i in range(3):
            print(json.dumps({"constraints": name, "run": i, **run(eng, con)}), flush=True)
        del eng
        torch.cuda.empty_cache()


if __name__ == "__main__":
    tpot() if "--tpot" in sys.argv else kernel()
