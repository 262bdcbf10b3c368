"""Decode TPOT of Llama-2-7B (random weights, bf16, one GPU) at batch 64 with ``max_logprobs=5`` against ``0``, in
one process: the cost of the log-probability launch, its two device-to-host copies and the host bookkeeping per
decode step. Drives LLMEngine directly (128-token prompts, 128 generated tokens, the bench's sampling parameters)."""
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from llmss_amd.engine import LLMEngine, SamplingParams  # noqa: E402
from llmss_amd.models.config import get_preset  # noqa: E402
from llmss_amd.models.decoder import DecoderLM  # noqa: E402
from llmss_amd.models.weights import random_weights  # noqa: E402

B, PROMPT, GEN = 64, 128, 128


def run(eng, prompts, n):
    sps = [SamplingParams(max_new_tokens=GEN, temperature=1.0, top_p=0.95, top_k=50, ignore_eos=True, seed=7 + i,
                          logprobs=n) for i in range(len(prompts))]
    for p, sp in zip(prompts, sps):
        eng.add_request(p, sp)
    done = []
    t0 = time.perf_counter()
    while eng.has_unfinished():
        eng.step()
        done += eng.pop_finished()
    wall = time.perf_counter() - t0
    tpot = [r.metrics()["tpot_s"] for r in done]
    assert all(len(r.output_ids) == GEN for r in done)
    assert n is None or all(len(r.output_logprobs) == GEN for r in done)
    return {"tok_s": round(B * GEN / wall, 1), "p50_tpot_ms": round(statistics.median(tpot) * 1e3, 3)}


def main():
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    cfg = get_preset("llama2-7b")
    model = DecoderLM(cfg, random_weights(cfg, device=dev, dtype=torch.bfloat16, seed=0))
    g = torch.Generator().manual_seed(0)
    prompts = [torch.randint(0, cfg.vocab_size, (PROMPT,), generator=g).tolist() for _ in range(B)]
    for N in (0, 5):
        eng = LLMEngine(model, max_num_seqs=B, use_graphs=True, max_logprobs=N)
        n = N or None
        run(eng, prompts, n)  # warm-up
        for i in range(3):
            print(json.dumps({"max_logprobs": N, "run": i, **run(eng, prompts, n)}), flush=True)
        del eng
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
