"""Sampler kernel time per call (B rows) by vocab, logit spread and sampling mode. The modes without ``+`` launch
without a min-p lane (the kernels as they are without the feature); ``+lane_off`` runs the same rows through the MINP
kernel variants with an all -inf lane (no floor), ``+minp0.05`` with a floor of min_p = 0.05. ``sample_all`` is
temperature 1 with top-k 0 / top-p 1, the baseline of min-p alone. ``--tpot`` instead measures Llama-2-7B (random
weights, bf16) batch-64 decode TPOT with min_p off, on with default requests and on with every request at
min_p = 0.05 (the method of bench/constraint_bench.py). One JSON line per measurement."""
import json
import math
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from llmss_amd.ops import hip as H  # noqa: E402

MODES = ("greedy", "topk50_topp0.95", "topp0.95", "sample_all", "topk50_topp0.95+lane_off",
         "topk50_topp0.95+minp0.05", "sample_all+lane_off", "sample_all+minp0.05")


def main():
    dev = torch.device("cuda", 0)
    B = int(os.environ.get("B", "64"))
    for V in (32000, 50257, 50304):
        for spread in (0.5, 1.0, 5.0):
            logits = (torch.randn(B, V, device=dev) * spread).to(torch.bfloat16)
            for mode in MODES:
                temp = torch.full((B,), 0.0 if mode == "greedy" else 1.0, device=dev)
                topk = torch.full((B,), 50 if "topk" in mode else 0, dtype=torch.int32, device=dev)
                topp = torch.full((B,), 0.95 if "topp" in mode else 1.0, device=dev)
                seeds = torch.arange(B, dtype=torch.int64, device=dev)
                out = torch.empty(B, dtype=torch.int64, device=dev)
                lane = None
                if "+" in mode:
                    lane = torch.full((B,), math.log(0.05) if "minp" in mode else float("-inf"), device=dev)
                f = lambda: H.sample(logits, temp, topk, topp, seeds, vocab=V, out=out, ln_min_p=lane)  # noqa: E731
                for _ in range(3):
                    f()
                torch.cuda.synchronize()
                g = torch.cuda.CUDAGraph()
                with torch.cuda.graph(g, capture_error_mode="thread_local"):
                    for _ in range(20):
                        f()
                g.replay()
                torch.cuda.synchronize()
                s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                s.record()
                g.replay()
                e.record()
                e.synchronize()
                print(json.dumps({"B": B, "V": V, "spread": spread, "mode": mode,
                                  "us": round(s.elapsed_time(e) / 20 * 1e3, 2)}), flush=True)


def tpot():
    from llmss_amd.engine import LLMEngine, SamplingParams
    from llmss_amd.models.config import get_preset
    from llmss_amd.models.decoder import DecoderLM
    from llmss_amd.models.weights import random_weights

    B, PROMPT, GEN = 64, 128, 128
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    cfg = get_preset("llama2-7b")
    model = DecoderLM(cfg, random_weights(cfg, device=dev, dtype=torch.bfloat16, seed=0))
    g = torch.Generator().manual_seed(0)
    prompts = [torch.randint(0, cfg.vocab_size, (PROMPT,), generator=g).tolist() for _ in range(B)]

    def run(eng, min_p):
        for i, p in enumerate(prompts):
            eng.add_request(p, SamplingParams(max_new_tokens=GEN, temperature=1.0, top_p=0.95, top_k=50,
                                              ignore_eos=True, seed=7 + i, min_p=min_p))
        done = []
        t0 = time.perf_counter()
        while eng.has_unfinished():
            eng.step()
            done += eng.pop_finished()
        wall = time.perf_counter() - t0
        assert all(len(r.output_ids) == GEN for r in done)
        return {"tok_s": round(B * GEN / wall, 1),
                "p50_tpot_ms": round(statistics.median(r.metrics()["tpot_s"] for r in done) * 1e3, 3)}

    for name, on, min_p in (("off", False, 0.0), ("on_default_requests", True, 0.0), ("on_all_min_p_0.05", True, 0.05)):
        eng = LLMEngine(model, max_num_seqs=B, use_graphs=True, min_p=on)
        run(eng, min_p)  # warm-up
        for i in range(3):
            print(json.dumps({"min_p": name, "run": i, **run(eng, min_p)}), flush=True)
        del eng
        torch.cuda.empty_cache()


if __name__ == "__main__":
    tpot() if "--tpot" in sys.argv else main()
