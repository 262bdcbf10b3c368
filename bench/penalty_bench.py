"""apply_penalties kernel time per call at batch 64 x 32,000 bf16 columns with 0 %, 50 % and 100 % of the rows
penalised, next to ``Tensor.copy_`` of the same [B, V] and the sampler on the same rows, in one process. A copy row
moves 2 x 2 bytes per column, a penalised one also reads its 4-byte state word: ``bytes`` is what a launch moves and
``vs_copy_by_bytes`` its time over the copy's time scaled by bytes moved. ``--tpot`` instead measures Llama-2-7B
(random weights, bf16) batch-64 decode TPOT with penalties off, on with default requests and on with every request
penalised (the method of bench/logprob_tpot.py). One JSON line per measurement."""
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from llmss_amd.ops import hip as H  # noqa: E402

REPS = 20
B, V = 64, 32000


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


def kernel():
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    logits = torch.randn(B, V, device=dev).to(torch.bfloat16)
    out = torch.empty_like(logits)
    state = torch.zeros(256, V, dtype=torch.int32, device=dev)
    state[:, ::7] = -(1 << 31)  # bit 31: a seventh of the tokens seen in the prompt
    state[:, ::11] += 2
    rep = torch.full((B,), 1.3, device=dev)
    pres = torch.full((B,), 0.7, device=dev)
    freq = torch.full((B,), 0.45, device=dev)
    tok = torch.full((B,), -1, dtype=torch.int64, device=dev)  # nothing registered: every replay sees the same state
    copy_us = timed(lambda: out.copy_(logits))
    copy_bytes = B * V * 4
    print(json.dumps({"what": "copy_", "us": copy_us, "bytes": copy_bytes}), flush=True)
    seeds = torch.arange(B, dtype=torch.int64, device=dev)
    ids = torch.empty(B, dtype=torch.int64, device=dev)
    temp, topk, topp = torch.ones(B, device=dev), torch.full((B,), 50, dtype=torch.int32, device=dev), \
        torch.full((B,), 0.95, device=dev)
    print(json.dumps({"what": "sample_k50_p0.95",
                      "us": timed(lambda: H.sample(logits, temp, topk, topp, seeds, vocab=V, out=ids))}), flush=True)
    for pct in (0, 50, 100):
        slots = torch.arange(B, dtype=torch.int32, device=dev) * 3  # distinct rows of the state
        if pct == 0:
            slots.fill_(-1)
        elif pct == 50:
            slots[1::2] = -1
        n = int((slots >= 0).sum())
        us = timed(lambda: H.apply_penalties(logits, state, slots, tok, rep, pres, freq, 0, V, out))
        nbytes = copy_bytes + n * V * 4
        print(json.dumps({"what": f"apply_penalties_{pct}pct", "rows_penalised": n, "us": us, "bytes": nbytes,
                          "vs_copy_by_bytes": round(us / (copy_us * nbytes / copy_bytes), 2)}), flush=True)


def tpot():
    from llmss_amd.engine import LLMEngine, SamplingParams
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

    def run(eng, pen):
        for i, p in enumerate(prompts):
            eng.add_request(p, SamplingParams(max_new_tokens=GEN, temperature=1.0, top_p=0.95, top_k=50,
                                              ignore_eos=True, seed=7 + i, **pen))
        done = []
        t0 = time.perf_counter()
        while eng.has_unfinished():
            eng.step()
            done += eng.pop_finished()
        wall = time.perf_counter() - t0
        assert all(len(r.output_ids) == GEN for r in done)
        return {"tok_s": round(B * GEN / wall, 1),
                "p50_tpot_ms": round(statistics.median(r.metrics()["tpot_s"] for r in done) * 1e3, 3)}

    real = dict(repetition_penalty=1.3, presence_penalty=0.7, frequency_penalty=0.45)
    for name, on, pen in (("off", False, {}), ("on_default_requests", True, {}), ("on_all_penalised", True, real)):
        eng = LLMEngine(model, max_num_seqs=B, use_graphs=True, penalties=on)
        run(eng, pen)  # warm-up
        for i in range(3):
            print(json.dumps({"penalties": name, "run": i, **run(eng, pen)}), flush=True)
        del eng
        torch.cuda.empty_cache()


if __name__ == "__main__":
    tpot() if "--tpot" in sys.argv else kernel()
