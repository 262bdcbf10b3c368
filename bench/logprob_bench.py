"""token_logprobs kernel time per call next to the sampler's on the same logits, in one process.

Rows: B = 64 and 512; V = 32000 and 50257 (row stride 50304); N = 0, 5 and 20. The sampler column is the engine's
default request (temperature 1, top-k 50, top-p 0.95) and greedy on the same bf16 rows: both kernels read each row
once from memory. ``partial+combine`` is the vocab-parallel pair over 8 column shards of the same rows.
One JSON line per measurement; ``--md`` prints the table of profiles/logprobs/README.md."""
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from llmss_amd.ops import hip as H  # noqa: E402

REPS = 20


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


def main():
    dev = torch.device("cuda", 0)
    rows = []
    for B in (64, 512):
        for V, ld in ((32000, 32000), (50257, 50304)):
            torch.manual_seed(0)
            logits = torch.randn(B, ld, device=dev).to(torch.bfloat16)
            seeds = torch.arange(B, dtype=torch.int64, device=dev)
            out = torch.empty(B, dtype=torch.int64, device=dev)
            rec = {"B": B, "V": V, "ld": ld}
            for mode, (t, k, p) in (("sample_greedy", (0.0, 1, 1.0)), ("sample_k50_p0.95", (1.0, 50, 0.95))):
                temp = torch.full((B,), t, device=dev)
                topk = torch.full((B,), k, dtype=torch.int32, device=dev)
                topp = torch.full((B,), p, device=dev)
                rec[mode] = timed(lambda: H.sample(logits, temp, topk, topp, seeds, vocab=V, out=out))
            for N in (0, 5, 20):
                outs = (torch.empty(B, device=dev), torch.empty(B, N, device=dev),
                        torch.empty(B, N, dtype=torch.int32, device=dev))
                rec[f"logprobs_N{N}"] = timed(lambda: H.token_logprobs(logits, V, out, N, out=outs))
                pack = torch.empty(B, 8 * (3 + 2 * N), device=dev)
                local = logits  # the padded row: 8 shards of ld / 8 columns
                rec[f"partial8+combine_N{N}"] = timed(lambda: H.token_logprobs_combine(
                    H.token_logprobs_partial(local, 0, V, out, N, shards=8, out=pack), N, out=outs))
            print(json.dumps(rec), flush=True)
            rows.append(rec)
    if "--md" in sys.argv:
        keys = [k for k in rows[0] if k not in ("B", "V", "ld")]
        print("| B | V (stride) | " + " | ".join(keys) + " |")
        print("|---|---|" + "---|" * len(keys))
        for r in rows:
            print(f"| {r['B']} | {r['V']} ({r['ld']}) | " + " | ".join(str(r[k]) for k in keys) + " |")


if __name__ == "__main__":
    main()
