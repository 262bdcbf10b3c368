"""Offline tensor-parallel generation CLI (API-compatible with the reference ``generate.py``).

Same flags, defaults, validation and the same three stdout lines as the reference
(``generate.py:21-40,192-196``); launched with ``torchrun --nproc_per_node N generate.py ...``
(one rank per GPU, RCCL) or plain ``python generate.py ...`` (TP=1, GPU or CPU).

Deliberate fixes: TP=1 works (Q2); temperature/top-k/top-p are actually applied
(Q1); prompts are not padded, each sequence has its own length and positions (Q3); load time and
generation throughput are reported on extra lines after the original three (Q12).
``--use_cache`` absent keeps the reference's recompute mode (the whole prefix is re-run every
token, generate.py:146-190) over the same kernels.
"""
from __future__ import annotations

import json
import os
import sys
import time
from argparse import ArgumentParser

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def get_args(argv=None):
    parser = ArgumentParser()
    parser.add_argument("--pretrained_model_path", type=str, required=True)
    parser.add_argument("--prompts", type=str, nargs="+", required=True)
    parser.add_argument("--max_new_tokens", type=int, default=20)
    parser.add_argument("--is_greedy", action="store_true")
    parser.add_argument("--temperature", type=float, default=1.0, help="If you don't wanna use this, set to 1.0")
    parser.add_argument("--top_p", type=float, default=0.95, help="If you don't wanna use this, set to 1.0")
    parser.add_argument("--top_k", type=int, default=50, help="If you don't wanna use this, set to 0")
    parser.add_argument("--use_cache", action="store_true")
    # additions
    parser.add_argument("--dtype", type=str, default=None, help="bf16 (GPU default) | fp32 (CPU default)")
    parser.add_argument("--fp8", action="store_true", help="fp8-e4m3 weights (per-channel scales)")
    parser.add_argument("--seed", type=int, default=None)
    parser.add_argument("--device", type=str, default=None, help="cuda | cpu (default: cuda if available)")
    parser.add_argument("--json_metrics", action="store_true")
    parser.add_argument("--logprobs", type=int, default=None,
                        help="print, per generated token, its log-probability under the raw model distribution and the "
                             "N most likely tokens (0..20; 0: the token's alone)")
    parser.add_argument("--repetition_penalty", type=float, default=1.0,
                        help="> 0: the logit x of a token seen in the prompt or the output becomes x / r (x > 0) or x * r")
    parser.add_argument("--presence_penalty", type=float, default=0.0,
                        help="[-2, 2]: subtracted from the logit of every token generated so far")
    parser.add_argument("--frequency_penalty", type=float, default=0.0,
                        help="[-2, 2]: subtracted once per occurrence among the generated tokens")
    parser.add_argument("--logit_bias", type=str, default=None,
                        help='JSON object of token id -> bias in [-100, 100] added to its logit, e.g. \'{"50256": -100}\'')
    parser.add_argument("--banned_token_ids", type=int, nargs="+", default=[], help="token ids that are never sampled")
    parser.add_argument("--allowed_token_ids", type=int, nargs="+", default=[],
                        help="the only token ids that are sampled")
    parser.add_argument("--min_tokens", type=int, default=0,
                        help="EOS is not sampled before this many tokens were generated")
    parser.add_argument("--min_p", type=float, default=0.0,
                        help="[0, 1]: after top-k and top-p, keep only tokens at least this likely relative to the most "
                             "likely one (0: off)")
    return parser.parse_args(argv)


def recompute_generate(model, prompts, params, eos, lp_out=None):
    """Reference no-cache mode: every step re-runs the full prefix of every sequence. ``lp_out`` (one list per
    prompt, with params.logprobs set): receives each generated token's (log-probability, [(id, log-probability)])."""
    from llmss_amd import ops
    from llmss_amd.engine.sampling import step_seed
    from llmss_amd.models.decoder import StepInput

    dev = model.device
    seqs = [list(p) for p in prompts]
    outs = [[] for _ in prompts]
    done = [False] * len(prompts)
    nokv = [(None, None)] * model.cfg.num_layers
    maxlen = model.cfg.max_position_embeddings
    V = model.cfg.vocab_size
    state = None
    if params.has_penalties and model.dtype not in (torch.bfloat16, torch.float32):
        raise ValueError(f"penalties need bfloat16 or float32 logits (--dtype bf16 | fp32), the model computes "
                         f"{model.dtype}")
    if params.has_penalties:  # one state row per prompt: its tokens flagged now, every generated token counted below
        state = torch.zeros(len(prompts), V, dtype=torch.int32, device=dev)
        words = [ops.penalty_words(p, []) for p in prompts]
        cu = [0]
        for t, _ in words:
            cu.append(cu[-1] + t.size)
        ops.penalty_reset(state, torch.arange(len(prompts), dtype=torch.int32, device=dev),
                          torch.tensor(cu, dtype=torch.int32, device=dev),
                          *(torch.cat([torch.from_numpy(w[k]) for w in words]).to(dev) for k in (0, 1)))
    edits = None
    if params.has_constraints:  # every prompt has the same constraints: one slot
        from llmss_amd.engine.sampling import MAX_TOKEN_EDITS, resolve_token_edits

        if model.dtype not in (torch.bfloat16, torch.float32):
            raise ValueError(f"token constraints need bfloat16 or float32 logits (--dtype bf16 | fp32), the model "
                             f"computes {model.dtype}")
        early, late, fill = resolve_token_edits(params, eos, V)
        edits = [torch.from_numpy(a).unsqueeze(0).to(dev)
                 for a in ops.pack_token_edits(early, late, fill, params.min_tokens, MAX_TOKEN_EDITS)]
    for step in range(params.max_new_tokens):
        live = [i for i in range(len(seqs)) if not done[i]]
        if not live:
            break
        cur = [seqs[i][-maxlen:] for i in live]  # sliding window like the reference (generate.py:176-178)
        lens = [len(c) for c in cur]
        ids = torch.tensor([t for c in cur for t in c], dtype=torch.int64, device=dev)
        pos = torch.cat([torch.arange(n, dtype=torch.int64) for n in lens]).to(dev)
        cu = torch.tensor([0] + list(torch.tensor(lens).cumsum(0).tolist()), dtype=torch.int32, device=dev)
        inp = StepInput("prefill", ids, pos, torch.full_like(pos, -1), cu_seqlens=cu, max_seqlen=max(lens),
                        last_idx=(cu[1:] - 1).to(torch.int64))
        logits = model(inp, nokv)
        n = len(live)
        temp = torch.full((n,), params.k_temperature, dtype=torch.float32, device=dev)
        topk = torch.full((n,), params.k_top_k, dtype=torch.int32, device=dev)
        topp = torch.full((n,), params.k_top_p, dtype=torch.float32, device=dev)
        seeds = torch.tensor([step_seed(params.resolved_seed() + i, step) for i in live], dtype=torch.int64, device=dev)
        plogits = logits
        if state is not None:  # register each sequence's previous token, then penalise (log-probabilities stay raw)
            pen = (torch.full((n,), v, dtype=torch.float32, device=dev) for v in
                   (params.repetition_penalty, params.presence_penalty, params.frequency_penalty))
            plogits = ops.apply_penalties(logits, state, torch.tensor(live, dtype=torch.int32, device=dev),
                                          torch.tensor([outs[i][-1] if outs[i] else -1 for i in live], device=dev),
                                          *pen, 0, V)
        if edits is not None:  # after the penalties, before the sampler
            plogits = ops.apply_token_edits(plogits, *edits, torch.zeros(n, dtype=torch.int32, device=dev),
                                            torch.tensor([len(outs[i]) for i in live], dtype=torch.int32, device=dev),
                                            0, V)
        lnmp = torch.full((n,), params.k_ln_min_p, dtype=torch.float32, device=dev) if params.has_min_p else None
        tok = ops.sample(plogits, temp, topk, topp, seeds, vocab=model.cfg.vocab_size, ln_min_p=lnmp)
        if lp_out is not None:
            nlp = params.logprobs
            lp, top, tids = (x.cpu().tolist() for x in ops.token_logprobs(logits, model.cfg.vocab_size, tok, nlp))
            for j, i in enumerate(live):
                lp_out[i].append((lp[j], [(a, b) for a, b in zip(tids[j], top[j]) if a >= 0]))
        tok = tok.tolist()
        for i, t in zip(live, tok):
            seqs[i].append(t)
            outs[i].append(t)
            if eos is not None and t == eos:
                done[i] = True
    return outs


def main(argv=None):
    args = get_args(argv)
    assert args.max_new_tokens > 0, "Value of max_new_tokens should be over than 0."
    assert 0.0 < args.temperature <= 1.0, "Value of temperature is not valid."
    assert 0.0 < args.top_p <= 1.0, "Value of top_p is not valid."
    assert args.top_k >= 0, "Value of top_k is not valid."
    assert args.logprobs is None or 0 <= args.logprobs <= 20, "Value of logprobs is not valid."
    assert 0.0 < args.repetition_penalty < float("inf"), "Value of repetition_penalty is not valid."
    assert -2.0 <= args.presence_penalty <= 2.0, "Value of presence_penalty is not valid."
    assert -2.0 <= args.frequency_penalty <= 2.0, "Value of frequency_penalty is not valid."
    logit_bias = json.loads(args.logit_bias) if args.logit_bias else {}
    assert isinstance(logit_bias, dict), "Value of logit_bias should be a JSON object."
    logit_bias = {int(k): float(v) for k, v in logit_bias.items()}  # JSON object keys are strings
    assert 0 <= args.min_tokens <= args.max_new_tokens, "Value of min_tokens is not valid."
    assert 0.0 <= args.min_p <= 1.0, "Value of min_p is not valid."

    from llmss_amd.engine import LLMEngine, SamplingParams, build_model
    from llmss_amd.parallel.dist import initialize_distributed
    from llmss_amd.utils.tokenizer import encode, load_tokenizer

    tp, rank, world_size = initialize_distributed()
    start_time = time.time()
    if args.device:
        device = torch.device(args.device if args.device != "cuda" else f"cuda:{torch.cuda.current_device()}")
    else:
        device = torch.device("cuda", torch.cuda.current_device()) if torch.cuda.is_available() else torch.device("cpu")
    dtype = args.dtype or ("bf16" if device.type == "cuda" else "fp32")
    tp.barrier()
    model = build_model(args.pretrained_model_path, tp, dtype, device, fp8=args.fp8)
    tokenizer = load_tokenizer(args.pretrained_model_path, model.cfg.vocab_size)
    load_done = time.time()

    seed = args.seed
    if seed is None:  # one seed for all ranks so they sample identically
        seed = tp.broadcast_object(int.from_bytes(os.urandom(4), "little") if rank == 0 else None)
    params = SamplingParams(max_new_tokens=args.max_new_tokens, is_greedy=args.is_greedy,
                            temperature=args.temperature, top_p=args.top_p, top_k=args.top_k, seed=seed,
                            logprobs=args.logprobs, repetition_penalty=args.repetition_penalty,
                            presence_penalty=args.presence_penalty, frequency_penalty=args.frequency_penalty,
                            logit_bias=logit_bias, banned_token_ids=args.banned_token_ids,
                            allowed_token_ids=args.allowed_token_ids, min_tokens=args.min_tokens,
                            min_p=args.min_p).validate()
    eos = getattr(tokenizer, "eos_token_id", None)
    prompts = [encode(tokenizer, p) for p in args.prompts]
    max_len = model.cfg.max_position_embeddings
    prompts = [p[-max(1, max_len - 1):] for p in prompts]  # left truncation (reference tokenizer settings)

    t0 = time.time()
    if args.use_cache:
        engine = LLMEngine(model, max_num_seqs=max(1, len(prompts)), eos_token_id=eos,
                           # --logprobs 0 still needs the kernel, hence an engine with N >= 1
                           max_logprobs=0 if args.logprobs is None else max(1, args.logprobs),
                           # the states only when a flag differs from its default
                           penalties=params.has_penalties, constraints=params.has_constraints,
                           min_p=params.has_min_p)
        per = [SamplingParams(**{**params.__dict__, "seed": seed + i}) for i in range(len(prompts))]
        if args.logprobs is None:
            outputs = engine.generate(prompts, per)
        else:  # the engine's own loop, keeping the finished requests for their log-probabilities
            rids = [engine.add_request(p, sp) for p, sp in zip(prompts, per)]
            fin = {}
            while engine.has_unfinished():
                engine.step()
                fin.update((r.id, r) for r in engine.pop_finished())
            outputs = [fin[i].output_ids for i in rids]
            logprobs = [list(zip(fin[i].output_logprobs, fin[i].output_top_logprobs)) for i in rids]
    else:
        logprobs = [[] for _ in prompts] if args.logprobs is not None else None
        outputs = recompute_generate(model, prompts, params, eos, lp_out=logprobs)
    gen_s = time.time() - t0

    if rank == 0:
        end_time = time.time()
        print(f"elapsed time: {end_time - start_time}")
        print(f"prompts: {args.prompts}")
        print(f"continuations: {[tokenizer.decode(o) for o in outputs]}")
        n = sum(len(o) for o in outputs)
        print(f"load time: {load_done - start_time:.3f} s, generation: {gen_s:.3f} s, "
              f"{n} tokens, {n / max(gen_s, 1e-9):.1f} tokens/s (tp={world_size}, {device.type}, {dtype})")
        if args.logprobs is not None:  # one line per generated token, after the lines above
            for p, (out, lps) in enumerate(zip(outputs, logprobs)):
                for t, (tok, (lp, top)) in enumerate(zip(out, lps)):
                    print("logprobs: " + json.dumps({
                        "prompt": p, "position": t, "token_id": tok, "text": tokenizer.decode([tok]), "logprob": lp,
                        "top": [[i, tokenizer.decode([i]), v] for i, v in top]}, ensure_ascii=False))
        if args.json_metrics:
            print(json.dumps({"load_s": load_done - start_time, "generate_s": gen_s, "tokens": n,
                              "tokens_per_s": n / max(gen_s, 1e-9), "tp": world_size}))
    return outputs


if __name__ == "__main__":
    main()
