"""min_p through the engine on the CPU (tiny Llama, fp32): every sampled token of a request with min_p = m at
temperature T satisfies (logit_tok - logit_max) / T >= ln m - 1e-4 on Hugging Face's logits for the same prefix -
penalised and constrained first where the request asks for it - while the same requests and seeds without min_p
violate it; min_p = 1 reproduces greedy decoding; a mixed batch gives each request the tokens it gets alone; the
same under chunked prefill, a preemption and TP=2 over gloo on both sampler routes; and the opt-in rules."""
import math
import os
import socket

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

import constraint_cases as C
import penalty_cases as P
from helpers import save_hf_model
from llmss_amd.engine import LLMEngine, SamplingParams
from llmss_amd.models.config import ModelConfig
from llmss_amd.models.decoder import DecoderLM
from llmss_amd.models.weights import load_hf_weights
from llmss_amd.utils.checkpoint import CheckpointReader, weight_files

SLACK = 1e-4  # nats, on fp32 logits against Hugging Face's
NEW = 16
M_FLOOR = 0.3  # the floor of the property tests; T_FLOOR and the seeds below make the runs without it violate it
T_FLOOR = 0.2  # the tiny model's logits span well under one nat: a low temperature spreads the scaled ones
PROMPTS = [[(3 * i + 7 * j) % 100 for j in range(5 + 2 * i)] for i in range(6)]


def sp(n=NEW, **kw):
    kw.setdefault("ignore_eos", True)
    kw.setdefault("top_k", 0)
    kw.setdefault("top_p", 1.0)
    return SamplingParams(max_new_tokens=n, **kw)


def floor_sps(m, extra=lambda i: {}):
    return [sp(temperature=T_FLOOR, seed=100 + i, min_p=m, **extra(i)) for i in range(len(PROMPTS))]


def run(eng, prompts, sps, late=None):
    """Requests (in submission order) of a run to completion; ``late`` = (steps, prompt, params) arrives mid-run."""
    rids = [eng.add_request(p, s) for p, s in zip(prompts, sps)]
    done, steps = {}, 0
    while eng.has_unfinished():
        eng.step()
        steps += 1
        if late and steps == late[0]:
            rids.append(eng.add_request(late[1], late[2]))
        for r in eng.pop_finished():
            done[r.id] = r
    for r in eng.pop_finished():
        done[r.id] = r
    return [done[i] for i in rids]


@pytest.fixture(scope="module")
def ckpt(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("llama"))
    return d, save_hf_model("llama", d)


def _engine(d, **kw):
    cfg = ModelConfig.from_pretrained(d)
    w = load_hf_weights(cfg, CheckpointReader(weight_files(d)), 1, 0, device="cpu", dtype=torch.float32)
    kw.setdefault("max_num_seqs", 8)
    kw.setdefault("num_blocks", 64)
    return LLMEngine(DecoderLM(cfg, w), block_size=4, **kw), cfg


def margins(reqs, hf, V, m, eos=None):
    """Per sampled token: (logit_tok - logit_max) / T - ln m on the Hugging Face logits of its prefix, the row
    penalised and constrained first as the request asks (the row the sampler sees). >= -SLACK: on or above the floor."""
    out = []
    for r in reqs:
        q = r.params
        with torch.no_grad():
            logits = hf(torch.tensor([r.prompt_ids + r.output_ids])).logits[0].double().numpy()
        for t, tok in enumerate(r.output_ids):
            row = logits[len(r.prompt_ids) - 1 + t, :V]
            if q.has_penalties:
                row = P.penalise_row(row, r.prompt_ids, r.output_ids[:t], q.repetition_penalty, q.presence_penalty,
                                     q.frequency_penalty)
            if q.has_constraints:
                row = C.constrain_row(row, q, eos, t)
            out.append((row[tok] - row.max()) / q.temperature - math.log(m))
    return np.array(out)


def without(sps):
    return [SamplingParams(**{**s.__dict__, "min_p": 0.0}) for s in sps]


def test_floor_respected_and_violated_without(ckpt):
    d, hf = ckpt
    on, cfg = _engine(d, min_p=True)
    sps = floor_sps(M_FLOOR)
    got = margins(run(on, PROMPTS, sps), hf, cfg.vocab_size, M_FLOOR)
    assert got.size == NEW * len(PROMPTS) and got.min() >= -SLACK, got.min()
    off, _ = _engine(d)
    plain = margins(run(off, PROMPTS, without(sps)), hf, cfg.vocab_size, M_FLOOR)
    print(f"margin to the floor: with min_p {got.min():.4f}, without {plain.min():.4f}; "
          f"{int((plain < -SLACK).sum())} of {plain.size} tokens below it without")
    assert (plain < -SLACK).sum() >= 1  # the same requests and seeds do leave the floor without the feature


def test_min_p_one_is_the_greedy_twin(ckpt):
    d, hf = ckpt
    on, cfg = _engine(d, min_p=True)
    greedy = run(on, PROMPTS, [sp(is_greedy=True) for _ in PROMPTS])
    twin = run(on, PROMPTS, [sp(temperature=1.0, seed=7 + i, min_p=1.0) for i in range(len(PROMPTS))])
    ties = 0
    for r, s in zip(greedy, twin):
        with torch.no_grad():
            logits = hf(torch.tensor([r.prompt_ids + r.output_ids])).logits[0, len(r.prompt_ids) - 1:-1]
        top = logits[:, :cfg.vocab_size].double().topk(2, dim=-1).values
        tie = np.flatnonzero(((top[:, 0] - top[:, 1]) <= SLACK).numpy())
        ties += tie.size
        # a position where the top two logits tie is not judged, nor what follows it in that request
        upto = int(tie[0]) if tie.size else NEW
        assert s.output_ids[:upto] == r.output_ids[:upto] and len(s.output_ids) == NEW
    print(f"{ties} of {NEW * len(PROMPTS)} positions have the top two logits within {SLACK}")
    assert ties < 0.02 * NEW * len(PROMPTS)


def test_mixed_batch_equals_solo_runs(ckpt):
    """min_p {0, 0.05, 0.3, 1.0}, unequal lengths (rows finish and are dropped at different steps) and a late arrival:
    every request's tokens are those of the same request run alone."""
    d, _ = ckpt
    ms, lens = [0.0, 0.05, 0.3, 1.0, 0.3], [16, 5, 11, 8, 13]
    sps = [sp(n=lens[i], temperature=T_FLOOR, seed=40 + i, min_p=ms[i]) for i in range(5)]
    on, _ = _engine(d, min_p=True)
    mixed = run(on, PROMPTS[:4], sps[:4], late=(3, PROMPTS[4], sps[4]))
    assert [len(r.output_ids) for r in mixed] == lens
    for i in range(5):
        solo, _ = _engine(d, min_p=True)
        alone = run(solo, [PROMPTS[i]], [SamplingParams(**sps[i].__dict__)])[0]
        assert alone.output_ids == mixed[i].output_ids, i
    # the floor is what parts them: rows 1-4 differ from their min_p = 0 runs
    off, _ = _engine(d)
    plain = run(off, PROMPTS[:4], without(sps[:4]))
    assert plain[0].output_ids == mixed[0].output_ids
    assert sum(plain[i].output_ids != mixed[i].output_ids for i in (1, 2, 3)) >= 2


@pytest.mark.parametrize("how", ["chunked", "preempt", "with_penalties_and_constraints"])
def test_floor_under(ckpt, how):
    d, hf = ckpt
    kw = {"chunked": dict(prefill_chunk=4), "preempt": dict(num_blocks=14, max_num_seqs=4),
          "with_penalties_and_constraints": dict(penalties=True, constraints=True)}[how]
    eng, cfg = _engine(d, min_p=True, **kw)
    extra = lambda i: {}  # noqa: E731
    if how == "with_penalties_and_constraints":
        extra = lambda i: dict(repetition_penalty=1.3, presence_penalty=0.5, frequency_penalty=0.25,  # noqa: E731
                               banned_token_ids=[(7 * i + 3) % 100, 11], logit_bias={5 + i: 2.0, 40: -1.5})
    sps = floor_sps(M_FLOOR, extra)
    reqs = run(eng, PROMPTS, sps)
    if how == "preempt":
        assert eng.stats["preemptions"] > 0
    assert all(len(r.output_ids) == NEW for r in reqs)
    got = margins(reqs, hf, cfg.vocab_size, M_FLOOR)
    assert got.min() >= -SLACK, got.min()
    if how == "with_penalties_and_constraints":
        for r in reqs:
            assert not set(r.params.banned_token_ids) & set(r.output_ids)
    else:  # the schedule changes nothing: the tokens of the plain min_p engine
        base, _ = _engine(d, min_p=True)
        assert [r.output_ids for r in reqs] == [r.output_ids for r in run(base, PROMPTS, floor_sps(M_FLOOR))]


def test_opt_in(ckpt):
    d, _ = ckpt
    off, _ = _engine(d)
    assert off.min_p is False and off.fingerprint()["min_p"] is False
    for bad in (0.05, 1.0, 1):
        with pytest.raises(ValueError, match="min_p=True"):
            off.add_request([1, 2, 3], sp(n=2, min_p=bad))
    with pytest.raises(ValueError, match="finite number in"):
        off.add_request([1, 2, 3], sp(n=2, min_p=1.5))
    assert not off.has_unfinished() and not off.requests  # the rejected requests left nothing behind
    on, _ = _engine(d, min_p=True)
    fp_on, fp_off = on.fingerprint(), off.fingerprint()
    assert fp_on["min_p"] is True and {k: v for k, v in fp_on.items() if k != "min_p"} == \
        {k: v for k, v in fp_off.items() if k != "min_p"}
    with pytest.raises(ValueError):
        on.add_request([1, 2, 3], sp(n=2, min_p=float("nan")))
    assert not on.requests
    # default requests: the plain engine's tokens, sampled and greedy
    sps = [sp(temperature=0.9, top_k=20, top_p=0.9, seed=5 + i) for i in range(3)] + [sp(is_greedy=True)]
    a = run(off, PROMPTS[:4], sps)
    b = run(on, PROMPTS[:4], [SamplingParams(**s.__dict__) for s in sps])
    assert [r.output_ids for r in a] == [r.output_ids for r in b]
    # greedy requests ignore min_p
    g = run(on, PROMPTS[3:4], [sp(is_greedy=True, min_p=0.5)])[0]
    assert g.output_ids == a[3].output_ids


def test_staging_blob_layout():
    """The lane is the last fp32 section of the staging blob; no other offset moves, with or without penalties."""
    from llmss_amd.engine.engine import _DecodeBuffers

    dev = torch.device("cpu")
    for pen in (False, True):
        for con in (False, True):
            a = _DecodeBuffers(8, 4, dev, 0, pen, con)
            b = _DecodeBuffers(8, 4, dev, 0, pen, con, True)
            assert (a.o32, a.of32) == (b.o32, b.of32) and b.d.numel() == a.d.numel() + 8 * 4 and a.lnmp is None
            assert b.lnmp.data_ptr() == b.d.data_ptr() + a.d.numel()
            for name in ("ids", "pos", "slots", "seeds", "ctx", "topk", "bt", "temp", "topp") + \
                    (("pslot", "rep", "pres", "freq") if pen else ()) + (("cslot", "cnout") if con else ()):
                assert getattr(a, name).data_ptr() - a.d.data_ptr() == getattr(b, name).data_ptr() - b.d.data_ptr()
            n = 3
            z = np.zeros(n, dtype=np.int64)
            b.fill(0, 8, z, z, z, z, z.astype(np.int32), z.astype(np.int32), np.zeros((n, 4), np.int32),
                   np.ones(n, np.float32), np.ones(n, np.float32), lnmp=np.array([-1.0, -np.inf, 0.0], np.float32))
            assert b.lnmp.tolist() == [-1.0, -math.inf, 0.0] + [-math.inf] * 5  # pad rows: no floor


# ---------------------------------------------------------------------------------------- TP=2 over gloo
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _tp_runs():
    """Rows the vocab-parallel candidate sampler takes (top-k <= 64), then a batch with an unrestricted row, which
    goes through the gathered logits; penalties and constraints ride along."""
    extra = dict(repetition_penalty=1.2, presence_penalty=0.3, banned_token_ids=[3, 97], logit_bias={50: 2.0, 51: -2.0})
    cand = [sp(temperature=T_FLOOR, top_k=20, seed=11 + i, min_p=M_FLOOR, **(extra if i % 2 else {})) for i in range(4)]
    gath = [sp(temperature=T_FLOOR, top_k=0 if i == 0 else 20, seed=3 + i, min_p=M_FLOOR, **(extra if i % 2 else {}))
            for i in range(4)]
    return cand, gath


def _worker(rank, world, port, ckpt, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                      LOCAL_RANK=str(rank))
    torch.set_num_threads(1)
    from llmss_amd import ops
    from llmss_amd.engine import LLMEngine, build_model
    from llmss_amd.parallel.dist import initialize_distributed

    tp, r, w = initialize_distributed(backend="gloo")
    eng = LLMEngine(build_model(ckpt, tp, "fp32", "cpu"), max_num_seqs=4, block_size=4, num_blocks=64,
                    check_tokens=True, penalties=True, constraints=True, min_p=True)
    assert eng.dist_sampling
    routes = []
    inner_d, inner_s = ops.sample_distributed, ops.sample
    ops.sample_distributed = lambda *a, **k: (routes.append(("cand", k.get("ln_min_p") is not None)),
                                              inner_d(*a, **k))[1]
    ops.sample = lambda *a, **k: (routes.append(("gathered", k.get("ln_min_p") is not None)), inner_s(*a, **k))[1]
    res = []
    for run_sps in _tp_runs():
        res.append([x.output_ids for x in run(eng, PROMPTS[:4], run_sps)])
        res.append(sorted(set(routes)))
        del routes[:]
    allres = tp.all_gather_object(res[0::2])
    assert all(a == res[0::2] for a in allres), "ranks disagree on tokens"
    if r == 0:
        q.put(res)
    torch.distributed.barrier()
    torch.distributed.destroy_process_group()


def test_tp2_gloo_matches_single(tmp_path):
    d = str(tmp_path / "llama")
    hf = save_hf_model("llama", d, vocab=101)  # 101 % 2 != 0: the padded vocab-parallel head
    from llmss_amd.engine import build_model

    eng = LLMEngine(build_model(d, None, "fp32", "cpu"), max_num_seqs=8, block_size=4, num_blocks=64, penalties=True,
                    constraints=True, min_p=True)
    ref = []
    for s in _tp_runs():
        reqs = run(eng, PROMPTS[:4], s)
        assert margins(reqs, hf, 101, M_FLOOR).min() >= -SLACK
        ref.append([x.output_ids for x in reqs])
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, d, q)) for r in range(2)]
    for p in procs:
        p.start()
    got = q.get(timeout=240)
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    cand_tokens, cand_routes, gath_tokens, gath_routes = got
    assert cand_tokens == ref[0] and gath_tokens == ref[1]
    # the first run's decode steps take the candidate route, the second's the gathered one, both with the lane
    assert ("cand", True) in cand_routes and all(lane for _, lane in cand_routes + gath_routes)
    assert ("gathered", True) in gath_routes
