"""Repetition / presence / frequency penalties through the engine on the CPU (tiny GPT-2 and Llama, fp32): every
greedy token is the argmax of the oracle-penalised Hugging Face logits for the same prefix - also under chunked
prefill, preemption, slot reuse and an abort - plus the opt-in rules and TP=2 over gloo on both sampler routes."""
import os
import socket

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

import penalty_cases as P
from helpers import save_hf_model
from llmss_amd.engine import LLMEngine, SamplingParams
from llmss_amd.models.config import ModelConfig
from llmss_amd.models.decoder import DecoderLM
from llmss_amd.models.weights import load_hf_weights
from llmss_amd.utils.checkpoint import CheckpointReader, weight_files

TOL = 1e-4  # the facade parity tests' tolerance on fp32 logits
NEW = 16
PROMPTS = [[(3 * i + 7 * j) % 100 for j in range(5 + 2 * i)] for i in range(6)]
PENALTIES = [(1.3, 0.0, 0.0), (1.0, 0.7, 0.45), (1.5, 1.0, 0.5), (0.8, 0.25, 0.0), (2.0, 0.0, 1.0), (1.2, 2.0, 2.0)]


def sp(pen=None, n=NEW, **kw):
    r, p, f = pen or (1.0, 0.0, 0.0)
    kw.setdefault("is_greedy", True)
    return SamplingParams(max_new_tokens=n, ignore_eos=True, repetition_penalty=r, presence_penalty=p,
                          frequency_penalty=f, **kw)


def run(eng, prompts, sps, abort_after=None):
    """Requests (in submission order) of a run to completion; ``abort_after`` = (steps, index) aborts one mid-run."""
    rids = [eng.add_request(p, s) for p, s in zip(prompts, sps)]
    done, steps = {}, 0
    while eng.has_unfinished():
        eng.step()
        steps += 1
        if abort_after and steps == abort_after[0]:
            eng.abort(rids[abort_after[1]])
        for r in eng.pop_finished():
            done[r.id] = r
    for r in eng.pop_finished():
        done[r.id] = r
    return [done[i] for i in rids]


@pytest.fixture(scope="module")
def ckpts(tmp_path_factory):
    out = {}
    for name in ("gpt2", "llama"):
        d = str(tmp_path_factory.mktemp(name))
        out[name] = (d, save_hf_model(name, d))
    return out


def _engine(d, **kw):
    cfg = ModelConfig.from_pretrained(d)
    w = load_hf_weights(cfg, CheckpointReader(weight_files(d)), 1, 0, device="cpu", dtype=torch.float32)
    kw.setdefault("max_num_seqs", 4)
    kw.setdefault("num_blocks", 64)
    return LLMEngine(DecoderLM(cfg, w), block_size=4, **kw), cfg


def verify(reqs, hf, cfg):
    """Every generated token is the argmax of the oracle-penalised Hugging Face logits for its prefix."""
    for r in reqs:
        if not r.output_ids:
            continue
        q = r.params
        with torch.no_grad():
            logits = hf(torch.tensor([r.prompt_ids + r.output_ids])).logits[0].double().numpy()
        for t, tok in enumerate(r.output_ids):
            row = logits[len(r.prompt_ids) - 1 + t, :cfg.vocab_size]
            pen = P.penalise_row(row, r.prompt_ids, r.output_ids[:t], q.repetition_penalty, q.presence_penalty,
                                 q.frequency_penalty)
            assert pen.max() - pen[tok] <= TOL, (r.id, t, tok, int(pen.argmax()), pen.max() - pen[tok])


def repeats(reqs):
    return sum(len(set(r.output_ids)) < len(r.output_ids) for r in reqs)


def idle(eng):
    return not eng._pen_slot and sorted(eng._pen_free) == list(range(eng.max_num_seqs))


@pytest.mark.parametrize("name", ["gpt2", "llama"])
def test_greedy_tokens_match_penalised_hf(ckpts, name):
    d, hf = ckpts[name]
    eng, cfg = _engine(d, penalties=True, max_num_seqs=8)
    assert eng.stats["penalty_state_bytes"] == 8 * cfg.vocab_size * 4
    plain = run(eng, PROMPTS, [sp() for _ in PROMPTS])
    assert repeats(plain) * 2 >= len(plain), "the unpenalised outputs do not repeat: the test shows nothing"
    verify(plain, hf, cfg)
    reqs = run(eng, PROMPTS, [sp(pen) for pen in PENALTIES])
    assert all(len(r.output_ids) == NEW for r in reqs)
    verify(reqs, hf, cfg)
    assert [r.output_ids for r in reqs] != [r.output_ids for r in plain]
    assert idle(eng)


@pytest.mark.parametrize("how", ["chunked", "preempt", "reuse", "abort"])
def test_same_check_under(ckpts, how):
    d, hf = ckpts["llama"]
    kw = {"chunked": dict(prefill_chunk=4), "preempt": dict(num_blocks=14), "reuse": dict(max_num_seqs=2),
          "abort": {}}[how]
    eng, cfg = _engine(d, penalties=True, **kw)
    reqs = run(eng, PROMPTS, [sp(pen) for pen in PENALTIES], abort_after=(9, 1) if how == "abort" else None)
    if how == "preempt":
        assert eng.stats["preemptions"] > 0
    if how == "abort":
        assert reqs[1].finish_reason == "abort" and 0 < len(reqs[1].output_ids) < NEW
    assert all(len(r.output_ids) == NEW for r in reqs if r.finish_reason != "abort")
    verify(reqs, hf, cfg)
    assert idle(eng)


def test_mixed_batch_defaults_unchanged(ckpts):
    d, hf = ckpts["llama"]
    off, cfg = _engine(d)
    on, _ = _engine(d, penalties=True)
    base = run(off, PROMPTS[:4], [sp() for _ in range(4)])
    sps = [sp(), sp(PENALTIES[2]), sp(), sp(PENALTIES[1])]
    mixed = run(on, PROMPTS[:4], sps)
    assert mixed[0].output_ids == base[0].output_ids and mixed[2].output_ids == base[2].output_ids
    assert mixed[1].output_ids != base[1].output_ids
    verify(mixed, hf, cfg)
    seeded = [sp(temperature=0.9, top_k=20, top_p=0.9, seed=5 + i, is_greedy=False) for i in range(4)]
    a = run(off, PROMPTS[:4], seeded)
    b = run(on, PROMPTS[:4], [SamplingParams(**s.__dict__) for s in seeded])
    assert [r.output_ids for r in a] == [r.output_ids for r in b]


def test_opt_in_and_validation(ckpts):
    d, _ = ckpts["llama"]
    assert SamplingParams().has_penalties is False
    for kw in (dict(repetition_penalty=1.1), dict(presence_penalty=0.5), dict(frequency_penalty=-0.5)):
        assert SamplingParams(**kw).validate().has_penalties
    for kw in (dict(repetition_penalty=0.0), dict(repetition_penalty=-1.0), dict(repetition_penalty=float("inf")),
               dict(repetition_penalty=float("nan")), dict(repetition_penalty="2"), dict(presence_penalty=2.5),
               dict(presence_penalty=-2.5), dict(presence_penalty=float("nan")), dict(frequency_penalty=2.01),
               dict(frequency_penalty=float("-inf")), dict(frequency_penalty=None)):
        with pytest.raises(ValueError):
            SamplingParams(**kw).validate()
    for kw in (dict(repetition_penalty=100.0), dict(presence_penalty=2.0), dict(frequency_penalty=-2.0)):
        SamplingParams(**kw).validate()
    off, _ = _engine(d)
    assert off.penalties is False and off.fingerprint()["penalties"] is False and off.pen_state is None
    assert "penalty_state_bytes" not in off.stats
    with pytest.raises(ValueError):
        off.add_request([1, 2, 3], sp((1.2, 0.0, 0.0), n=2))
    assert not off.has_unfinished() and not off.requests  # the rejected request left nothing behind
    off.add_request([1, 2, 3], sp(n=2))  # the defaults are no penalty
    on, _ = _engine(d, penalties=True)
    assert on.fingerprint()["penalties"] is True
    with pytest.raises(ValueError):
        on.add_request([1, 2, 3], sp((0.0, 0.0, 0.0), n=2))
    with pytest.raises(ValueError):
        on.add_request([1, 2, 3], sp((1.0, 3.0, 0.0), n=2))
    assert not on.has_unfinished() and not on.requests


# ---------------------------------------------------------------------------------------- TP=2 over gloo
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _tp_runs():
    """Two runs: rows the vocab-parallel candidate sampler takes (greedy, top-k <= 64), then a batch with an
    unrestricted row, which goes through the gathered logits."""
    cand = [sp(PENALTIES[i], is_greedy=i % 2 == 0, temperature=0.9, top_k=20, top_p=0.9, seed=11 + i) for i in range(4)]
    gath = [sp(PENALTIES[i + 1], is_greedy=False, temperature=0.9, top_k=0 if i == 0 else 20, top_p=0.9, seed=3 + i)
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
                    check_tokens=True, penalties=True)
    assert eng.dist_sampling
    widths = []
    inner = ops.apply_penalties
    ops.apply_penalties = lambda lg, *a, **k: (widths.append((lg.shape[1], a[6])), inner(lg, *a, **k))[1]
    res = []
    for sps in _tp_runs():
        res.append([x.output_ids for x in run(eng, PROMPTS[:4], sps)])
        res.append(sorted(set(widths)))
        del widths[:]
    assert idle(eng)
    allres = tp.all_gather_object(res[0::2])
    assert all(a == res[0::2] for a in allres), "ranks disagree on tokens"
    if r == 0:
        q.put(res)
    torch.distributed.barrier()
    torch.distributed.destroy_process_group()


def test_tp2_gloo_matches_single(tmp_path):
    d = str(tmp_path / "llama")
    save_hf_model("llama", d, vocab=101)  # 101 % 2 != 0: the padded vocab-parallel head
    from llmss_amd.engine import build_model

    eng = LLMEngine(build_model(d, None, "fp32", "cpu"), max_num_seqs=4, block_size=4, num_blocks=64, penalties=True)
    ref = [[x.output_ids for x in run(eng, PROMPTS[:4], sps)] for sps in _tp_runs()]
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
    cand_tokens, cand_calls, gath_tokens, gath_calls = got
    assert cand_tokens == ref[0] and gath_tokens == ref[1]
    # rank 0's launches: its shard of the padded head (fewer columns than the vocabulary) at lo = 0 on the
    # vocab-parallel route, whole rows on the gathered one
    assert cand_calls and all(wd < 101 and lo == 0 for wd, lo in cand_calls), cand_calls
    assert any(wd >= 101 and lo == 0 for wd, lo in gath_calls), gath_calls
