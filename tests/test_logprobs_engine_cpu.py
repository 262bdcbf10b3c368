"""Per-token log-probabilities through the engine on the CPU: against Hugging Face's fp32 logits for the same
prefix (tiny GPT-2 and Llama), the opt-in rules, and TP=2 over gloo through the vocab-parallel path."""
import os
import socket

import pytest
import torch
import torch.multiprocessing as mp

import logprob_cases as L
from helpers import save_hf_model
from llmss_amd.engine import LLMEngine, SamplingParams
from llmss_amd.engine.engine import Request, StepEvent
from llmss_amd.engine.sampling import MAX_TOP_LOGPROBS
from llmss_amd.models.config import ModelConfig
from llmss_amd.models.decoder import DecoderLM
from llmss_amd.models.weights import load_hf_weights
from llmss_amd.utils.checkpoint import CheckpointReader, weight_files

TOL = 1e-4  # the facade parity tests' tolerance on fp32 logits
PROMPTS = [[(3 * i + 7 * j) % 100 for j in range(5 + 2 * i)] for i in range(3)]


def run(eng, prompts, sps):
    """Requests (in submission order) and every event of a run to completion."""
    sps = sps if isinstance(sps, list) else [sps] * len(prompts)
    rids = [eng.add_request(p, sp) for p, sp in zip(prompts, sps)]
    events, done = [], {}
    while eng.has_unfinished():
        events += eng.step()
        for r in eng.pop_finished():
            done[r.id] = r
    return [done[i] for i in rids], events


def _sps(n, logprobs, greedy):
    if greedy:
        return [SamplingParams(max_new_tokens=8, is_greedy=True, ignore_eos=True, logprobs=logprobs) for _ in range(n)]
    return [SamplingParams(max_new_tokens=8, temperature=0.9, top_k=20, top_p=0.9, seed=5 + i, ignore_eos=True,
                           logprobs=logprobs) for i in range(n)]


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
    return LLMEngine(DecoderLM(cfg, w), max_num_seqs=4, block_size=4, num_blocks=64, **kw), cfg


@pytest.mark.parametrize("greedy", [True, False])
@pytest.mark.parametrize("name", ["gpt2", "llama"])
def test_engine_logprobs_match_hf(ckpts, name, greedy):
    d, hf = ckpts[name]
    eng, cfg = _engine(d, max_logprobs=5)
    reqs, events = run(eng, PROMPTS, _sps(len(PROMPTS), 5, greedy))
    by_req = {}
    for e in events:
        by_req.setdefault(e.req_id, []).append(e)
    for r in reqs:
        n = len(r.output_ids)
        assert n == 8 and len(r.output_logprobs) == n and len(r.output_top_logprobs) == n
        assert [e.token for e in by_req[r.id]] == r.output_ids
        assert [e.logprob for e in by_req[r.id]] == r.output_logprobs
        assert [e.top_logprobs for e in by_req[r.id]] == r.output_top_logprobs
        with torch.no_grad():
            logits = hf(torch.tensor([r.prompt_ids + r.output_ids])).logits[0].float()
        want = torch.log_softmax(logits[:, :cfg.vocab_size], dim=-1)
        for t, (tok, lp, top) in enumerate(zip(r.output_ids, r.output_logprobs, r.output_top_logprobs)):
            row = want[len(r.prompt_ids) - 1 + t]
            assert abs(lp - row[tok].item()) <= TOL
            assert len(top) == 5 and len({i for i, _ in top}) == 5
            hv, hi = torch.sort(row, descending=True, stable=True)
            for j, (i, v) in enumerate(top):
                assert abs(v - row[i].item()) <= TOL
                # the same id, unless Hugging Face's own values at this place tie within the tolerance
                assert i == hi[j].item() or abs(row[i].item() - hv[j].item()) <= TOL, (t, j, top, hi[:5].tolist())
            if greedy:
                assert top[0] == (tok, lp)


def test_opt_in_rules(ckpts):
    d, _ = ckpts["llama"]
    off, _ = _engine(d)
    assert off.max_logprobs == 0 and off.fingerprint()["max_logprobs"] == 0
    with pytest.raises(ValueError):
        off.add_request([1, 2, 3], SamplingParams(max_new_tokens=2, logprobs=0))
    assert not off.has_unfinished()  # the rejected request left nothing behind
    reqs, events = run(off, PROMPTS[:1], SamplingParams(max_new_tokens=3, is_greedy=True, ignore_eos=True))
    assert reqs[0].output_logprobs == [] and all(e.logprob is None and e.top_logprobs is None for e in events)
    on, _ = _engine(d, max_logprobs=3)
    assert on.fingerprint()["max_logprobs"] == 3
    with pytest.raises(ValueError):
        on.add_request([1, 2, 3], SamplingParams(max_new_tokens=2, logprobs=4))
    for bad in (-1, MAX_TOP_LOGPROBS + 1, 1.5, True):
        with pytest.raises(ValueError):
            SamplingParams(logprobs=bad).validate()
        with pytest.raises(ValueError):
            on.add_request([1, 2, 3], SamplingParams(max_new_tokens=2, logprobs=bad))
    for ok in (None, 0, MAX_TOP_LOGPROBS):
        SamplingParams(logprobs=ok).validate()
    with pytest.raises(ValueError):
        _engine(d, max_logprobs=MAX_TOP_LOGPROBS + 1)
    # positional and default construction as before
    assert StepEvent(1, 2, False).logprob is None and StepEvent(1, 2, True, "eos").top_logprobs is None
    assert Request(0, [1], SamplingParams(), 7).output_logprobs == []


def test_mixed_batch_and_truncation(ckpts):
    """One batch: a request without the option gets None, logprobs=0 the token's alone, logprobs=2 two of three."""
    d, _ = ckpts["llama"]
    eng, _ = _engine(d, max_logprobs=3)
    sps = [SamplingParams(max_new_tokens=6, is_greedy=True, ignore_eos=True, logprobs=n) for n in (None, 0, 2)]
    reqs, events = run(eng, PROMPTS, sps)
    full, _ = run(eng, PROMPTS, [SamplingParams(max_new_tokens=6, is_greedy=True, ignore_eos=True, logprobs=3)] * 3)
    assert [r.output_ids for r in reqs] == [r.output_ids for r in full]
    assert reqs[0].output_logprobs == [] and reqs[0].output_top_logprobs == []
    assert all(e.logprob is None for e in events if e.req_id == reqs[0].id)
    assert reqs[1].output_logprobs == full[1].output_logprobs and reqs[1].output_top_logprobs == [[]] * 6
    assert all(e.logprob is not None and e.top_logprobs == [] for e in events if e.req_id == reqs[1].id)
    assert reqs[2].output_logprobs == full[2].output_logprobs
    assert reqs[2].output_top_logprobs == [t[:2] for t in full[2].output_top_logprobs]


# ---------------------------------------------------------------------------------------- TP=2 over gloo
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, world, port, ckpt, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                      LOCAL_RANK=str(rank))
    torch.set_num_threads(1)
    from llmss_amd.engine import LLMEngine, build_model
    from llmss_amd.parallel.dist import initialize_distributed

    tp, r, w = initialize_distributed(backend="gloo")
    eng = LLMEngine(build_model(ckpt, tp, "fp32", "cpu"), max_num_seqs=4, block_size=4, num_blocks=64,
                    check_tokens=True, max_logprobs=5)
    assert eng.dist_sampling  # greedy and top-k <= 64 rows take the vocab-parallel path
    calls = [0]
    from llmss_amd import ops
    inner = ops.token_logprobs_distributed
    ops.token_logprobs_distributed = lambda *a, **k: (calls.__setitem__(0, calls[0] + 1), inner(*a, **k))[1]
    res = []
    for greedy in (True, False):
        reqs, _ = run(eng, PROMPTS, _sps(len(PROMPTS), 5, greedy))
        res.append([(x.output_ids, x.output_logprobs, x.output_top_logprobs) for x in reqs])
    assert calls[0] > 0, "the vocab-parallel log-probability path never ran"
    allres = tp.all_gather_object(res)
    assert all(a == res for a in allres), "ranks disagree on log-probabilities"
    if r == 0:
        q.put(res)
    torch.distributed.barrier()
    torch.distributed.destroy_process_group()


def test_tp2_gloo_matches_single(tmp_path):
    d = str(tmp_path / "llama")
    save_hf_model("llama", d, vocab=101)  # 101 % 2 != 0: the padded vocab-parallel head
    from llmss_amd.engine import build_model

    eng = LLMEngine(build_model(d, None, "fp32", "cpu"), max_num_seqs=4, block_size=4, num_blocks=64, max_logprobs=5)
    ref = []
    for greedy in (True, False):
        reqs, _ = run(eng, PROMPTS, _sps(len(PROMPTS), 5, greedy))
        ref.append([(x.output_ids, x.output_logprobs, x.output_top_logprobs) for x in reqs])
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
    worst = 0.0
    for ref_run, got_run in zip(ref, got):
        for (ids, lps, tops), (ids2, lps2, tops2) in zip(ref_run, got_run):
            assert ids == ids2
            for a, b, ta, tb in zip(lps, lps2, tops, tops2):
                assert [i for i, _ in ta] == [i for i, _ in tb]
                # max - x of an entry = (log-probability of the row's maximum, top[0]) - (its own)
                worst = max(worst, abs(a - b) / L.tol(101, ta[0][1] - a))
                for (_, va), (_, vb) in zip(ta, tb):
                    worst = max(worst, abs(va - vb) / L.tol(101, ta[0][1] - va))
    print(f"TP=2 against TP=1: worst difference {worst:.3f} x tol")
    assert worst <= 1.0
