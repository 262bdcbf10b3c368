"""min_p through the GPU engine: graph-captured, pipelined decode (the MINP sampler variants inside the graphs)
against the same engine decoding eagerly across a bucket change, the floor property against a one-shot prefill's
logits, log-probabilities still those of the raw distribution, and default requests and a min_p=False engine
unchanged."""
import math
import struct

import numpy as np
import pytest
import torch

from llmss_amd.engine import LLMEngine, SamplingParams
from llmss_amd.models.config import get_preset
from llmss_amd.models.decoder import DecoderLM, StepInput
from llmss_amd.models.weights import random_weights

pytestmark = pytest.mark.gpu
N = 5
NEW = 24
# rows 1 and 3 leave early; the pipelined decode keeps their rows as padding until the scheduler runs again, which the
# late arrival of a sixth request forces: the batch then falls from the 8-row bucket into the 4-row one
LENS = (24, 6, 24, 10, 24)
LATE = 14  # engine steps before the sixth request arrives
NEAR_TIE = 0.1  # test_engine_gpu._near_tie: a 0.05 per-logit difference between kernel routes is bf16 noise
# The floor property: m = 0.05 at temperature 1, two batches of 5 x 48 tokens. The model's 211 logits have a standard
# deviation of 0.7 and the most likely token a probability of about 0.025, so about four tokens lie within NEAR_TIE of
# the floor 3.0 below the maximum, each drawn with probability 0.05 x 0.025: 0.5 % of the draws fall in the band where
# a token is not judged (2 % are allowed), while the tokens below the floor hold about 3 % of the mass - the run
# without min_p leaves the floor about a dozen times in 480 draws. On the CPU engine in fp32: 1 of 120 in the band
# with min_p, 4 of 120 below the band without.
M_FLOOR = 0.05
FLOOR_NEW = 48
FLOOR_SEEDS = (21, 57)


def _bits(x):
    return struct.pack("<f", x)


def run(eng, prompts, sps, late=None):
    """``late``: (prompt, params) of one more request that arrives after LATE engine steps."""
    rids = [eng.add_request(p, sp) for p, sp in zip(prompts, sps)]
    events, done, steps = [], {}, 0
    while eng.has_unfinished():
        events += eng.step()
        steps += 1
        if late is not None and steps == LATE:
            rids.append(eng.add_request(*late))
        for r in eng.pop_finished():
            done[r.id] = r
    return [done[i] for i in rids], events


def _sps(ms, lens=(NEW,) * 5, logprobs=None, seed=11):
    """Row 0 greedy, rows 1-4 sampled with fixed seeds (row 1 with top-k and top-p, the others unrestricted), row i
    with min_p = ms[i]."""
    out = []
    for i, m in enumerate(ms):
        kw = dict(max_new_tokens=lens[i], ignore_eos=True, logprobs=logprobs, min_p=m)
        if i == 0:
            kw.update(is_greedy=True)
        elif i == 1:
            kw.update(temperature=0.8, top_k=20, top_p=0.9, seed=seed + i)
        else:
            kw.update(temperature=1.0, top_k=0, top_p=1.0, seed=seed + i)
        out.append(SamplingParams(**kw))
    return out


NONE = [0.0] * 5
MIXED = [0.3, 0.3, 0.05, 1.0, 0.5]


@pytest.fixture(scope="module")
def setup():
    cfg = get_preset("tiny-llama", hidden_size=256, num_heads=4, num_kv_heads=2, head_dim=64, rotary_dim=64,
                     intermediate_size=512, max_position_embeddings=256)
    w = random_weights(cfg, device="cuda", dtype=torch.bfloat16, seed=3, std=0.05)
    m = DecoderLM(cfg, w)
    g = torch.Generator().manual_seed(0)
    prompts = [[int(x) for x in torch.randint(0, cfg.vocab_size, (n,), generator=g)] for n in (5, 17, 33, 2, 60)]
    on = LLMEngine(m, max_num_seqs=8, block_size=16, use_graphs=True, max_logprobs=N, min_p=True)
    off = LLMEngine(m, max_num_seqs=8, block_size=16, use_graphs=True, max_logprobs=N)
    plain, _ = run(on, prompts, _sps(NONE))
    return cfg, m, prompts, on, off, plain


def _raw_logits(m, r):
    """[len(output), width] logits of a one-shot prefill of prompt + output: row t is the distribution of output[t]."""
    ids = r.prompt_ids + r.output_ids
    T, Pn = len(ids), len(r.prompt_ids)
    x = torch.tensor(ids, device="cuda")
    return m(StepInput("prefill", x, torch.arange(T, device="cuda"), torch.full((T,), -1, device="cuda"),
                       cu_seqlens=torch.tensor([0, T], dtype=torch.int32, device="cuda"), max_seqlen=T,
                       last_idx=torch.arange(Pn - 1, T - 1, device="cuda")), m.allocate_kv_cache(8, 16))


def test_graphs_equal_eager_across_a_bucket_change(setup):
    cfg, m, prompts, on, off, plain = setup
    assert on.use_graphs and on.graphs and on.async_decode and on.buf.lnmp is not None
    late = (prompts[1][:9], SamplingParams(max_new_tokens=12, ignore_eos=True, temperature=1.0, top_k=0, top_p=1.0,
                                           seed=77, min_p=0.3))
    buckets, lanes = [], []
    inner = on.buf.fill
    on.buf.fill = lambda k, b_pad, *a, **kw: (buckets.append(b_pad), lanes.append(kw.get("lnmp")),
                                              inner(k, b_pad, *a, **kw))[1]
    try:
        reqs, _ = run(on, prompts, _sps(MIXED, LENS), late=late)
    finally:
        on.buf.fill = inner
    assert len(set(buckets)) >= 2 and all((b, False) in on.graphs for b in set(buckets)), sorted(set(buckets))
    assert all(ln is not None for ln in lanes) and any(np.isfinite(ln).any() for ln in lanes)
    on.use_graphs = False
    try:
        eager, _ = run(on, prompts, _sps(MIXED, LENS), late=late)
    finally:
        on.use_graphs = True
    assert len(reqs) == 6 and reqs[5].output_ids == eager[5].output_ids and len(reqs[5].output_ids) == 12
    for r, e, n in zip(reqs, eager, LENS):
        assert r.output_ids == e.output_ids and len(r.output_ids) == n
    # the floor changes what the sampled rows draw
    assert sum(r.output_ids != p.output_ids[:len(r.output_ids)] for r, p in zip(reqs[1:5], plain[1:5])) >= 2


def _floor_gaps(m, reqs, V, mp):
    """Per sampled token, in logits: (logit_tok - logit_max) - T ln(min_p) on a one-shot prefill's logits."""
    out = []
    for r in reqs:
        lg = _raw_logits(m, r)[:, :V].double().cpu().numpy()
        for t, tok in enumerate(r.output_ids):
            out.append(lg[t, tok] - lg[t].max() - r.params.temperature * math.log(mp))
    return np.array(out)


def test_floor_property(setup):
    """Every token of a min_p request is on or above the floor of its own prefix's logits; a token within NEAR_TIE of
    the floor is not judged, and at most 2 % are. The same requests and seeds without min_p go below the band."""
    cfg, m, prompts, on, off, plain = setup
    V = cfg.vocab_size

    def sps(mp):
        return [[SamplingParams(max_new_tokens=FLOOR_NEW, ignore_eos=True, temperature=1.0, top_k=0, top_p=1.0,
                                seed=s + i, min_p=mp) for i in range(5)] for s in FLOOR_SEEDS]
    with_floor = np.concatenate([_floor_gaps(m, run(on, prompts, s)[0], V, M_FLOOR) for s in sps(M_FLOOR)])
    without = np.concatenate([_floor_gaps(m, run(on, prompts, s)[0], V, M_FLOOR) for s in sps(0.0)])
    band = int((np.abs(with_floor) <= NEAR_TIE).sum())
    print(f"with min_p: lowest gap {with_floor.min():.4f}, {band} of {with_floor.size} in the band; without: lowest "
          f"{without.min():.4f}, {int((without < -NEAR_TIE).sum())} of {without.size} below the band")
    assert with_floor.size == 2 * 5 * FLOOR_NEW
    assert with_floor.min() >= -NEAR_TIE
    assert band <= 0.02 * with_floor.size
    assert (without < -NEAR_TIE).sum() >= 1


def test_logprobs_stay_raw(setup):
    cfg, m, prompts, on, off, plain = setup
    V = cfg.vocab_size
    reqs, _ = run(on, prompts, _sps([1.0] * 5, logprobs=N))
    for r in reqs:
        want = torch.log_softmax(_raw_logits(m, r)[:, :V].double(), dim=-1).cpu()
        assert len(r.output_logprobs) == NEW
        for t, (tok, lp, top) in enumerate(zip(r.output_ids, r.output_logprobs, r.output_top_logprobs)):
            assert abs(lp - want[t, tok].item()) <= 0.1, (r.id, t, lp, want[t, tok].item())
            for i, v in top:
                assert abs(v - want[t, i].item()) <= 0.1
    # min_p = 1 leaves the most likely token alone: under the floored distribution its log-probability would be 0
    for r in reqs:
        assert max(r.output_logprobs) < -0.5


def test_default_requests_and_disabled_engine_unchanged(setup):
    cfg, m, prompts, on, off, plain = setup
    a, _ = run(on, prompts, _sps(NONE, logprobs=N))
    b, _ = run(off, prompts, _sps(NONE, logprobs=N))
    snap = lambda rs: [(r.output_ids, [_bits(v) for v in r.output_logprobs],  # noqa: E731
                        [[(i, _bits(v)) for i, v in top] for top in r.output_top_logprobs]) for r in rs]
    assert snap(a) == snap(b)
    # off: graph keys, buffers and fingerprint as without the feature
    assert off.min_p is False and sorted(off.graphs) == sorted(on.graphs)
    buf, B, MB = off.buf, off.buf.max_b, off.buf.max_blocks
    assert buf.lnmp is None
    assert buf.o32 == 32 * B and buf.of32 == buf.o32 + (2 * B + B * MB) * 4 and buf.d.numel() == buf.of32 + 8 * B
    assert buf.topp.data_ptr() + 4 * B == buf.d.data_ptr() + buf.d.numel()
    # on: the lane ends the fp32 part, nothing else moved
    ob = on.buf
    assert (ob.o32, ob.of32) == (buf.o32, buf.of32) and ob.d.numel() == buf.d.numel() + 4 * B
    assert ob.lnmp.data_ptr() == ob.topp.data_ptr() + 4 * B and ob.lnmp.numel() == B
    fa, fb = off.fingerprint(), on.fingerprint()
    assert fa.pop("min_p") is False and fb.pop("min_p") is True and fa == fb
    with pytest.raises(ValueError, match="min_p=True"):
        off.add_request([1, 2, 3], SamplingParams(max_new_tokens=2, min_p=0.1))
    assert not off.has_unfinished() and not off.requests
