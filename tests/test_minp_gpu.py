"""The MINP variants of the HIP sampler (csrc/sampling.hip) against the fp64 oracle of tests/minp_cases.py, token
for token: every dispatch of launch_sample, the candidate path by shards of one GPU and by per-rank packs, the null
pointer and an all -inf lane against today's sampler, tokens exactly on the floor, tied maxima under min_p = 1, an
all -inf row, and the drawn distribution under a floor. tests/test_minp_cases_cpu.py holds the CPU definition to the
same cases."""
import numpy as np
import pytest
import torch

import minp_cases as M
import sampler_cases as S

pytestmark = pytest.mark.gpu


def _dev():
    return torch.device("cuda")


def _lane(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(_dev())


def test_native_loaded():
    import llmss_amd
    from llmss_amd.ops import hip as H

    assert H.lib().__file__.startswith(llmss_amd.__path__[0])


def _sample_twice(H, logits, params, vocab, lane):
    """H.sample with out2 and ln_min_p, and once more: tokens, after asserting out2 == out and an identical repeat."""
    B = logits.shape[0]
    out2 = torch.full((B,), -1, dtype=torch.int64, device=logits.device)
    got = H.sample(logits, *params, vocab=vocab, out2=out2, ln_min_p=lane)
    assert torch.equal(out2, got)
    assert torch.equal(H.sample(logits, *params, vocab=vocab, ln_min_p=lane), got)  # TP ranks rely on identical draws
    return got.cpu().numpy()


# ------------------------------------------------------------------------------------------ the cases
@pytest.mark.parametrize("case", M.FULL_ROW_CASES, ids=lambda c: c.name)
def test_sample_equals_oracle(case):
    from llmss_amd.ops import hip as H

    inp = M.inputs(case)
    logits = inp.logits.to(_dev())
    assert M.dispatch(case.V, logits.stride(0), case.dtype) == case.kernel and logits.data_ptr() % 16 == 0
    got = _sample_twice(H, logits, inp.params(_dev()), case.V if case.V < case.width else None,
                        _lane(M.ln_min_p(case)))
    assert int(got.max()) < case.V and int(got.min()) >= 0
    M.check_tokens(got, case)


@pytest.mark.parametrize("case", M.SHARD_CASES, ids=lambda c: c.name)
def test_sharded_candidates_equal_oracle(case):
    from llmss_amd.ops import hip as H

    inp = M.inputs(case)
    logits = inp.logits.to(_dev())
    temp, topk, topp, seeds = inp.params(_dev())
    lane = _lane(M.ln_min_p(case))
    pack = H.cand_topk(logits, 0, case.V, temp, topk, shards=case.shards)
    out2 = torch.full((M.B_ROWS,), -1, dtype=torch.int64, device=_dev())
    got = H.sample_cand(pack, H.CAND_KC, temp, topk, topp, seeds, out2=out2, ln_min_p=lane)
    assert torch.equal(out2, got)
    assert torch.equal(H.sample_cand(pack, H.CAND_KC, temp, topk, topp, seeds, ln_min_p=lane), got)
    M.check_tokens(got.cpu().numpy(), case)
    # the full-row kernel draws the same tokens from the same rows
    full = H.sample(logits, temp, topk, topp, seeds, vocab=case.V, ln_min_p=lane)
    assert torch.equal(full, got)


class _FakeGather:
    """In-process stand-in for the TP group: all_gather_last_dim over precomputed per-rank packs."""

    def __init__(self, packs):
        self.packs = packs

    def all_gather_last_dim(self, _):
        return torch.cat(self.packs, -1)


@pytest.mark.parametrize("case", M.TP_CASES, ids=lambda c: c.name)
def test_distributed_candidates_equal_oracle(case):
    from llmss_amd import ops
    from llmss_amd.ops import hip as H

    inp = M.inputs(case)
    logits = inp.logits.to(_dev())
    temp, topk, topp, seeds = inp.params(_dev())
    tp = case.shards
    vl = case.width // tp
    assert vl * tp == case.width
    packs = [H.cand_topk(logits[:, r * vl:(r + 1) * vl].contiguous(), r * vl, case.V, temp, topk) for r in range(tp)]
    for rank in (0, tp - 1):  # what the first and the last rank compute from the same gathered packs
        local = logits[:, rank * vl:(rank + 1) * vl].contiguous()
        got = ops.sample_distributed(local, _FakeGather(packs), rank * vl, case.V, temp, topk, topp, seeds,
                                     ln_min_p=_lane(M.ln_min_p(case)))
        M.check_tokens(got.cpu().numpy(), case)


@pytest.mark.parametrize("case", S.ALL_CASES, ids=lambda c: c.name)
def test_null_pointer_and_off_lane_are_todays_sampler(case):
    """Without the argument (the instantiations that ran before), with ln_min_p = None and with an all -inf lane (the
    MINP instantiations): the same tokens, and the oracle's of sampler_cases on its own cases."""
    from llmss_amd import ops
    from llmss_amd.ops import hip as H

    inp = S.inputs(case)
    logits = inp.logits.to(_dev())
    temp, topk, topp, seeds = inp.params(_dev())
    off = _lane(np.full(S.B_ROWS, -np.inf))
    if case in S.TP_CASES:
        vl = case.width // case.shards
        packs = [H.cand_topk(logits[:, r * vl:(r + 1) * vl].contiguous(), r * vl, case.V, temp, topk)
                 for r in range(case.shards)]
        call = lambda **kw: ops.sample_distributed(logits[:, :vl].contiguous(), _FakeGather(packs), 0, case.V,  # noqa: E731
                                                   temp, topk, topp, seeds, **kw)
    elif case.cand:
        pack = H.cand_topk(logits, 0, case.V, temp, topk, shards=case.shards)
        call = lambda **kw: H.sample_cand(pack, H.CAND_KC, temp, topk, topp, seeds, **kw)  # noqa: E731
    else:
        call = lambda **kw: H.sample(logits, temp, topk, topp, seeds,  # noqa: E731
                                     vocab=case.V if case.V < case.width else None, **kw)
    today = call()
    assert torch.equal(call(ln_min_p=None), today)
    assert torch.equal(call(ln_min_p=off), today)
    S.check_tokens(today.cpu().numpy(), case)


def test_lane_is_validated():
    from llmss_amd.ops import hip as H

    inp = S.inputs(S.FULL_ROW_CASES[0])
    logits = inp.logits.to(_dev())
    params = inp.params(_dev())
    for bad in (torch.zeros(S.B_ROWS, dtype=torch.float64, device=_dev()), torch.zeros(S.B_ROWS - 1, device=_dev()),
                torch.zeros(S.B_ROWS), torch.zeros(S.B_ROWS, 1, device=_dev())):
        with pytest.raises(ValueError, match="ln_min_p"):
            H.sample(logits, *params, ln_min_p=bad)


# ------------------------------------------------------------------------------------------ special rows
BND_SHAPES = [(torch.bfloat16, 1000, 1000, "v3<2,false>"), (torch.bfloat16, 32000, 32000, "v3<4,false>"),
              (torch.bfloat16, 50257, 50304, "v3<8,true>"), (torch.bfloat16, 50257, 50257, "sample_kernel<bf16>"),
              (torch.float32, 1000, 1000, "sample_kernel<float>")]


@pytest.mark.parametrize("kind", list(M.BND_KINDS))
@pytest.mark.parametrize("dtype,V,width,kernel", BND_SHAPES, ids=[s[3] for s in BND_SHAPES])
def test_boundary_rows(kind, dtype, V, width, kernel):
    """top-k 0, top-p 1 - the path that builds no histogram - with ln_min_p = -2 given directly: the token exactly on
    the floor is kept and wins the rows the oracle says (with the floor at +0.0 it holds -0.0), the next bf16 value
    below the floor never wins although its noise is the largest in six rows."""
    from llmss_amd.ops import hip as H

    want = M.boundary_oracle(kind)
    n = want.size
    x = torch.full((n, width), S.PAD_LOGIT, dtype=dtype)
    x[:, :V] = M.boundary_rows(kind, V, dtype)
    logits = x.to(_dev())
    assert M.dispatch(V, logits.stride(0), "fp32" if dtype == torch.float32 else "bf16") == kernel
    params = (torch.ones(n, device=_dev()), torch.zeros(n, dtype=torch.int32, device=_dev()),
              torch.ones(n, device=_dev()), torch.tensor(M.BND_SEEDS[kind], dtype=torch.int64, device=_dev()))
    got = _sample_twice(H, logits, params, V if V < width else None, _lane(np.full(n, M.BND_LN)))
    assert got.tolist() == want.tolist()
    assert M.BND_TOK_KEPT in got.tolist() and M.BND_TOK_MAX in got.tolist()


@pytest.mark.parametrize("kind", list(M.BND_KINDS))
def test_boundary_rows_candidate_path(kind):
    from llmss_amd.ops import hip as H

    want = M.boundary_oracle(kind)
    n = want.size
    logits = M.boundary_rows(kind, 32000, torch.bfloat16).to(_dev())
    temp, topp = torch.ones(n, device=_dev()), torch.ones(n, device=_dev())
    topk = torch.full((n,), 64, dtype=torch.int32, device=_dev())  # the candidate route's rows; the floor keeps two
    seeds = torch.tensor(M.BND_SEEDS[kind], dtype=torch.int64, device=_dev())
    pack = H.cand_topk(logits, 0, 32000, temp, topk, shards=8)
    got = H.sample_cand(pack, H.CAND_KC, temp, topk, topp, seeds, ln_min_p=_lane(np.full(n, M.BND_LN)))
    assert got.tolist() == want.tolist()


@pytest.mark.parametrize("dtype,width", [(torch.bfloat16, 1000), (torch.float32, 1000), (torch.bfloat16, 1001)],
                         ids=["v3", "fallback-fp32", "fallback-bf16"])
def test_tied_maxima_min_p_one(dtype, width):
    """Four tied maxima, min_p = 1: only they are drawn, the oracle's token on every decidable draw, and their counts
    over TIE_N seeds pass the chi-square bound against uniform. Greedy rows with the same lane draw the lowest id."""
    from llmss_amd.ops import hip as H

    toks, dec = M.tie_oracle()
    N = M.TIE_N
    x = torch.full((N, width), S.PAD_LOGIT, dtype=dtype)
    x[:, :M.TIE_V] = M.tie_row(dtype)[None, :]
    logits = x.to(_dev())
    params = (torch.ones(N, device=_dev()), torch.zeros(N, dtype=torch.int32, device=_dev()),
              torch.ones(N, device=_dev()), torch.arange(N, dtype=torch.int64, device=_dev()))
    got = _sample_twice(H, logits, params, M.TIE_V if M.TIE_V < width else None, _lane(np.zeros(N)))
    bad = np.flatnonzero(dec & (got != toks))
    assert bad.size == 0, (bad[:8].tolist(), got[bad[:8]].tolist(), toks[bad[:8]].tolist())
    stat, bound = M.tie_chi2(got), S.chi2_bound(len(M.TIE_TOKENS) - 1)
    print(f"chi2 {stat:.2f} bound {bound:.2f}")
    assert stat < bound
    greedy = (torch.zeros(N, device=_dev()),) + params[1:]
    got = H.sample(logits, *greedy, vocab=M.TIE_V if M.TIE_V < width else None, ln_min_p=_lane(np.zeros(N)))
    assert got.unique().tolist() == [M.TIE_TOKENS[0]]


@pytest.mark.parametrize("dtype,V", [(torch.bfloat16, 1000), (torch.bfloat16, 50257), (torch.float32, 1000)],
                         ids=["v3", "fallback-bf16", "fallback-fp32"])
def test_all_inf_row(dtype, V):
    from llmss_amd.ops import hip as H

    logits = torch.full((4, V), float("-inf"), dtype=dtype, device=_dev())
    params = (torch.ones(4, device=_dev()), torch.tensor([0, 40, 0, 40], dtype=torch.int32, device=_dev()),
              torch.tensor([1.0, 0.9, 0.9, 1.0], device=_dev()), torch.arange(4, dtype=torch.int64, device=_dev()))
    for lane in (np.full(4, -2.0), np.full(4, -np.inf), np.zeros(4)):
        assert H.sample(logits, *params, ln_min_p=_lane(lane)).tolist() == [0, 0, 0, 0]
    if dtype == torch.bfloat16 and V == 1000:
        topk = torch.full((4,), 40, dtype=torch.int32, device=_dev())
        pack = H.cand_topk(logits, 0, V, params[0], topk, shards=2)
        assert H.sample_cand(pack, H.CAND_KC, params[0], topk, params[2], params[3],
                             ln_min_p=_lane(np.full(4, -2.0))).tolist() == [0, 0, 0, 0]


# ------------------------------------------------------------------------------------------ distribution
@pytest.mark.parametrize("family", S.DIST_FAMILIES)
@pytest.mark.parametrize("k,p,t,min_p", M.DIST_PARAMS)
def test_distribution_under_floor(k, p, t, min_p, family):
    """DIST_N draws of one 64-token row under a floor (alone: no histogram is built; inside a top-k; with top-p at
    temperature 0.7): the oracle's token on every decidable draw, and the counts pass Pearson's chi-square against
    the exact renormalised probabilities of the kept set at the 1 - 1e-6 quantile."""
    from llmss_amd.ops import hip as H

    toks, dec, kept, pr = M.dist_oracle(k, p, t, min_p, family)
    assert 1.0 - dec.mean() <= M.MAX_UNDECIDABLE
    N = S.DIST_N
    logits = S.dist_row()[None, :].repeat(N, 1).contiguous().to(_dev())
    params = (torch.full((N,), t, device=_dev()), torch.full((N,), k, dtype=torch.int32, device=_dev()),
              torch.full((N,), p, device=_dev()), torch.from_numpy(S.dist_seeds(family)).to(_dev()))
    got = _sample_twice(H, logits, params, None, _lane(np.repeat(M.ln_of(min_p), N)))
    bad = np.flatnonzero(dec & (got != toks))
    assert bad.size == 0, (bad[:8].tolist(), got[bad[:8]].tolist(), toks[bad[:8]].tolist())
    stat, bound = S.chi2_stat(got, kept, pr), S.chi2_bound(kept.size - 1)
    print(f"chi2 {stat:.1f} bound {bound:.1f} dof {kept.size - 1} undecidable {(~dec).sum()}")
    assert stat < bound, (stat, bound)
