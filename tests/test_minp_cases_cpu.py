"""The min-p floor on the CPU: the oracle of tests/minp_cases.py against the definition ops/reference.py on the very
cases tests/test_minp_gpu.py gives the HIP kernels; that the cases tell eight wrong definitions from the right one;
the kept set against Hugging Face's MinPLogitsWarper; and the request field (validate, k_ln_min_p)."""
import math

import numpy as np
import pytest
import torch

import minp_cases as M
import sampler_cases as S
from llmss_amd.engine.sampling import SamplingParams
from llmss_amd.ops import reference as R


def _vl(case):
    return case.width // case.shards if case in M.TP_CASES else -(-case.width // case.shards)


def _ref_full(case, lane):
    inp = M.inputs(case)
    return R.sample(inp.logits[:, :case.V], inp.temp, inp.topk, inp.topp, inp.seeds, ln_min_p=lane).numpy()


def _ref_cand(case, lane):
    inp = M.inputs(case)
    vl = _vl(case)
    packs = [R.cand_topk(inp.logits[:, r * vl:(r + 1) * vl], r * vl, case.V, inp.temp, inp.topk, 64, 128)
             for r in range(case.shards)]
    return R.sample_cand(torch.cat(packs, -1), case.shards, 128, inp.temp, inp.topk, inp.topp, inp.seeds, case.V,
                         ln_min_p=lane).numpy()


# ------------------------------------------------------------------------------------------ the cases themselves
def test_cases_mirror_every_dispatch():
    assert [c.kernel for c in M.ALL_CASES] == [c.kernel for c in S.ALL_CASES]
    assert not {c.seed for c in M.ALL_CASES} & {c.seed for c in S.ALL_CASES}
    for c in M.FULL_ROW_CASES:
        assert M.dispatch(c.V, c.width, c.dtype) == c.kernel
    assert any(c.width > c.V and c.kernel.startswith("v3") for c in M.FULL_ROW_CASES)  # PAD_LOGIT columns
    assert any(c.width % 8 for c in M.FULL_ROW_CASES)  # the odd stride
    for c in M.ALL_CASES:
        assert set(M.min_ps(c)) <= set(M.MIN_PS) and len(set(M.min_ps(c))) == len(M.MIN_PS)
        lane = M.ln_min_p(c)
        assert lane.dtype == np.float32 and bool((np.isneginf(lane) == (M.min_ps(c) == 0)).all())


@pytest.mark.parametrize("case", M.ALL_CASES, ids=lambda c: c.name)
def test_oracle_decides_every_row_and_the_floor_matters(case):
    """No undecidable row at these seeds, and the floor changes drawn tokens: a sampler without it fails the case."""
    tok, dec = M.oracle(case)
    assert bool(dec.all()), np.flatnonzero(~dec)
    tok0, _ = M.oracle(case, False)
    changed = int((tok != tok0).sum())
    assert changed >= 4, changed
    with pytest.raises(AssertionError):
        M.check_tokens(tok0, case)


# ------------------------------------------------------------------------------------------ definition vs oracle
@pytest.mark.parametrize("case", M.FULL_ROW_CASES, ids=lambda c: c.name)
def test_reference_sample_equals_oracle(case):
    M.check_tokens(_ref_full(case, M.ln_min_p(case)), case)


@pytest.mark.parametrize("case", M.SHARD_CASES + M.TP_CASES, ids=lambda c: c.name)
def test_reference_candidates_equal_oracle(case):
    got = _ref_cand(case, M.ln_min_p(case))
    M.check_tokens(got, case)
    assert got.tolist() == _ref_full(case, M.ln_min_p(case)).tolist()


@pytest.mark.parametrize("case", S.ALL_CASES, ids=lambda c: c.name)
def test_no_floor_is_todays_sampler(case):
    """ln_min_p = None and an all -inf lane give the tokens of the sampler without the argument, on its own cases."""
    inp = S.inputs(case)
    off = np.full(S.B_ROWS, -np.inf, dtype=np.float32)
    if case.cand:
        vl = case.width // case.shards if case in S.TP_CASES else -(-case.width // case.shards)
        packs = torch.cat([R.cand_topk(inp.logits[:, r * vl:(r + 1) * vl], r * vl, case.V, inp.temp, inp.topk, 64,
                                       128) for r in range(case.shards)], -1)
        args = (packs, case.shards, 128, inp.temp, inp.topk, inp.topp, inp.seeds, case.V)
        today = R.sample_cand(*args)
        assert R.sample_cand(*args, ln_min_p=None).tolist() == today.tolist()
        assert R.sample_cand(*args, ln_min_p=off).tolist() == today.tolist()
    else:
        args = (inp.logits[:, :case.V], inp.temp, inp.topk, inp.topp, inp.seeds)
        today = R.sample(*args)
        assert R.sample(*args, ln_min_p=None).tolist() == today.tolist()
        assert R.sample(*args, ln_min_p=off).tolist() == today.tolist()
    S.check_tokens(today.numpy(), case)


# ------------------------------------------------------------------------------------------ special rows
@pytest.mark.parametrize("kind", list(M.BND_KINDS))
def test_boundary_rows(kind):
    """A token exactly on the floor is kept (it wins rows 0-5), the next bf16 value below is cut (it would have won
    rows 12-17)."""
    want = M.boundary_oracle(kind)
    scan = M.boundary_scan(kind, M.BND_SEEDS[kind])
    assert want[:6].tolist() == [M.BND_TOK_KEPT] * 6 and want[6:12].tolist() == [M.BND_TOK_MAX] * 6
    assert [w for _, _, w in scan[12:]] == [M.BND_TOK_CUT] * 6 and M.BND_TOK_CUT not in want.tolist()
    n = len(want)
    seeds = np.array(M.BND_SEEDS[kind], dtype=np.int64)
    for dtype, V in ((torch.bfloat16, 1000), (torch.float32, 1000), (torch.bfloat16, 50257)):
        x = M.boundary_rows(kind, V, dtype).float()
        got = R.sample(x, np.ones(n, np.float32), np.zeros(n, np.int32), np.ones(n, np.float32), seeds,
                       ln_min_p=np.full(n, M.BND_LN, np.float32))
        assert got.tolist() == want.tolist()


def test_tied_maxima_min_p_one():
    toks, dec = M.tie_oracle()
    assert 1.0 - dec.mean() <= M.MAX_UNDECIDABLE
    assert M.tie_chi2(toks) < S.chi2_bound(len(M.TIE_TOKENS) - 1)
    assert M.tie_chi2(np.where(np.arange(M.TIE_N) % 10 == 0, M.TIE_TOKENS[0], toks)) > S.chi2_bound(3)  # it notices
    n = 256
    x = M.tie_row()[None, :].float().repeat(n, 1)
    got = R.sample(x, np.ones(n, np.float32), np.zeros(n, np.int32), np.ones(n, np.float32), np.arange(n),
                   ln_min_p=np.zeros(n, np.float32)).numpy()
    assert got[dec[:n]].tolist() == toks[:n][dec[:n]].tolist()
    # greedy rows with the same lane ignore it: the lowest index of the maxima, not a drawn one
    got = R.sample(x[:8], np.zeros(8, np.float32), np.zeros(8, np.int32), np.ones(8, np.float32), np.arange(8),
                   ln_min_p=np.zeros(8, np.float32))
    assert got.tolist() == [M.TIE_TOKENS[0]] * 8


def test_all_inf_row():
    x = torch.full((2, 1000), float("-inf"))
    for lane in (np.full(2, -2.0, np.float32), np.full(2, -np.inf, np.float32)):
        got = R.sample(x, np.ones(2, np.float32), np.array([0, 40], np.int32), np.array([1.0, 0.9], np.float32),
                       np.array([3, 4]), ln_min_p=lane)
        assert got.tolist() == [0, 0]
    assert M.oracle_row(x[0].numpy(), 1.0, 0, 1.0, 3, S.eps_v3, -2.0)[:2] == (0, True)


@pytest.mark.parametrize("k,p,t,min_p", M.DIST_PARAMS)
def test_distribution_oracle_under_bound(k, p, t, min_p):
    toks, dec, kept, pr = M.dist_oracle(k, p, t, min_p, "consecutive")
    toks0, _, kept0, _ = S.dist_oracle(k, p, t, "consecutive")
    assert 1 < kept.size < kept0.size and set(kept) < set(kept0)  # the floor binds inside top-k / top-p
    assert 1.0 - dec.mean() <= M.MAX_UNDECIDABLE
    assert S.chi2_stat(toks, kept, pr) < S.chi2_bound(kept.size - 1)
    assert S.chi2_stat(toks0, kept, pr) == float("inf")  # the draws without the floor leave the kept set
    n = 256
    got = R.sample(S.dist_row()[None, :].float().repeat(n, 1), np.full(n, t, np.float32), np.full(n, k, np.int32),
                   np.full(n, p, np.float32), S.dist_seeds("consecutive")[:n],
                   ln_min_p=np.repeat(M.ln_of(min_p), n)).numpy()
    assert got[dec[:n]].tolist() == toks[:n][dec[:n]].tolist()


# ------------------------------------------------------------------------------------------ mutation checks
def _mutant_row(kind, row_full, V, t, k, p, seed, eps_fn, ln, ln_next, vl):
    """One row under a wrong definition of the floor. ``row_full``: the fp32 logits including padding columns."""
    x32 = S.scaled(row_full[:V], t, k)
    idx = np.flatnonzero(x32 > -np.inf)
    if idx.size == 0:
        return 0
    xs = x32[idx]
    x = xs.astype(np.float64)
    greedy = S.is_greedy(t, k)
    if greedy and kind != "greedy":
        return int(idx[np.argmax(x)])
    mx = np.float32(xs.max())
    floor_keep = xs >= np.float32(mx + np.float32(ln))
    if kind == "before-top-p":  # the nucleus of the distribution already cut by the floor
        idx, xs, x = idx[floor_keep], xs[floor_keep], x[floor_keep]
        floor_keep = np.ones(idx.size, dtype=bool)
    elif kind == "unscaled":  # the floor on the raw logits: temperature ignored
        raw = row_full[:V][idx].astype(np.float32)
        floor_keep = raw >= np.float32(np.float32(raw.max()) + np.float32(ln))
    elif kind == "strict":  # > instead of >=
        floor_keep = xs > np.float32(mx + np.float32(ln))
    elif kind == "padding":  # the maximum over the padding columns too
        allx = S.scaled(row_full, t, k)
        floor_keep = xs >= np.float32(np.float32(allx.max()) + np.float32(ln))
    elif kind == "absolute":  # p_i >= min_p instead of p_i >= min_p * p_max
        pr = np.exp(x - x.max())
        floor_keep = np.log(pr / pr.sum()) >= ln
    elif kind == "neighbour":  # the next row's lane
        floor_keep = xs >= np.float32(mx + np.float32(ln_next))
    elif kind == "first-shard":  # the maximum of the first shard's candidates only
        first = xs[idx < vl]
        floor_keep = xs >= np.float32(np.float32(first.max() if first.size else -np.inf) + np.float32(ln))
    if kind == "greedy" and greedy:  # the floor's kept set sampled on a greedy row: ties no longer go to the lowest id
        keep = floor_keep
    else:
        _, _, loose = S.thresholds(x, k, p, V, eps_fn)
        keep = (x >= loose) & floor_keep
    if not keep.any():
        return 0
    v = x[keep] + S.gumbel(idx[keep], seed)
    return int(idx[keep][np.argmax(v)])


def _mutant_tokens(kind, case):
    inp = M.inputs(case)
    rows = inp.logits.float().numpy()
    lane = M.ln_min_p(case)
    return np.array([_mutant_row(kind, rows[b], case.V, float(inp.temp[b]), int(inp.topk[b]), float(inp.topp[b]),
                                 int(inp.seeds[b]), M.EPS[case.eps], float(lane[b]), float(lane[(b + 1) % M.B_ROWS]),
                                 _vl(case) if case.cand else case.V) for b in range(M.B_ROWS)])


@pytest.mark.parametrize("kind,cases", [
    ("before-top-p", M.FULL_ROW_CASES[:4]), ("unscaled", M.FULL_ROW_CASES[:4]), ("strict", M.FULL_ROW_CASES[:4]),
    ("padding", [c for c in M.ALL_CASES if c.width > c.V]), ("absolute", M.FULL_ROW_CASES[:4]),
    ("neighbour", M.FULL_ROW_CASES[:4]), ("first-shard", M.SHARD_CASES + M.TP_CASES)])
def test_wrong_definitions_fail_a_decidable_row(kind, cases):
    failed = 0
    for case in cases:
        want, dec = M.oracle(case)
        failed += int((dec & (_mutant_tokens(kind, case) != want)).sum())
    assert failed >= 1, kind


def test_right_definition_passes_the_mutation_harness():
    """The harness itself: with no mutation it reproduces the oracle, so a failure above is the mutation's."""
    for case in (M.FULL_ROW_CASES[0], M.SHARD_CASES[2]):
        want, dec = M.oracle(case)
        assert _mutant_tokens("none", case)[dec].tolist() == want[dec].tolist()


def test_floor_on_greedy_ties_fails():
    """Greedy rows with tied maxima and a finite lane: the definition draws the lowest id; a sampler that let the
    floor's kept set (the tied maxima) go through Gumbel-max would not."""
    row = M.tie_row().float().numpy()
    got = [_mutant_row("greedy", row, M.TIE_V, 0.0, 0, 1.0, s, S.eps_v3, 0.0, 0.0, M.TIE_V) for s in range(16)]
    want = [M.oracle_row(row, 0.0, 0, 1.0, s, S.eps_v3, 0.0)[0] for s in range(16)]
    assert want == [M.TIE_TOKENS[0]] * 16 and got != want


# ------------------------------------------------------------------------------------------ Hugging Face
def test_kept_set_equals_hugging_face_min_p_warper():
    from transformers.generation.logits_process import MinPLogitsWarper

    case = M.FULL_ROW_CASES[0]
    inp = M.inputs(case)
    rows = inp.logits[:, :case.V].float().numpy()
    checked = 0
    for b in range(M.B_ROWS - 1):  # the last row is all -inf
        t, m = float(inp.temp[b]), float(M.min_ps(case)[b])
        if not t > 0 or m == 0:
            continue
        x32 = S.scaled(rows[b], t, 0)
        ln = float(M.ln_of(m)[0])
        fin = x32[x32 > -np.inf].astype(np.float64)
        near = np.abs(fin - (fin.max() + math.log(m))).min()
        if m < 1.0:
            assert near > 1e-4, (b, near)  # no token within 1e-4 nats of the floor: the kept set is beyond rounding
        ours = x32 >= M.floor_of(x32[x32 > -np.inf], ln)
        hf = MinPLogitsWarper(min_p=m)(None, torch.from_numpy(x32)[None, :].double())[0]
        assert np.array_equal(ours, torch.isfinite(hf).numpy()), b
        checked += 1
    assert checked >= 20


# ------------------------------------------------------------------------------------------ the request field
@pytest.mark.parametrize("bad", ["0.1", None, True, float("nan"), float("inf"), -0.01, 1.01, [0.1]])
def test_validate_rejects(bad):
    with pytest.raises(ValueError, match=r"Value of min_p should be a finite number in \[0, 1\]\."):
        SamplingParams(min_p=bad).validate()


def test_validate_accepts_and_has_min_p():
    for ok in (0, 0.0, 0.05, 1, 1.0, np.float32(0.25)):
        SamplingParams(min_p=ok).validate()
    assert not SamplingParams().has_min_p and not SamplingParams(min_p=0).has_min_p
    assert SamplingParams(min_p=0.05).has_min_p and SamplingParams(min_p=1.0).has_min_p
    assert SamplingParams(min_p="x").has_min_p  # so that add_request validates and rejects it


def test_k_ln_min_p():
    assert SamplingParams().k_ln_min_p == float("-inf")
    assert SamplingParams(min_p=0.0).k_ln_min_p == float("-inf")
    assert SamplingParams(min_p=0.3, is_greedy=True).k_ln_min_p == float("-inf")
    assert SamplingParams(min_p=1.0).k_ln_min_p == 0.0
    for m in (0.02, 0.05, 0.1, 0.5, 1e-30):
        v = SamplingParams(min_p=m).k_ln_min_p
        assert v == float(np.float32(math.log(m))) and np.float32(v) == v  # fp64 log, rounded to fp32 once
        assert v == float(M.ln_of(m)[0])
