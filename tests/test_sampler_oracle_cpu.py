"""The sampler's CPU definition (ops/reference.py) against the fp64 oracle of tests/sampler_cases.py, on the
very cases tests/test_sampler_oracle_gpu.py gives the HIP kernels - plus the pieces both stand on: Philox pinned
against a scalar implementation, the uniform mapping checked on all 2^24 inputs, and the oracle's own checks
shown to notice a wrong draw."""
import numpy as np
import pytest
import torch

import sampler_cases as S
from llmss_amd.ops import reference as R


# ------------------------------------------------------------------------------------------ Philox
def _philox_scalar(c0: int, k0: int, k1: int) -> int:
    """Philox-4x32-10 (Salmon et al., SC'11), counter (c0, 0, 0, 0), key (k0, k1): first output word."""
    M = 0xFFFFFFFF
    c = [c0 & M, 0, 0, 0]
    for _ in range(10):
        p0, p1 = 0xD2511F53 * c[0], 0xCD9E8D57 * c[2]
        c = [(p1 >> 32) ^ c[1] ^ k0, p1 & M, (p0 >> 32) ^ c[3] ^ k1, p0 & M]
        k0, k1 = (k0 + 0x9E3779B9) & M, (k1 + 0xBB67AE85) & M
    return c[0]


def _philox_pairs():
    rng = np.random.default_rng(7)
    ctr = [0, 1, 2, 31399, 50256, 2 ** 31 - 1, 2 ** 31, 2 ** 32 - 1] + rng.integers(0, 2 ** 32, 24).tolist()
    keys = [0, 1, 247, 2 ** 32 - 1, 2 ** 63, 2 ** 64 - 1] + rng.integers(0, 2 ** 64, 10, dtype=np.uint64).tolist()
    pairs = [(ctr[i % len(ctr)], keys[i % len(keys)]) for i in range(48)]
    for i in range(8):  # keys that differ only in the upper 32 bits
        lo = int(rng.integers(0, 2 ** 32))
        pairs += [(ctr[i], lo | (i + 1) << 32), (ctr[i], lo | (i + 2) << 32)]
    return pairs


def test_philox_known_answer():
    """Random123's known-answer vectors for philox4x32-10 (all-zero, and all-ones counter and key), by the scalar
    implementation with a full counter - so the scalar code the other tests trust is Philox and not a lookalike."""
    def full(c, k):
        M = 0xFFFFFFFF
        c, k = list(c), list(k)
        for _ in range(10):
            p0, p1 = 0xD2511F53 * c[0], 0xCD9E8D57 * c[2]
            c = [(p1 >> 32) ^ c[1] ^ k[0], p1 & M, (p0 >> 32) ^ c[3] ^ k[1], p0 & M]
            k = [(k[0] + 0x9E3779B9) & M, (k[1] + 0xBB67AE85) & M]
        return c

    assert full([0] * 4, [0] * 2) == [0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8]
    assert full([0xFFFFFFFF] * 4, [0xFFFFFFFF] * 2) == [0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD]
    assert _philox_scalar(0, 0, 0) == 0x6627E8D5


def test_philox_matches_scalar():
    pairs = _philox_pairs()
    assert len(pairs) == 64
    for c, key in pairs:
        want = _philox_scalar(c, key & 0xFFFFFFFF, key >> 32)
        assert int(R.philox(np.array([c]), key)[0]) == want, (c, hex(key))
        assert int(S.philox(c, key)) == want, (c, hex(key))
        signed = key - 2 ** 64 if key >= 2 ** 63 else key  # the int64 the engine passes
        assert int(S.philox(np.array([c]), np.array([signed], dtype=np.int64))[0]) == want
    up = [_philox_scalar(5, 123, hi) for hi in range(16)]
    assert len(set(up)) == 16  # the upper key word matters


# ------------------------------------------------------------------------------------------ uniform mapping
def test_uniform_mapping_exhaustive():
    """All 2^24 values of r >> 8 through the fp32 mapping of ops/reference.py."""
    m = np.arange(1 << 24, dtype=np.uint64)
    u = R._gumbel_u(m << np.uint64(8))
    assert u.dtype == np.float32
    assert float(u.min()) > 0.0 and float(u.max()) < 1.0
    assert bool((np.diff(u) >= 0).all())
    g = -np.log(-np.log(u))
    assert bool(np.isfinite(g).all())
    # the oracle's integer definition is the same number, bit for bit
    assert np.array_equal(u.astype(np.float64), S.uniform(m))
    # and the low 8 bits of r do not take part
    assert np.array_equal(R._gumbel_u((m[:4096] << np.uint64(8)) | np.uint64(0xFF)), u[:4096])
    # DELTA's basis: fp32 logs against fp64 logs of the same u
    err = float(np.abs(g.astype(np.float64) - (-np.log(-np.log(u.astype(np.float64))))).max())
    assert err <= S.G_FP32_MAX_ERR * 1.001, err
    assert S.DELTA == 1000 * S.G_FP32_MAX_ERR


@pytest.mark.parametrize("seed,tok", S.U1_PAIRS)
def test_u1_pairs_hit_the_last_value(seed, tok):
    assert int(R.philox(np.array([tok]), seed)[0]) >> 8 == 0xFFFFFF
    assert int(S.philox(tok, seed)) >> 8 == 0xFFFFFF


# ------------------------------------------------------------------------------------------ oracle self-checks
def test_oracle_small_rows():
    """Rows small enough to decide by hand."""
    e = S.eps_v3
    x = np.array([1.0, 3.0, -np.inf, 3.0, 2.0], dtype=np.float32)
    assert S.oracle_row(x, 0.0, 0, 1.0, 5, e)[:2] == (1, True)          # greedy: lowest index of the maxima
    assert S.oracle_row(x, 1.0, 1, 1.0, 5, e)[:2] == (1, True)          # top-k 1 is greedy
    assert S.oracle_row(np.full(4, -np.inf, np.float32), 1.0, 0, 0.9, 5, e)[:2] == (0, True)
    xd = x[x > -np.inf].astype(np.float64)
    assert S.thresholds(xd, 2, 1.0, 5, e) == (3.0, 3.0, 3.0)
    assert S.thresholds(xd, 3, 1.0, 5, e)[0] == 2.0
    assert S.thresholds(xd, 5, 1.0, 5, e)[0] == -np.inf                 # k == V: no top-k
    # top-p: masses 1, 1, e^-1, e^-2 -> z = 2.503; p z = 1.25 is first reached by the second 3.0
    assert S.thresholds(xd, 0, 0.5, 5, e) == (-np.inf, 3.0, 3.0)
    # a target that sits on a cumulative sum exactly is ambiguous: strict and loose thresholds part
    z = 2.0 + np.exp(-1.0) + np.exp(-2.0)
    _, strict, loose = S.thresholds(xd, 0, 2.0 / z, 5, e)
    assert (strict, loose) == (3.0, 2.0)
    # tokens drawn only ever come from the kept set, whatever the seed
    for seed in range(200):
        tok, _, _ = S.oracle_row(x, 1.0, 2, 1.0, seed, e)
        assert tok in (1, 3)
    assert S.eps_fallback(50000) > S.eps_v3(50000) > 2e-6


def test_oracle_frequencies_small_row():
    """The oracle draws from the renormalised kept softmax: 20000 seeds on a 5-token row, top-k 3."""
    x = np.array([0.5, 2.0, 1.0, -1.0, 1.5], dtype=np.float32)
    kept = np.array([1, 2, 4])
    pr = np.exp(x[kept].astype(np.float64))
    pr /= pr.sum()
    n = 20000
    v = x[kept].astype(np.float64)[None, :] + S.gumbel(kept[None, :], np.arange(n, dtype=np.int64)[:, None] * 7919)
    counts = np.bincount(kept[np.argmax(v, 1)], minlength=5)[kept]
    stat = float(((counts - n * pr) ** 2 / (n * pr)).sum())
    assert stat < S.chi2_bound(2), (counts, n * pr)


def test_chi2_bound_forms_agree():
    from statistics import NormalDist

    z = NormalDist().inv_cdf(1.0 - 1e-6)
    for dof in (9, 19, 63):
        wh = dof * (1.0 - 2.0 / (9.0 * dof) + z * (2.0 / (9.0 * dof)) ** 0.5) ** 3
        # scipy's exact quantile (if present) against Wilson-Hilferty, which this far out in the tail is 2.6 % high
        # at 9 degrees of freedom and closer above
        assert abs(S.chi2_bound(dof) - wh) / wh < 0.03


def test_cases_cover_every_dispatch():
    for c in S.FULL_ROW_CASES:
        assert S.dispatch(c.V, c.width, c.dtype) == c.kernel, c.name
    assert {c.kernel for c in S.FULL_ROW_CASES} == {"v3<2,false>", "v3<4,false>", "v3<8,true>",
                                                     "sample_kernel<bf16>", "sample_kernel<float>"}
    assert len({c.name for c in S.ALL_CASES}) == len(S.ALL_CASES)
    for c in S.ALL_CASES:
        inp = S.inputs(c)
        assert inp.logits.shape == (S.B_ROWS, c.width)
        assert bool((inp.logits[:, c.V:] == S.PAD_LOGIT).all())
        assert bool(torch.isinf(inp.logits[-1, :c.V]).all())
        assert int(inp.seeds.min()) < 0 < int(inp.seeds.max())
        if c.cand:
            assert bool(((inp.topk >= 1) & (inp.topk <= 64)).all())


# ------------------------------------------------------------------------------------------ definition vs oracle
@pytest.mark.parametrize("case", S.FULL_ROW_CASES, ids=lambda c: c.name)
def test_reference_sample_equals_oracle(case):
    inp = S.inputs(case)
    got = R.sample(inp.logits[:, :case.V], inp.temp, inp.topk, inp.topp, inp.seeds)
    S.check_tokens(got.numpy(), case)


@pytest.mark.parametrize("case", S.SHARD_CASES + S.TP_CASES, ids=lambda c: c.name)
def test_reference_candidates_equal_oracle(case):
    inp = S.inputs(case)
    vl = case.width // case.shards if case in S.TP_CASES else -(-case.width // case.shards)
    assert vl * case.shards >= case.V
    packs = [R.cand_topk(inp.logits[:, r * vl:(r + 1) * vl], r * vl, case.V, inp.temp, inp.topk, 64, 128)
             for r in range(case.shards)]
    got = R.sample_cand(torch.cat(packs, -1), case.shards, 128, inp.temp, inp.topk, inp.topp, inp.seeds, case.V)
    S.check_tokens(got.numpy(), case)
    full = R.sample(inp.logits[:, :case.V], inp.temp, inp.topk, inp.topp, inp.seeds)
    assert got.tolist() == full.tolist()


def test_check_tokens_notices_one_wrong_row():
    case = S.FULL_ROW_CASES[0]
    want, dec = S.oracle(case)
    S.check_tokens(want, case)
    b = int(np.flatnonzero(dec & (S.inputs(case).temp > 0))[0])
    bad = want.copy()
    bad[b] = (bad[b] + 1) % case.V
    with pytest.raises(AssertionError):
        S.check_tokens(bad, case)


def test_oracle_tells_a_wrong_sampler():
    """What the GPU mutation check does to the kernels, done to the oracle's own noise: a key that drops the upper
    seed word, or a counter shifted by one, no longer passes check_tokens."""
    case = S.FULL_ROW_CASES[0]
    inp = S.inputs(case)
    rows = inp.logits[:, :case.V].float().numpy()
    for mutate in (lambda idx, seed: (idx, seed & 0xFFFFFFFF), lambda idx, seed: (idx + 1, seed)):
        got = []
        for b in range(S.B_ROWS):
            t, k, p = float(inp.temp[b]), int(inp.topk[b]), float(inp.topp[b])
            x = S.scaled(rows[b], t, k)
            idx = np.flatnonzero(x > -np.inf)
            if idx.size == 0 or S.is_greedy(t, k):
                got.append(S.oracle(case)[0][b])
                continue
            xd = x[idx].astype(np.float64)
            keep = xd >= S.thresholds(xd, k, p, case.V, S.eps_v3)[2]
            i2, s2 = mutate(idx[keep], int(inp.seeds[b]) & (2 ** 64 - 1))
            got.append(int(idx[keep][np.argmax(xd[keep] + S.gumbel(i2, s2))]))
        with pytest.raises(AssertionError):
            S.check_tokens(got, case)


# ------------------------------------------------------------------------------------------ u == 1
@pytest.mark.parametrize("finite,topk", [(None, 0), (64, 64)])
def test_u1_rows(finite, topk):
    """(seed, token) pairs whose Philox word maps to the last u. Unclamped, u == 1 gives that token +inf noise and
    it wins at logit -30. With the clamp its noise is 16.6, it loses by more than 10 whatever else happens, and the
    definition draws the oracle's token. (finite = 64: the row the GPU candidate path gets, top-k 64.)"""
    x = S.u1_rows(finite)
    toks, dec, lead = S.u1_oracle(finite, topk)
    assert bool(dec.all())
    assert bool((lead > 10.0).all()), lead
    B = len(S.U1_PAIRS)
    seeds = np.array([s for s, _ in S.U1_PAIRS], dtype=np.int64)
    got = R.sample(x, np.ones(B, np.float32), np.full(B, topk, np.int32), np.ones(B, np.float32), seeds)
    assert got.tolist() == toks.tolist()
    assert all(int(g) != tok for g, (_, tok) in zip(got, S.U1_PAIRS))
    if finite is not None:
        packs = [R.cand_topk(x[:, r * 4000:(r + 1) * 4000], r * 4000, S.U1_V, np.ones(B, np.float32),
                             np.full(B, topk, np.int32), 64, 128) for r in range(8)]
        ids = torch.cat([pk[:, 128:] for pk in packs], -1).contiguous().view(torch.int32)
        for b, (_, tok) in enumerate(S.U1_PAIRS):  # a shard with fewer than 64 finite logits keeps all of them
            assert tok in ids[b].tolist() and set(range(63)) <= set(ids[b].tolist())
        got = R.sample_cand(torch.cat(packs, -1), 8, 128, np.ones(B, np.float32), np.full(B, topk, np.int32),
                            np.ones(B, np.float32), seeds, S.U1_V)
        assert got.tolist() == toks.tolist()


def test_u1_token_zero_wins_when_it_leads():
    """The same four pairs with nothing but token 0 (+5) and the pair's token (-30) finite: token 0 leads by more
    than 30 in the oracle and must be drawn."""
    B = len(S.U1_PAIRS)
    x = torch.full((B, S.U1_V), float("-inf"))
    seeds = np.array([s for s, _ in S.U1_PAIRS], dtype=np.int64)
    for b, (seed, tok) in enumerate(S.U1_PAIRS):
        x[b, 0], x[b, tok] = 5.0, -30.0
        t, ok, lead = S.oracle_row(x[b].numpy(), 1.0, 0, 1.0, seed, S.eps_v3)
        assert (t, ok) == (0, True) and lead > 15.0, (t, ok, lead)
    got = R.sample(x, np.ones(B, np.float32), np.zeros(B, np.int32), np.ones(B, np.float32), seeds)
    assert got.tolist() == [0] * B


# ------------------------------------------------------------------------------------------ distribution
@pytest.mark.parametrize("family", S.DIST_FAMILIES)
@pytest.mark.parametrize("k,p,t", S.DIST_PARAMS)
def test_distribution_oracle_under_bound(k, p, t, family):
    """The draws are a fixed function of the seeds: the oracle's own tokens pass the chi-square bound the GPU test
    uses, for these exact seeds, and nearly every draw is decidable."""
    toks, dec, kept, pr = S.dist_oracle(k, p, t, family)
    assert toks.size == S.DIST_N and abs(pr.sum() - 1.0) < 1e-12
    assert 1.0 - dec.mean() <= S.MAX_UNDECIDABLE
    if k:
        assert kept.size <= k
    stat = S.chi2_stat(toks, kept, pr)
    assert stat < S.chi2_bound(kept.size - 1), (stat, S.chi2_bound(kept.size - 1), kept.size)
    # the statistic does notice a shifted distribution: move 10 % of the draws onto the most likely token
    moved = toks.copy()
    moved[: S.DIST_N // 10] = kept[0]
    assert S.chi2_stat(moved, kept, pr) > S.chi2_bound(kept.size - 1)
    # the definition draws the same tokens
    logits = S.dist_row()[None, :].float().repeat(256, 1)
    seeds = S.dist_seeds(family)[:256]
    got = R.sample(logits, np.full(256, t, np.float32), np.full(256, k, np.int32), np.full(256, p, np.float32), seeds)
    d = dec[:256]
    assert got.numpy()[d].tolist() == toks[:256][d].tolist()
