"""The HIP sampler (csrc/sampling.hip) against the fp64 oracle of tests/sampler_cases.py, token for token: every
dispatch of launch_sample by shape and dtype, the candidate path (cand_topk + sample_cand) by shards of one GPU and
by per-rank packs, the rows whose Philox word maps to the last uniform value, and the drawn distribution under
top-k / top-p / temperature. tests/test_sampler_oracle_cpu.py holds the CPU definition to the same cases."""
import numpy as np
import pytest
import torch

import sampler_cases as S

pytestmark = pytest.mark.gpu


def _dev():
    return torch.device("cuda")


def _sample_twice(H, logits, params, vocab):
    """H.sample with out2, and once more: (tokens) after asserting out2 == out and that the repeat is identical."""
    B = logits.shape[0]
    out2 = torch.full((B,), -1, dtype=torch.int64, device=logits.device)
    got = H.sample(logits, *params, vocab=vocab, out2=out2)
    assert torch.equal(out2, got)
    assert torch.equal(H.sample(logits, *params, vocab=vocab), got)  # TP ranks rely on identical draws
    return got.cpu().numpy()


@pytest.mark.parametrize("case", S.FULL_ROW_CASES, ids=lambda c: c.name)
def test_sample_equals_oracle(case):
    from llmss_amd.ops import hip as H

    inp = S.inputs(case)
    logits = inp.logits.to(_dev())
    assert logits.stride(0) == case.width and logits.data_ptr() % 16 == 0
    assert S.dispatch(case.V, logits.stride(0), case.dtype) == case.kernel
    got = _sample_twice(H, logits, inp.params(_dev()), case.V if case.V < case.width else None)
    assert int(got.max()) < case.V and int(got.min()) >= 0
    S.check_tokens(got, case)


@pytest.mark.parametrize("case", S.SHARD_CASES, ids=lambda c: c.name)
def test_sharded_candidates_equal_oracle(case):
    from llmss_amd.ops import hip as H

    inp = S.inputs(case)
    logits = inp.logits.to(_dev())
    temp, topk, topp, seeds = inp.params(_dev())
    pack = H.cand_topk(logits, 0, case.V, temp, topk, shards=case.shards)
    assert pack.shape == (S.B_ROWS, case.shards * 2 * H.CAND_KC)
    out2 = torch.full((S.B_ROWS,), -1, dtype=torch.int64, device=_dev())
    got = H.sample_cand(pack, H.CAND_KC, temp, topk, topp, seeds, out2=out2)
    assert torch.equal(out2, got)
    assert torch.equal(H.sample_cand(H.cand_topk(logits, 0, case.V, temp, topk, shards=case.shards), H.CAND_KC,
                                     temp, topk, topp, seeds), got)
    S.check_tokens(got.cpu().numpy(), case)


class _FakeGather:
    """In-process stand-in for the TP group: all_gather_last_dim over precomputed per-rank packs."""

    def __init__(self, packs):
        self.packs = packs

    def all_gather_last_dim(self, _):
        return torch.cat(self.packs, -1)


@pytest.mark.parametrize("case", S.TP_CASES, ids=lambda c: c.name)
def test_distributed_candidates_equal_oracle(case):
    from llmss_amd import ops
    from llmss_amd.ops import hip as H

    inp = S.inputs(case)
    logits = inp.logits.to(_dev())
    temp, topk, topp, seeds = inp.params(_dev())
    tp = case.shards
    vl = case.width // tp
    assert vl * tp == case.width
    packs = [H.cand_topk(logits[:, r * vl:(r + 1) * vl].contiguous(), r * vl, case.V, temp, topk) for r in range(tp)]
    for rank in (0, tp - 1):  # what the first and the last rank compute from the same gathered packs
        local = logits[:, rank * vl:(rank + 1) * vl].contiguous()
        got = ops.sample_distributed(local, _FakeGather(packs), rank * vl, case.V, temp, topk, topp, seeds)
        S.check_tokens(got.cpu().numpy(), case)


# ------------------------------------------------------------------------------------------ u == 1
def _u1_params(topk):
    B = len(S.U1_PAIRS)
    seeds = torch.tensor([s for s, _ in S.U1_PAIRS], dtype=torch.int64, device=_dev())
    return (torch.ones(B, device=_dev()), torch.full((B,), topk, dtype=torch.int32, device=_dev()),
            torch.ones(B, device=_dev()), seeds)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["v3", "fallback-fp32"])
def test_u1_rows_full_row(dtype):
    """Token 0 at +5, the pair's token at -30 with a Philox word that maps to the last u, the rest at 0: unclamped,
    u == 1 gives the pair's token +inf noise. It must lose; the oracle's token (decidable, and more than 10 ahead
    of the pair's token) must be drawn."""
    from llmss_amd.ops import hip as H

    toks, dec, lead = S.u1_oracle(None, 0)
    assert bool(dec.all()) and bool((lead > 10.0).all())
    got = _sample_twice(H, S.u1_rows().to(dtype).to(_dev()), _u1_params(0), None)
    assert all(int(g) != tok for g, (_, tok) in zip(got, S.U1_PAIRS)), got
    assert got.tolist() == toks.tolist()


def test_u1_rows_candidate_path():
    """The same pairs with only 64 tokens finite and top-k 64, so the -30 token is among the candidates: token 0
    wins in the oracle, and must win in cand_topk + sample_cand and in the full-row kernel."""
    from llmss_amd.ops import hip as H

    toks, dec, lead = S.u1_oracle(64, 64)
    assert toks.tolist() == [0] * len(S.U1_PAIRS) and bool(dec.all()) and bool((lead > 10.0).all())
    logits = S.u1_rows(64).to(torch.bfloat16).to(_dev())
    temp, topk, topp, seeds = _u1_params(64)
    pack = H.cand_topk(logits, 0, S.U1_V, temp, topk, shards=8)
    ids = pack.view(len(S.U1_PAIRS), 8, 2, H.CAND_KC)[:, :, 1].reshape(len(S.U1_PAIRS), -1).view(torch.int32).cpu()
    for b, (_, tok) in enumerate(S.U1_PAIRS):
        assert tok in ids[b].tolist()  # the -30 token is a candidate
    assert H.sample_cand(pack, H.CAND_KC, temp, topk, topp, seeds).tolist() == [0] * len(S.U1_PAIRS)
    assert _sample_twice(H, logits, (temp, topk, topp, seeds), None).tolist() == [0] * len(S.U1_PAIRS)


# ------------------------------------------------------------------------------------------ distribution
@pytest.mark.parametrize("family", S.DIST_FAMILIES)
@pytest.mark.parametrize("k,p,t", S.DIST_PARAMS)
def test_distribution_under_filters(k, p, t, family):
    """DIST_N draws of one 64-token row: the tokens are the oracle's on every decidable draw, and the counts pass
    Pearson's chi-square against the exact renormalised probabilities of the kept set at the 1 - 1e-6 quantile. The
    draws are a fixed function of the seeds; the CPU file shows the oracle's own tokens are under the bound."""
    from llmss_amd.ops import hip as H

    toks, dec, kept, pr = S.dist_oracle(k, p, t, family)
    assert 1.0 - dec.mean() <= S.MAX_UNDECIDABLE
    N = S.DIST_N
    logits = S.dist_row()[None, :].repeat(N, 1).contiguous().to(_dev())
    params = (torch.full((N,), t, device=_dev()), torch.full((N,), k, dtype=torch.int32, device=_dev()),
              torch.full((N,), p, device=_dev()), torch.from_numpy(S.dist_seeds(family)).to(_dev()))
    got = _sample_twice(H, logits, params, None)
    bad = np.flatnonzero(dec & (got != toks))
    assert bad.size == 0, (bad[:8].tolist(), got[bad[:8]].tolist(), toks[bad[:8]].tolist())
    stat, bound = S.chi2_stat(got, kept, pr), S.chi2_bound(kept.size - 1)
    print(f"chi2 {stat:.1f} bound {bound:.1f} dof {kept.size - 1} undecidable {(~dec).sum()}")
    assert stat < bound, (stat, bound)
