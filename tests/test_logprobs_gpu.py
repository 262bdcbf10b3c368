"""The HIP log-probability kernels (csrc/logprobs.hip) against the fp64 oracle of tests/logprob_cases.py: values
within the derived bound, top-list ids exactly on every row."""
import pytest
import torch

import logprob_cases as L
from llmss_amd.ops import hip as H

pytestmark = pytest.mark.gpu
dev = "cuda"


def _nan_out(B, N):
    """NaN / -7 filled outputs as row-strided views of [B, 1 + N + 3] buffers: every entry must be written."""
    f = torch.full((B, 1 + N + 3), float("nan"), device=dev)
    i = torch.full((B, N + 3), -7, dtype=torch.int32, device=dev)
    return (f[:, 0], f[:, 1:1 + N], i[:, :N]), f, i


def test_native_loaded():
    import llmss_amd

    assert H.lib().__file__.startswith(llmss_amd.__path__[0])
    assert hasattr(H.lib(), "token_logprobs") and hasattr(H.lib(), "logprobs_combine")


@pytest.mark.parametrize("name", L.CASE_NAMES)
def test_kernel_meets_oracle(name):
    c = L.cases()[name]
    lg, tok = c.logits.to(dev), c.tokens.to(dev)
    for N in L.N_VALUES:
        out, f, i = _nan_out(c.B, N)
        got = H.token_logprobs(lg, c.V, tok, N, out=out)
        worst = L.check(c, N, *got, what="kernel")
        print(f"{name} N={N}: worst error {worst:.3f} x tol")
        assert torch.isnan(f[:, 1 + N:]).all() and (i[:, N:] == -7).all(), "wrote outside its outputs"
        again = H.token_logprobs(lg, c.V, tok, N)  # fresh contiguous outputs, same bits
        for a, b in zip(got, again):
            assert torch.equal(a.view(torch.int32) if a.dtype == torch.float32 else a,
                               b.view(torch.int32) if b.dtype == torch.float32 else b), "not bit-identical"


@pytest.mark.parametrize("shards", [2, 4, 8])
@pytest.mark.parametrize("name", L.SHARDABLE)
def test_partial_and_combine_meet_oracle(name, shards):
    c = L.cases()[name]
    lg, tok = c.logits.to(dev), c.tokens.to(dev)
    local = lg[:, :c.V] if c.V % shards else lg  # a shard may also carry the padding columns
    for N in L.N_VALUES:
        pack = H.token_logprobs_partial(local, 0, c.V, tok, N, shards=shards)
        out, f, i = _nan_out(c.B, N)
        got = H.token_logprobs_combine(pack, N, out=out)
        L.check(c, N, *got, what=f"{shards} shards")
        pack2 = H.token_logprobs_partial(local, 0, c.V, tok, N, shards=shards)
        assert torch.equal(pack.view(torch.int32), pack2.view(torch.int32)), "packs not bit-identical"
        full = H.token_logprobs(lg, c.V, tok, N)
        assert torch.equal(got[2], full[2])


def test_rank_shards_with_offsets():
    """Two ranks' own shards (lo > 0, the second one carrying the padding) gathered rank-major."""
    c = L.cases()["v50257-pad50304-bf16"]
    lg, tok = c.logits.to(dev), c.tokens.to(dev)
    half = c.ld // 2
    packs = [H.token_logprobs_partial(lg[:, r * half:(r + 1) * half], r * half, c.V, tok, 5) for r in (0, 1)]
    L.check(c, 5, *H.token_logprobs_combine(torch.cat(packs, dim=1), 5), what="2 ranks")


def test_row_strided_logits():
    c = L.cases()["v101-pad112-bf16"]
    wide = torch.full((c.B, 2 * c.ld + 8), L.PAD, dtype=c.logits.dtype, device=dev)
    wide[:, :c.ld] = c.logits.to(dev)
    L.check(c, 5, *H.token_logprobs(wide[:, :c.ld], c.V, c.tokens.to(dev), 5), what="strided")
    odd = torch.full((c.B, c.ld + 3), L.PAD, dtype=c.logits.dtype, device=dev)  # rows not 16-B aligned
    odd[:, :c.ld] = c.logits.to(dev)
    L.check(c, 5, *H.token_logprobs(odd[:, :c.ld], c.V, c.tokens.to(dev), 5), what="unaligned rows")


def test_wrapper_validation():
    c = L.cases()["v101-pad112-bf16"]
    lg, tok = c.logits.to(dev), c.tokens.to(dev)
    bad = [
        lambda: H.token_logprobs(lg, c.V, tok, 21),
        lambda: H.token_logprobs(lg, c.V, tok, -1),
        lambda: H.token_logprobs(lg, c.ld + 1, tok, 5),
        lambda: H.token_logprobs(lg, 0, tok, 5),
        lambda: H.token_logprobs(lg.half(), c.V, tok, 5),
        lambda: H.token_logprobs(lg.cpu(), c.V, tok, 5),
        lambda: H.token_logprobs(lg.t().contiguous().t(), c.V, tok, 5),
        lambda: H.token_logprobs(lg, c.V, tok.int(), 5),
        lambda: H.token_logprobs(lg, c.V, tok[:-1], 5),
        lambda: H.token_logprobs(lg, c.V, tok.cpu(), 5),
        lambda: H.token_logprobs(lg, c.V, tok.view(-1, 1), 5),
        lambda: H.token_logprobs(lg, c.V, tok, 5, out=(torch.empty(c.B, device=dev), torch.empty(c.B, 4, device=dev),
                                                        torch.empty(c.B, 5, dtype=torch.int32, device=dev))),
        lambda: H.token_logprobs_partial(lg, 0, c.V, tok, 5, shards=0),
        lambda: H.token_logprobs_partial(lg, 0, c.V, tok, 5, out=torch.empty(c.B, 12, device=dev)),
        lambda: H.token_logprobs_combine(torch.empty(c.B, 14, device=dev), 5),
        lambda: H.token_logprobs_combine(torch.empty(c.B, 13, device=dev).double(), 5),
    ]
    for i, f in enumerate(bad):
        with pytest.raises(ValueError):
            f()
            pytest.fail(f"call {i} was accepted")
    torch.cuda.synchronize()
