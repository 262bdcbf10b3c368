"""The HIP constraint kernel (csrc/constraints.hip) against the fp64 oracle of tests/constraint_cases.py: the raw
bits of the whole output buffer, the bytes between the rows included, with the input and the state unchanged - and the
wrapper's rejections."""
import numpy as np
import pytest
import torch

import constraint_cases as C
from llmss_amd.engine.sampling import MAX_TOKEN_EDITS, SamplingParams, resolve_token_edits
from llmss_amd.ops import hip as H
from llmss_amd.ops import reference as R

pytestmark = pytest.mark.gpu
dev = "cuda"


def test_native_loaded():
    import llmss_amd

    assert H.lib().__file__.startswith(llmss_amd.__path__[0])
    assert hasattr(H.lib(), "apply_token_edits")


@pytest.mark.parametrize("name", C.CASE_NAMES)
def test_kernel_meets_oracle(name):
    C.run(C.cases()[name], H.apply_token_edits, resolve_token_edits, device=dev)


def _state(S=3, E=8, reqs=(), vocab=16):
    """Contiguous state tensors; ``reqs``: (slot, SamplingParams, eos)."""
    ids = torch.full((S, 2, E), -1, dtype=torch.int32)
    vals = torch.zeros(S, 2, E)
    meta = torch.zeros(S, 4, dtype=torch.int32)
    for s, p, eos in reqs:
        early, late, fill = resolve_token_edits(p, eos, vocab)
        i, v, m = R.pack_token_edits(early, late, fill, p.min_tokens, E)
        ids[s], vals[s], meta[s] = torch.from_numpy(i), torch.from_numpy(v), torch.from_numpy(m)
    return ids.to(dev), vals.to(dev), meta.to(dev)


def test_fresh_output_default_vocab_and_one_block_state():
    """out=None allocates; vocab=None takes lo + W; the three state tensors may be views of one [S, 4 E + 4] block, a
    slot's lists and meta side by side, as the engine keeps them."""
    E, S, W = 8, 3, 40
    g = torch.Generator().manual_seed(5)
    lg = (torch.randn(2, W, generator=g) * 4).to(torch.bfloat16)
    p = SamplingParams(max_new_tokens=4, logit_bias={39: 2.5, 0: -1.0}, banned_token_ids=[7], min_tokens=2,
                       stop_token_ids=[8]).validate()
    early, late, fill = resolve_token_edits(p, 3, W)
    i, v, m = R.pack_token_edits(early, late, fill, 2, E)
    block = torch.zeros(S, 4 * E + 4, dtype=torch.int32)
    block[2] = torch.from_numpy(np.concatenate([i.reshape(-1), v.reshape(-1).view(np.int32), m]))
    block = block.to(dev)
    ids = block[:, :2 * E].view(S, 2, E)
    vals = block[:, 2 * E:4 * E].view(torch.float32).view(S, 2, E)
    meta = block[:, 4 * E:]
    slots = torch.tensor([2, -1], dtype=torch.int32, device=dev)
    for nout in (1, 2):
        n = torch.full((2,), nout, dtype=torch.int32, device=dev)
        got = H.apply_token_edits(lg.to(dev), ids, vals, meta, slots, n)
        want = torch.stack([C.oracle_row(lg[0], p, 3, nout, 0, W), lg[1]])
        assert torch.equal(got.cpu().view(torch.int16), want.view(torch.int16))
    assert torch.isinf(want[0, 7]) and not torch.isinf(want[0, 8]) and not torch.isinf(want[0, 3])


def _args(B=2, W=16, S=3, E=8, dtype=torch.bfloat16):
    ids, vals, meta = _state(S, E)
    return dict(logits=torch.zeros(B, W, dtype=dtype, device=dev), edit_ids=ids, edit_vals=vals, edit_meta=meta,
                slots=torch.zeros(B, dtype=torch.int32, device=dev), nout=torch.zeros(B, dtype=torch.int32, device=dev))


@pytest.mark.parametrize("change", [
    dict(logits=lambda a: a["logits"].half()),
    dict(logits=lambda a: a["logits"].cpu()),
    dict(logits=lambda a: a["logits"].t().contiguous().t()),
    dict(logits=lambda a: a["logits"][:1].expand(2, 16)),
    dict(edit_ids=lambda a: a["edit_ids"].long()),
    dict(edit_ids=lambda a: a["edit_ids"].cpu()),
    dict(edit_ids=lambda a: a["edit_ids"][:, :, ::2]),
    dict(edit_ids=lambda a: a["edit_ids"][:, :1]),
    dict(edit_vals=lambda a: a["edit_vals"].double()),
    dict(edit_vals=lambda a: a["edit_vals"][:2]),
    dict(edit_vals=lambda a: a["edit_vals"][:1].expand(3, 2, 8)),
    dict(edit_meta=lambda a: a["edit_meta"][:, :3]),
    dict(edit_meta=lambda a: a["edit_meta"].long()),
    dict(slots=lambda a: a["slots"].long()),
    dict(slots=lambda a: a["slots"][:1]),
    dict(nout=lambda a: a["nout"].long()),
    dict(nout=lambda a: a["nout"].cpu()),
    dict(nout=lambda a: torch.zeros(4, dtype=torch.int32, device=dev)[::2]),
    dict(lo=lambda a: -1),
    dict(vocab=lambda a: -1),
    dict(out=lambda a: a["logits"]),
    dict(out=lambda a: torch.zeros(2, 40, dtype=torch.bfloat16, device=dev)[:, :16].as_strided((2, 16), (8, 1))),
    dict(out=lambda a: torch.zeros(2, 16, device=dev)),
    dict(out=lambda a: torch.zeros(2, 15, dtype=torch.bfloat16, device=dev)),
])
def test_apply_rejects(change):
    a = _args()
    a.update({k: f(a) for k, f in change.items()})
    with pytest.raises(ValueError):
        H.apply_token_edits(**a)


def test_out_may_not_overlap_logits_partially():
    buf = torch.zeros(2, 64, dtype=torch.bfloat16, device=dev)
    a = _args()
    a["logits"] = buf[:, :16]
    with pytest.raises(ValueError):
        H.apply_token_edits(**a, out=buf[:, 16:32])  # interleaved rows of one buffer share its address range


def test_slots_outside_the_state_copy():
    """A slot at or past the state's rows is treated as -1 (no read outside the state), list lengths are clamped to E."""
    a = _args()
    g = torch.Generator().manual_seed(2)
    a["logits"] = (torch.randn(2, 16, generator=g) * 4).to(torch.bfloat16).to(dev)
    a["slots"] = torch.tensor([3, 1], dtype=torch.int32, device=dev)
    a["edit_ids"][1, 1] = torch.arange(8, dtype=torch.int32, device=dev)
    a["edit_vals"][1, 1] = float("-inf")
    a["edit_meta"][1] = torch.tensor([0, MAX_TOKEN_EDITS * 4, 0, 0], dtype=torch.int32, device=dev)
    got = H.apply_token_edits(**a)
    assert torch.equal(got[0].view(torch.int16), a["logits"][0].view(torch.int16))
    assert torch.isinf(got[1, :8]).all() and torch.equal(got[1, 8:].view(torch.int16), a["logits"][1, 8:].view(torch.int16))
