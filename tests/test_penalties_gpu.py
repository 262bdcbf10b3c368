"""The HIP penalty kernels (csrc/penalties.hip) against the fp64 oracle of tests/penalty_cases.py - exact cases bit
for bit, general ones within the derived bound - and the wrapper's rejections."""
import pytest
import torch

import penalty_cases as P
from llmss_amd.ops import hip as H

pytestmark = pytest.mark.gpu
dev = "cuda"


def test_native_loaded():
    import llmss_amd

    assert H.lib().__file__.startswith(llmss_amd.__path__[0])
    assert hasattr(H.lib(), "apply_penalties") and hasattr(H.lib(), "penalty_reset")


@pytest.mark.parametrize("name", P.CASE_NAMES)
def test_kernel_meets_oracle(name):
    worst = P.run(P.cases()[name], H.apply_penalties, H.penalty_reset, device=dev)
    print(f"{name}: worst error {worst:.3f} x bound")


def test_fresh_output_and_default_vocab():
    """out=None allocates; vocab=None takes the state's width; the same call twice registers twice."""
    g = torch.Generator().manual_seed(5)
    lg = (torch.randint(-255, 256, (2, 40), generator=g).float() / 8).to(torch.bfloat16).to(dev)
    st = torch.zeros(3, 40, dtype=torch.int32, device=dev)
    slots = torch.tensor([2, 0], dtype=torch.int32, device=dev)
    tok = torch.tensor([39, 0], device=dev)
    one = torch.ones(2, device=dev)
    a = H.apply_penalties(lg, st, slots, tok, one, one, one)
    b = H.apply_penalties(lg, st, slots, tok, one, one, one)
    want = lg.float()
    want[0, 39] -= 2
    want[1, 0] -= 2
    assert torch.equal(a.float(), want.bfloat16().float())
    want[0, 39] -= 1
    want[1, 0] -= 1
    assert torch.equal(b.float(), want.bfloat16().float())
    assert st.sum().item() == 4 and st[2, 39].item() == 2 and st[0, 0].item() == 2 and not st[1].any()


def _args(B=2, W=16, V=16, S=3, dtype=torch.bfloat16):
    return dict(logits=torch.zeros(B, W, dtype=dtype, device=dev), state=torch.zeros(S, V, dtype=torch.int32, device=dev),
                slots=torch.zeros(B, dtype=torch.int32, device=dev), new_tokens=torch.zeros(B, dtype=torch.int64, device=dev),
                rep=torch.ones(B, device=dev), pres=torch.zeros(B, device=dev), freq=torch.zeros(B, device=dev))


@pytest.mark.parametrize("change", [
    dict(logits=lambda a: a["logits"].half()),
    dict(logits=lambda a: a["logits"].cpu()),
    dict(logits=lambda a: a["logits"].t().contiguous().t()),
    dict(logits=lambda a: a["logits"][:1].expand(2, 16)),
    dict(state=lambda a: a["state"].long()),
    dict(state=lambda a: a["state"].cpu()),
    dict(state=lambda a: a["state"][:, ::2]),
    dict(slots=lambda a: a["slots"].long()),
    dict(slots=lambda a: a["slots"][:1]),
    dict(new_tokens=lambda a: a["new_tokens"].int()),
    dict(rep=lambda a: a["rep"].double()),
    dict(pres=lambda a: a["pres"].cpu()),
    dict(freq=lambda a: torch.zeros(4, device=dev)[::2]),
    dict(vocab=lambda a: 17),
    dict(lo=lambda a: -1),
    dict(out=lambda a: a["logits"]),
    dict(out=lambda a: torch.zeros(2, 40, dtype=torch.bfloat16, device=dev)[:, :16].as_strided((2, 16), (8, 1))),
    dict(out=lambda a: torch.zeros(2, 16, device=dev)),
    dict(out=lambda a: torch.zeros(2, 15, dtype=torch.bfloat16, device=dev)),
])
def test_apply_rejects(change):
    a = _args()
    kw = {k: f(a) for k, f in change.items()}
    a.update(kw)
    with pytest.raises(ValueError):
        H.apply_penalties(**a)


def test_out_may_not_overlap_logits_partially():
    buf = torch.zeros(2, 64, dtype=torch.bfloat16, device=dev)
    a = _args()
    a["logits"] = buf[:, :16]
    with pytest.raises(ValueError):
        H.apply_penalties(**a, out=buf[:, 16:32])  # interleaved rows of one buffer share its address range


@pytest.mark.parametrize("change", [
    dict(state=lambda a: a["state"].long()),
    dict(slots=lambda a: a["slots"].long()),
    dict(cu=lambda a: a["cu"][:2]),
    dict(cu=lambda a: a["cu"].long()),
    dict(tokens=lambda a: a["tokens"].int()),
    dict(words=lambda a: a["words"][:1]),
    dict(words=lambda a: a["words"].cpu()),
])
def test_reset_rejects(change):
    a = dict(state=torch.zeros(3, 16, dtype=torch.int32, device=dev), slots=torch.zeros(2, dtype=torch.int32, device=dev),
             cu=torch.tensor([0, 1, 2], dtype=torch.int32, device=dev), tokens=torch.zeros(2, dtype=torch.int64, device=dev),
             words=torch.ones(2, dtype=torch.int32, device=dev))
    a.update({k: f(a) for k, f in change.items()})
    with pytest.raises(ValueError):
        H.penalty_reset(**a)


def test_zero_width_shard_registers_like_the_definition():
    """A shard without columns still registers its rows' tokens, as ops/reference.py does."""
    from llmss_amd.ops import reference as R

    st = torch.zeros(3, 16, dtype=torch.int32, device=dev)
    st[2, 5] = 3
    ref = st.cpu().clone()
    a = _args()
    a.update(logits=torch.zeros(2, 0, dtype=torch.bfloat16, device=dev), state=st,
             slots=torch.tensor([2, -1], dtype=torch.int32, device=dev), new_tokens=torch.tensor([5, 7], device=dev))
    out = H.apply_penalties(**a, lo=16)
    assert tuple(out.shape) == (2, 0)
    R.apply_penalties(torch.zeros(2, 0, dtype=torch.bfloat16), ref, a["slots"].cpu(), a["new_tokens"].cpu(),
                      a["rep"].cpu(), a["pres"].cpu(), a["freq"].cpu(), lo=16)
    assert torch.equal(st.cpu(), ref) and ref[2, 5].item() == 4 and ref.sum().item() == 4
