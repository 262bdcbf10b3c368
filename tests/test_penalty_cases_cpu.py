"""The CPU definition of the penalties (ops/reference.py through the ops dispatch) passes every case of
tests/penalty_cases.py, and each of a set of plausible wrong definitions fails at least one exact case - so the
cases can tell them apart."""
import numpy as np
import pytest
import torch

import penalty_cases as P
from llmss_amd import ops


@pytest.mark.parametrize("name", P.CASE_NAMES)
def test_reference_meets_oracle(name):
    c = P.cases()[name]
    worst = P.run(c, ops.apply_penalties, ops.penalty_reset)
    print(f"{name}: worst error {worst:.3f} x bound")


def test_case_shapes():
    cs = P.cases().values()
    assert {c.W for c in cs} >= set(P.WIDTHS) and {c.B for c in cs} >= {1, 3, 65}
    for c in cs:
        assert c.vocab <= c.W and c.ld > c.W and c.state_cols >= c.vocab
        held = c.slots[c.slots >= 0]
        assert len(set(held.tolist())) == held.size and (np.diff(held) < -1).all()
        assert c.B < 3 or (c.slots < 0).any()
        if not ("aligned" in c.name):
            assert c.ld % 8
        for b in range(c.B):
            assert max(c.outputs[b].count(t) for t in set(c.outputs[b])) <= 6
            assert set(c.outputs[b]) - set(c.prompts[b]) or c.vocab == 1
    assert any(c.vocab < c.W for c in cs) and any(c.nstates == 2 for c in cs)
    for kind in ("exact", "general"):
        for dn in ("bf16", "fp32"):
            for al in ("", "-aligned"):
                c = P.cases()[f"{kind}-{dn}-B6-W4131{al}"]
                held = [b for b in range(c.B) if c.slots[b] >= 0]
                new = [{int(step[0][3][b]) for step in c.steps} for b in range(c.B)]
                # a slotted row registers the last column of the first apply workgroup and the first of the second:
                # at the nominal edge, and at the edge shifted by the row's unaligned head
                assert any(new[b] == {P.GROUP_EDGE - 1, P.GROUP_EDGE} for b in held)
                assert any(new[b] == {P.edge_tokens(c, b) - 1, P.edge_tokens(c, b)} for b in held[2:])
                assert al or any(P.edge_tokens(c, b) != P.GROUP_EDGE for b in held[2:])
                # reset lists reach the second reset workgroup: tokens on both sides of state column RESET_EDGE
                assert c.vocab > P.RESET_EDGE + 9
                _, toks, _ = P.reset_lists(c)
                for b in held:
                    known = set(c.prompts[b]) | set(c.outputs[b])
                    assert {P.RESET_EDGE - 1, P.RESET_EDGE} & known and min(known) < P.RESET_EDGE <= max(known)
                    assert any(t >= P.RESET_EDGE for t in c.prompts[b]) and any(t >= P.RESET_EDGE for t in c.outputs[b])
                assert (toks >= P.RESET_EDGE).any() and (toks < P.RESET_EDGE).any()


# ------------------------------------------------------------------------------ wrong definitions
def _np_apply(bug):
    def apply(logits, state, slots, new_tokens, rep, pres, freq, lo, vocab, out):
        B, W = logits.shape
        S, cols = state.shape
        out.copy_(logits)
        n = max(0, min(W, vocab - lo))
        if bug == "padding":  # the state's width instead of the vocabulary
            n = max(0, min(W, cols - lo))
        for b in range(B):
            s = int(slots[b])
            if s < 0 and bug != "minus_one_row":
                continue
            if bug == "neighbour":
                s = (s + 1) % S
            t = int(new_tokens[b])
            if 0 <= t < vocab and bug != "missed_registration":
                state[s, t] += 2 if bug == "doubled_registration" else 1
            shift = 1 if bug == "lo_off_by_one" else 0
            w = np.zeros(n, dtype=np.int64)
            src = state[s].numpy().astype(np.int64)[lo + shift:lo + shift + n]
            w[:src.size] = src
            flag, c = w < 0, w & 0x7FFFFFFF
            seen = (c > 0) if bug == "rep_ignores_prompt" else (flag | (c > 0))
            if bug == "pf_count_prompt":
                c = c + flag
            x = logits[b, :n].float().numpy().astype(np.float32)
            r, p, f = (np.float32(v[b]) for v in (rep, pres, freq))
            times = np.where(seen, np.maximum(c, 1) if bug == "rep_per_occurrence" else 1, 0)
            with np.errstate(invalid="ignore"):
                for k in range(int(times.max()) if n else 0):
                    on = times > k
                    pos = (x > 0) | (bug == "divide_negative")
                    x = np.where(on, np.where(pos, x / r, x * r), x).astype(np.float32)
                x = np.where(c > 0, x - (f * c.astype(np.float32) + p), x).astype(np.float32)
            y = torch.from_numpy(x).to(out.dtype)
            touched = torch.from_numpy(seen | (c > 0))
            out[b, :n] = torch.where(touched, y, logits[b, :n])
        return out
    return apply


def _np_reset(bug):
    def reset(state, slots, cu, tokens, words):
        for i in range(slots.shape[0]):
            s = int(slots[i])
            if s < 0:
                continue
            if bug != "stale_reset":
                state[s].zero_()
            a, b = int(cu[i]), int(cu[i + 1])
            state[s, tokens[a:b]] = words[a:b]
        return state
    return reset


def test_numpy_definition_meets_every_case():
    """The mutants' common base (no bug switched on) is right, so each failure below is the bug's."""
    for name in P.CASE_NAMES:
        P.run(P.cases()[name], _np_apply(None), _np_reset(None))


BUGS = ("pf_count_prompt", "rep_ignores_prompt", "rep_per_occurrence", "divide_negative", "missed_registration",
        "doubled_registration", "lo_off_by_one", "padding", "minus_one_row", "neighbour", "stale_reset")


@pytest.mark.parametrize("bug", BUGS)
def test_wrong_definition_fails_an_exact_case(bug):
    failed = []
    for name in P.EXACT_NAMES:
        try:
            P.run(P.cases()[name], _np_apply(bug), _np_reset(bug))
        except AssertionError:
            failed.append(name)
    print(f"{bug}: fails {len(failed)} of {len(P.EXACT_NAMES)} exact cases")
    assert failed, f"no exact case notices the wrong definition {bug!r}"
