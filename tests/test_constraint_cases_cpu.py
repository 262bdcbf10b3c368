"""The CPU definition of the token constraints (ops/reference.py through the ops dispatch, resolve_token_edits of
engine/sampling.py) passes every case of tests/constraint_cases.py bit for bit, each of a set of plausible wrong
definitions fails at least one case - so the cases can tell them apart - and resolve_token_edits meets hand-written
expectations."""
import pickle

import numpy as np
import pytest
import torch

import constraint_cases as C
from llmss_amd import ops
from llmss_amd.engine.sampling import MAX_TOKEN_EDITS, SamplingParams, resolve_token_edits

NINF = float("-inf")


@pytest.mark.parametrize("name", C.CASE_NAMES)
def test_reference_meets_oracle(name):
    C.run(C.cases()[name], ops.apply_token_edits, resolve_token_edits)


def test_case_shapes():
    cs = list(C.cases().values())
    assert {c.W for c in cs} >= set(C.WIDTHS) | {0} and {c.B for c in cs} >= {1, 3, 65}
    assert {c.dtype for c in cs} == {torch.bfloat16, torch.float32}
    assert any(c.vocab < c.lo + c.W for c in cs) and any(c.lo > 0 for c in cs)
    assert any(c.off != c.ooff for c in cs) and any(c.off == c.ooff == 0 and c.ld % 8 == 0 for c in cs)
    lens, active, kinds = set(), set(), set()
    for c in cs:
        checked = False
        held = c.slots[c.slots >= 0]
        assert len(set(held.tolist())) == held.size and (c.B < 2 or (np.diff(held) < -1).all())  # apart, descending
        assert c.B < 3 or (c.slots < 0).any()
        if "aligned" not in c.name and "rounding" not in c.name:
            assert c.ld % 2 == 1
        assert c.B < 3 or {int(n) - C.MIN_TOKENS for n in c.nout} == {-1, 0, 1} or "rounding" in c.name
        for b in range(c.B):
            s = int(c.slots[b])
            if s < 0:
                continue
            p = c.reqs[s]
            early, late, fill = resolve_token_edits(p, c.eos[s], c.vocab)
            lens |= {len(early), len(late)}
            active.add(len(early) if c.nout[b] < p.min_tokens else len(late))
            kinds.add((fill, bool(p.logit_bias)))
            if "rounding" in c.name or c.W == 0 or checked:
                continue
            listed = {t for t, _ in late} | {t for t, _ in early}
            if not fill and p.logit_bias:  # the first bias-only row of every case lists every seam of its own row
                edges = {c.lo + j for j in C.chunk_edges(c, b) if c.lo + j < c.vocab}
                assert edges <= listed, (c.name, b, sorted(edges - listed))
                assert c.vocab - 1 in listed or not c.lo <= c.vocab - 1 < c.lo + c.W
                if c.lo > 0:
                    assert min(listed) < c.lo and (max(listed) >= c.lo + c.W or c.lo + c.W >= c.vocab)
                # a finite bias over a -inf logit
                assert any(torch.isinf(c.base[b, c.off + t - c.lo]) for t in p.logit_bias if c.lo <= t < c.lo + c.W)
                checked = True
    assert {0, 1, MAX_TOKEN_EDITS} <= lens and {0, 1, MAX_TOKEN_EDITS} <= active, (sorted(lens), sorted(active))
    assert kinds >= {(True, True), (True, False), (False, True), (False, False)}
    big = C.cases()["bf16-B8-W4099-long"]
    unit = 8
    assert {(b * big.ld + big.off) % unit for b in range(big.B)} == set(range(unit))  # every row phase
    assert len(C.chunk_edges(big, 0)) >= 6  # three chunks' first and last columns


# ------------------------------------------------------------------------------ wrong definitions
def _mut_resolve(bug):
    def resolve(p, eos, vocab):
        bias, banned, allowed = p.logit_bias, set(p.banned_token_ids), list(p.allowed_token_ids)
        fill = len(allowed) > 0
        if fill:
            late = {v: float(bias.get(v, 0.0)) for v in allowed if v not in banned or bug == "banned_allowed_kept"}
        else:
            late = {v: NINF if v in banned else float(bias[v]) for v in set(bias) | banned}
            if bug == "bias_beats_ban":
                late.update({v: float(a) for v, a in bias.items()})
        early = {}
        if p.min_tokens > 0:
            stop = set(p.stop_token_ids)
            if eos is not None and (not p.ignore_eos or bug == "ignore_eos_ignored"):
                stop.add(eos)
            if bug == "stop_tokens_forgotten":
                stop -= set(p.stop_token_ids)
            if fill:
                early = {v: a for v, a in late.items() if v not in stop or bug == "stop_kept_when_allowed"}
            else:
                early = {**late, **{t: NINF for t in stop if t < vocab}}
        return sorted(early.items()), sorted(late.items()), fill
    return resolve


def _mut_apply(bug):
    def apply(logits, ids, vals, meta, slots, nout, lo, vocab, out):
        B, W = logits.shape
        S = ids.shape[0]
        out.copy_(logits)
        if bug == "shard_offset_ignored":
            lo = 0
        n = max(0, min(W, vocab - lo))
        nfill = W if bug == "fill_padding" else n
        bf = logits.dtype == torch.bfloat16
        for b in range(B):
            s = int(slots[b])
            if s < 0 and bug != "minus_one_row":
                continue
            if bug == "neighbour":
                s = (s + 1) % S
            ne, nl, fill, mt = (int(v) for v in meta[s])
            early = int(nout[b]) <= mt if bug == "nout_le" else int(nout[b]) < mt
            if bug == "lists_swapped":
                early = not early
            k, cnt = (0, ne) if early else (1, nl)
            if bug == "last_entry_dropped":
                cnt = max(0, cnt - 1)
            t = ids[s, k, :cnt].long()
            a = vals[s, k, :cnt].float()
            ok = (t >= lo) & (t < lo + n)
            j, a = t[ok] - lo, a[ok]
            x = logits[b, j].float()
            if bug == "bias_in_bf16" and bf:
                a = a.bfloat16().float()
            y = x + a
            if bug == "double_rounding":
                y = torch.where(y.abs() < 60000, y.half().float() if bf else y.bfloat16().float(), y)
            y = torch.where(a == NINF, torch.full_like(y, NINF), y).to(out.dtype)
            if bug == "fill_after_edits":
                out[b, j] = y
            if fill and bug != "fill_ignored":
                out[b, :nfill] = NINF
            if bug != "fill_after_edits":
                out[b, j] = y
        return out
    return apply


def test_mutant_base_meets_every_case():
    """The mutants' common base (no bug switched on) is right, so each failure below is the bug's."""
    for name in C.CASE_NAMES:
        C.run(C.cases()[name], _mut_apply(None), _mut_resolve(None))


APPLY_BUGS = ("bias_in_bf16", "double_rounding", "fill_padding", "nout_le", "lists_swapped", "shard_offset_ignored",
              "last_entry_dropped", "fill_after_edits", "minus_one_row", "neighbour", "fill_ignored")
RESOLVE_BUGS = ("banned_allowed_kept", "bias_beats_ban", "ignore_eos_ignored", "stop_tokens_forgotten",
                "stop_kept_when_allowed")


@pytest.mark.parametrize("bug", APPLY_BUGS + RESOLVE_BUGS)
def test_wrong_definition_fails_a_case(bug):
    failed = []
    for name in C.CASE_NAMES:
        try:
            C.run(C.cases()[name], _mut_apply(bug if bug in APPLY_BUGS else None),
                  _mut_resolve(bug if bug in RESOLVE_BUGS else None))
        except (AssertionError, ValueError):  # ValueError: the wrong lists no longer fit a slot
            failed.append(name)
    print(f"{bug}: fails {len(failed)} of {len(C.CASE_NAMES)} cases")
    assert failed, f"no case notices the wrong definition {bug!r}"


# ------------------------------------------------------------------------------ resolve_token_edits
def sp(**kw):
    kw.setdefault("max_new_tokens", 8)
    return SamplingParams(**kw).validate()


def test_resolve_hand_written():
    V = 50
    assert resolve_token_edits(sp(), 2, V) == ([], [], False)
    assert not sp().has_constraints
    # biases and bans: -inf wins over a bias; early adds EOS and the stop tokens, overwriting a bias
    p = sp(logit_bias={3: 1.5, 5: -2.0, 9: 4.0}, banned_token_ids=[5, 7], min_tokens=2, stop_token_ids=[9, 11])
    assert p.has_constraints
    early, late, fill = resolve_token_edits(p, 2, V)
    assert fill is False and late == [(3, 1.5), (5, NINF), (7, NINF), (9, 4.0)]
    assert early == [(2, NINF), (3, 1.5), (5, NINF), (7, NINF), (9, NINF), (11, NINF)]
    # ignore_eos and an engine without EOS: only the stop tokens
    for q, eos in ((sp(**{**p.__dict__, "ignore_eos": True}), 2), (p, None)):
        e2, l2, _ = resolve_token_edits(q, eos, V)
        assert l2 == late and e2 == [(3, 1.5), (5, NINF), (7, NINF), (9, NINF), (11, NINF)]
    # min_tokens == 0: no early list
    assert resolve_token_edits(sp(banned_token_ids=[4], stop_token_ids=[6]), 2, V) == ([], [(4, NINF)], False)
    # min_tokens alone
    assert resolve_token_edits(sp(min_tokens=1), 2, V) == ([(2, NINF)], [], False)
    assert resolve_token_edits(sp(min_tokens=1, ignore_eos=True), 2, V) == ([], [], False)
    # an allowed set: fill, banned members dropped, biases of members kept, others' ignored; EOS both allowed and in
    # the stop set leaves the early list
    p = sp(allowed_token_ids=[11, 2, 3, 5, 9], banned_token_ids=[5, 30], logit_bias={3: 1.5, 40: 9.0}, min_tokens=2,
           stop_token_ids=[9])
    early, late, fill = resolve_token_edits(p, 2, V)
    assert fill is True and late == [(2, 0.0), (3, 1.5), (9, 0.0), (11, 0.0)] and early == [(3, 1.5), (11, 0.0)]
    e2, _, _ = resolve_token_edits(sp(**{**p.__dict__, "ignore_eos": True}), 2, V)
    assert e2 == [(2, 0.0), (3, 1.5), (11, 0.0)]
    # a stop token past the vocabulary cannot be sampled and takes no entry
    assert resolve_token_edits(sp(min_tokens=1, stop_token_ids=[70]), None, V) == ([], [], False)


def test_resolve_rejections():
    V = 1000
    for kw in (dict(logit_bias={V: 1.0}), dict(banned_token_ids=[V + 3]), dict(allowed_token_ids=[1, V])):
        with pytest.raises(ValueError):
            resolve_token_edits(sp(**kw), 2, V)
    # the empty set: everything allowed is banned; or stops before min_tokens
    with pytest.raises(ValueError):
        resolve_token_edits(sp(allowed_token_ids=[1, 2], banned_token_ids=[2, 1]), 0, V)
    with pytest.raises(ValueError):
        resolve_token_edits(sp(allowed_token_ids=[1, 2], stop_token_ids=[1], min_tokens=1), 2, V)
    resolve_token_edits(sp(allowed_token_ids=[1, 2], stop_token_ids=[1]), 2, V)  # fine without min_tokens
    resolve_token_edits(sp(allowed_token_ids=[1, 2], stop_token_ids=[1], min_tokens=1), 7, V)
    # capacity: MAX_TOKEN_EDITS entries fit, one more does not - also when only the early list overflows
    E = MAX_TOKEN_EDITS
    assert len(resolve_token_edits(sp(banned_token_ids=list(range(E))), 2, V)[1]) == E
    with pytest.raises(ValueError):
        resolve_token_edits(sp(banned_token_ids=list(range(E + 1))), 2, V)
    with pytest.raises(ValueError):
        resolve_token_edits(sp(allowed_token_ids=list(range(E + 1))), 2, V)
    full = dict(logit_bias={t: 1.0 for t in range(E)}, min_tokens=1)
    resolve_token_edits(sp(**full), 5, V)  # EOS already listed
    with pytest.raises(ValueError):
        resolve_token_edits(sp(**full), E + 5, V)


def test_validation():
    for kw in (dict(logit_bias={1: 100.0, 2: -100.0}), dict(banned_token_ids=[0]), dict(allowed_token_ids=[5, 6]),
               dict(min_tokens=8), dict(logit_bias={np.int64(3): np.float32(1.0)})):
        assert sp(**kw).has_constraints
    for kw in (dict(logit_bias={1: 100.5}), dict(logit_bias={1: float("nan")}), dict(logit_bias={1: NINF}),
               dict(logit_bias={-1: 1.0}), dict(logit_bias={"1": 1.0}), dict(logit_bias={1: "x"}), dict(logit_bias=[1]),
               dict(logit_bias={True: 1.0}), dict(banned_token_ids=[1, 1]), dict(banned_token_ids=[-2]),
               dict(banned_token_ids=[1.5]), dict(allowed_token_ids=[3, 4, 3]), dict(allowed_token_ids="12"),
               dict(min_tokens=-1), dict(min_tokens=9), dict(min_tokens=1.0), dict(min_tokens=None)):
        with pytest.raises(ValueError):
            SamplingParams(max_new_tokens=8, **kw).validate()


def test_fields_survive_the_control_plane():
    """The TP control plane pickles params.__dict__ (serving/driver.py): int keys and float values come back."""
    p = sp(logit_bias={50256: -100.0, 7: 0.25}, banned_token_ids=[1, 2], allowed_token_ids=[7, 9, 50256], min_tokens=3)
    q = SamplingParams(**pickle.loads(pickle.dumps(p.__dict__.copy(), protocol=pickle.HIGHEST_PROTOCOL)))
    assert q == p and q.validate().has_constraints and all(isinstance(k, int) for k in q.logit_bias)
    assert resolve_token_edits(q, 0, 60000) == resolve_token_edits(p, 0, 60000)
