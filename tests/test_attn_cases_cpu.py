"""The closed-form attention cases of tests/attn_cases.py, checked without a GPU: the fp32 oracles
(R.attn_decode / attn_extend / attn_prefill) meet the closed form under the tolerances the GPU tests use, and the
same oracles with one key too many, one too few, a causal mask off by one, pages of another sequence or the wrong
kv head FAIL the check on every affected (row, head). That is the proof that tests/test_attn_exact_gpu.py can fail."""
import pytest
import torch

import attn_cases as AC
from llmss_amd.ops import reference as R

DECODE_CTX = [1, 15, 16, 17, 63, 64, 65, 255, 256, 257, 300]
EXTEND = [(0, 1), (0, 63), (0, 64), (0, 65), (63, 1), (64, 1), (65, 1), (15, 17), (40, 22), (100, 130), (200, 1),
          (255, 2)]
PREFILL_LENS = [1, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 200]
NH, NKV = 6, 2


def paged_cases(geo, D, kv8, extend):
    yield AC.census(geo, NH, NKV, D, 0, kv8=kv8)
    yield AC.census(geo, NH, NKV, D, 1, kv8=kv8)
    if extend:
        strong, weak = AC.chunk_needles(geo, NKV, (16, 21, 32, 64))
        yield AC.needle(geo, NH, NKV, D, strong, weak, kv8=kv8)
    else:
        yield AC.needle(geo, NH, NKV, D, AC.decode_needles(geo, NKV, (64, 256)), kv8=kv8)


def run_paged(case, extend, ctx_delta=0, table=None, roll=0):
    geo = case.geo
    kc, vc = case.k_cache.roll(roll, 1), case.v_cache.roll(roll, 1)
    table = geo.table if table is None else table
    ctx = geo.ctx_lens + ctx_delta
    if extend:
        return R.attn_extend(case.q, kc, vc, table, geo.cu_q, ctx, case.nh, case.nkv, case.D, case.scale)
    return R.attn_decode(case.q, kc, vc, table, ctx, case.nh, case.nkv, case.D, case.scale)


def per_head(case, rows_kv):
    """[T, nkv] -> [T, nh]"""
    return rows_kv.repeat_interleave(case.nh // case.nkv, 1)


def all_rows(case):
    return torch.ones(case.geo.T, case.nh, dtype=torch.bool)


def roll_affected(case):
    """Rows that the next kv head's data changes. A census row whose histogram is uniform (pass 0 at a context of
    64 k keys) looks the same from every kv head: the other pass and the needle tell those apart."""
    if case.kind == "needle":
        return all_rows(case)
    other = case.expected.view(case.geo.T, case.nkv, -1).roll(1, 1).reshape(case.geo.T, -1)
    return AC.bad_rows(case, other.to(torch.bfloat16))


def caught(case, out, affected, what):
    """The perturbed output fails on every affected (row, head)."""
    assert bool(affected.any()), f"{what}: the perturbation affects nothing"
    missed = affected & ~AC.bad_rows(case, out)
    assert not bool(missed.any()), (f"{what} {case.kind}: {int(missed.sum())} of {int(affected.sum())} affected "
                                    f"(row, head) pairs pass, first {missed.nonzero()[0].tolist()}")


def swapped_table(geo, a, b):
    """The first two pages of sequences a and b exchanged."""
    t = geo.table.clone()
    t[a, :2], t[b, :2] = geo.table[b, :2], geo.table[a, :2]
    return t


def swap_affected(case, a, b):
    geo = case.geo
    rows = (geo.row_seq == a) | (geo.row_seq == b)
    if case.kind == "census":
        return all_rows(case) & rows[:, None]
    hit = case.extra["strong"] < 2 * geo.bs  # the needle lies in an exchanged page
    return per_head(case, hit[geo.row_seq] & rows[:, None])


def one_key(case):
    """Does this case see a single key more or less? The second census pass (digit = t // 64) does not: a column
    that counts all n keys reads n / n whatever n is. It is there for keys replaced by ones 64 k positions away."""
    return case.kind == "needle" or case.extra["digit_pass"] == 0


def dup_table(geo):
    """Table entries 4..7 replaced by entries 0..3: keys 64..127 are read from 64 positions earlier, the error of a
    partition that walks another partition's pages. Invisible to digit = t % 64; the second census pass sees it."""
    t = geo.table.clone()
    t[:, 4:8] = geo.table[:, 0:4]
    return t


def dup_affected(case):
    geo = case.geo
    long = torch.tensor(geo.ctx)[geo.row_seq] >= 128
    return all_rows(case) & (long & (geo.row_pos >= 64))[:, None]


def last_rows(geo):
    return geo.row_pos == torch.tensor(geo.ctx)[geo.row_seq] - 1


@pytest.mark.parametrize("kv8", [False, True], ids=["bf16", "fp8"])
@pytest.mark.parametrize("D", [64, 128])
def test_decode_cases(D, kv8):
    geo = AC.geometry(DECODE_CTX, bs=16, seed=D)
    for case in paged_cases(geo, D, kv8, extend=False):
        AC.assert_exact(case, run_paged(case, False), "R.attn_decode")
        AC.assert_exact(case, AC.oracle(case).to(torch.bfloat16), "oracle")
        if case.kind == "census":
            # the oracle gives the correctly rounded quotient, so the GPU tolerance has 2^-8 left for the kernel
            assert torch.equal(run_paged(case, False), case.expected.to(torch.bfloat16))
            minus = plus = all_rows(case)
        else:
            minus = per_head(case, case.extra["strong"] == torch.tensor(geo.ctx)[:, None] - 1)
            plus = all_rows(case)  # the forbidden needle at position ctx
        if one_key(case):
            caught(case, run_paged(case, False, ctx_delta=-1), minus, "ctx - 1")
            caught(case, run_paged(case, False, ctx_delta=1), plus, "ctx + 1")
        else:
            caught(case, run_paged(case, False, table=dup_table(geo)), dup_affected(case), "pages 64 keys away")
        caught(case, run_paged(case, False, roll=1), roll_affected(case), "kv head + 1")
        a, b = 7, 9
        caught(case, run_paged(case, False, table=swapped_table(geo, a, b)), swap_affected(case, a, b), "pages")


@pytest.mark.parametrize("kv8", [False, True], ids=["bf16", "fp8"])
def test_extend_cases(kv8):
    D = 64
    geo = AC.geometry([p + c for p, c in EXTEND], [c for _, c in EXTEND], bs=16, seed=3)
    last = last_rows(geo)
    for case in paged_cases(geo, D, kv8, extend=True):
        AC.assert_exact(case, run_paged(case, True), "R.attn_extend")
        AC.assert_exact(case, AC.oracle(case).to(torch.bfloat16), "oracle")
        if case.kind == "census":
            lost = seen = all_rows(case)           # every row loses its own key / gains the next one
            seen_mask = all_rows(case) & ~last[:, None]  # the last row has no next key inside the context
        else:
            st = case.extra["strong"][geo.row_seq]  # [T, nkv]
            lost = per_head(case, geo.row_pos[:, None] == st)
            seen_mask = per_head(case, geo.row_pos[:, None] == st - 1)
            seen = seen_mask | last[:, None]        # the last row reaches the forbidden needle at position ctx
        if one_key(case):
            caught(case, run_paged(case, True, ctx_delta=-1), lost, "ctx - 1")
            caught(case, run_paged(case, True, ctx_delta=1), seen, "ctx + 1")
            caught(case, AC.oracle(case, mask_shift=-1).to(torch.bfloat16), lost, "mask >=")
            caught(case, AC.oracle(case, mask_shift=1).to(torch.bfloat16), seen_mask, "mask > qpos + 1")
        else:
            caught(case, run_paged(case, True, table=dup_table(geo)), dup_affected(case), "pages 64 keys away")
        caught(case, run_paged(case, True, roll=1), roll_affected(case), "kv head + 1")
        a, b = 3, 9
        caught(case, run_paged(case, True, table=swapped_table(geo, a, b)), swap_affected(case, a, b), "pages")


def run_prefill(case, roll=0):
    nh, nkv, D = case.nh, case.nkv, case.D
    x = case.qkv.clone()
    T = x.shape[0]
    for off in (nh * D, (nh + nkv) * D):
        x[:, off: off + nkv * D] = case.qkv[:, off: off + nkv * D].reshape(T, nkv, D).roll(roll, 1).reshape(T, -1)
    return R.attn_prefill(x, case.geo.cu_q, nh, nkv, D, case.scale)


@pytest.mark.parametrize("D", [64, 128])
def test_prefill_cases(D):
    geo = AC.packed_geometry(PREFILL_LENS)
    last = last_rows(geo)
    strong, weak = AC.chunk_needles(geo, NKV, (16, 32, 64, 128))
    for case in (AC.census(geo, NH, NKV, D, 0), AC.census(geo, NH, NKV, D, 1),
                 AC.needle(geo, NH, NKV, D, strong, weak)):
        assert case.qkv.stride(0) == case.qkv.shape[1] + AC.PAD
        AC.assert_exact(case, run_prefill(case), "R.attn_prefill")
        AC.assert_exact(case, AC.oracle(case).to(torch.bfloat16), "oracle")
        if case.kind == "census":
            lost, seen = all_rows(case), all_rows(case) & ~last[:, None]
        else:
            st = case.extra["strong"][geo.row_seq]
            lost = per_head(case, geo.row_pos[:, None] == st)
            seen = per_head(case, geo.row_pos[:, None] == st - 1)
        if one_key(case):
            caught(case, AC.oracle(case, mask_shift=-1).to(torch.bfloat16), lost, "mask >=")
            caught(case, AC.oracle(case, mask_shift=1).to(torch.bfloat16), seen, "mask > qpos + 1")
        caught(case, run_prefill(case, roll=1), roll_affected(case), "kv head + 1")


def test_poison_is_everywhere_else():
    """Every cache row outside the sequences' keys is poison (or a forbidden needle with poison V), the spare page
    and the tail of the last page included; the block table's unused entries point at an unowned page."""
    geo = AC.geometry(DECODE_CTX, bs=16, seed=1)
    case = AC.census(geo, NH, NKV, 64)
    free = torch.ones(geo.nb * geo.bs, dtype=torch.bool)
    free[geo.slot] = False
    for cache in (case.k_cache, case.v_cache):
        rows = cache.permute(0, 2, 1, 3).reshape(geo.nb * geo.bs, NKV, 64)
        assert bool((rows[free].float() == AC.POISON).all())
        assert not bool((rows[~free].float() == AC.POISON).any())
    assert int(free.sum()) >= geo.B * geo.bs + 3 * geo.bs
    assert set(geo.table[geo.B:].flatten().tolist()) == {int(geo.unowned[0])}
    ndl = AC.needle(geo, NH, NKV, 64, AC.decode_needles(geo, NKV, (64,)))
    vrows = ndl.v_cache.permute(0, 2, 1, 3).reshape(geo.nb * geo.bs, NKV, 64)
    assert bool((vrows[free].float() == AC.POISON).all())
    assert bool((ndl.q.storage_offset() == 0) and ndl.q.stride(0) == NH * 64 + AC.PAD)


def test_census_refuses_crowded_histograms():
    with pytest.raises(AssertionError, match="census entry counts"):
        AC.census(AC.geometry([64 * 81]), 2, 1, 64, 0)
