"""The windowed closed forms of tests/attn_window_cases.py, checked without a GPU, in the manner of
tests/test_attn_cases_cpu.py: the fp32 references (R.attn_decode / R.attn_extend with window / kv_starts) and the
helper's own oracle meet the closed form, and the oracle with one key too many or too few at the lower edge, or with
the window taken from the sequence's last row instead of the row's own position, FAILS on every affected (row, head).
That is the proof that tests/test_attn_window_gpu.py can fail."""
import pytest
import torch

import attn_cases as AC
import attn_window_cases as WC
from llmss_amd.ops import reference as R

NH, NKV, BS = 6, 2, 16
DECODE = [(1, [1, 5, 40]), (15, [1, 14, 15, 16, 31, 300]), (16, [15, 16, 17, 32, 33, 300]),
          (17, [16, 17, 18, 33, 35, 300]), (256, [255, 256, 257, 272, 513])]  # (W, contexts)
EXTEND = [(0, 17, 8), (100, 130, 16), (200, 1, 63), (200, 1, 64), (200, 1, 65), (63, 1, 64), (64, 1, 64), (65, 1, 64),
          (40, 22, 21), (40, 22, 22), (40, 22, 23), (255, 2, 1)]  # (prefix, chunk, W)


def run_ref(case, extend):
    geo, ks = case.geo, case.extra["kv_starts"]
    ks = None if ks is None else ks.to(torch.int32)
    if extend:
        return R.attn_extend(case.q, case.k_cache, case.v_cache, geo.table, geo.cu_q, geo.ctx_lens, case.nh, case.nkv,
                             case.D, case.scale, window=case.extra["window"], kv_starts=ks)
    return R.attn_decode(case.q, case.k_cache, case.v_cache, geo.table, geo.ctx_lens, case.nh, case.nkv, case.D,
                         case.scale, window=case.extra["window"], kv_starts=ks)


def per_head(case, rows_kv):
    return rows_kv.repeat_interleave(case.nh // case.nkv, 1)


def caught(case, out, affected, what):
    assert bool(affected.any()), f"{what}: the perturbation affects nothing"
    missed = affected & ~AC.bad_rows(case, out)
    assert not bool(missed.any()), (f"{what} {case.kind}: {int(missed.sum())} of {int(affected.sum())} affected "
                                    f"(row, head) pairs pass, first {missed.nonzero()[0].tolist()}")


def affected_rows(case, lo_wrong):
    """(row, head) pairs whose key set [lo_wrong, p] is another one than the right one: every such row of the census
    (digit = t % 64 sees any single key), and the needle rows whose strongest needle changes."""
    geo = case.geo
    lo = WC.row_lo(geo, case.extra["window"], case.extra["kv_starts"])
    if case.kind == "census":
        return (lo_wrong != lo)[:, None].expand(geo.T, case.nh)
    right, _ = WC.selection(case, lo, geo.row_pos)
    wrong, _ = WC.selection(case, lo_wrong, geo.row_pos)
    return per_head(case, right != wrong)


def check_mutants(case):
    geo = case.geo
    W, ks = case.extra["window"], case.extra["kv_starts"]
    lo = WC.row_lo(geo, W, ks)
    AC.assert_exact(case, WC.oracle(case).to(torch.bfloat16), "windowed oracle")
    can_grow = lo > 0
    caught(case, WC.oracle(case, lo_shift=-1).to(torch.bfloat16), affected_rows(case, lo - 1) & can_grow[:, None],
           "one key too many at the lower edge")
    caught(case, WC.oracle(case, lo_shift=1).to(torch.bfloat16), affected_rows(case, lo + 1),
           "one key too few at the lower edge")
    if max(geo.qlen) > 1 and W > 0:
        last = torch.tensor(geo.ctx)[geo.row_seq] - 1
        caught(case, WC.oracle(case, last_row_window=True).to(torch.bfloat16),
               affected_rows(case, WC.row_lo(geo, W, ks, last)), "the last row's window for every row")


@pytest.mark.parametrize("kv8", [False, True], ids=["bf16", "fp8"])
@pytest.mark.parametrize("W,ctx", DECODE)
def test_window_decode_cases(W, ctx, kv8):
    D = 64
    geo = AC.geometry(ctx, bs=BS, seed=W)
    for case in (WC.census(geo, NH, NKV, D, W, kv8=kv8), WC.needle(geo, NH, NKV, D, W, kv8=kv8)):
        AC.assert_exact(case, run_ref(case, False), "R.attn_decode")
        check_mutants(case)


@pytest.mark.parametrize("kv8", [False, True], ids=["bf16", "fp8"])
def test_kv_starts_decode_cases(kv8):
    """kv_starts alone, and with a window where each of the two binds in turn."""
    D, ctx = 64, [40, 40, 40, 40, 40, 40]
    geo = AC.geometry(ctx, bs=BS, seed=5)
    starts = [0, 1, BS - 1, BS, BS + 1, 39]
    for W in (0, 30, 8):  # none; binds for the low starts only; binds for all but the last
        for case in (WC.census(geo, NH, NKV, D, W, starts, kv8=kv8), WC.needle(geo, NH, NKV, D, W, starts, kv8=kv8)):
            AC.assert_exact(case, run_ref(case, False), f"R.attn_decode W {W}")
            check_mutants(case)


@pytest.mark.parametrize("kv8", [False, True], ids=["bf16", "fp8"])
def test_window_extend_cases(kv8):
    D = 64
    for W in sorted({w for _, _, w in EXTEND}):
        chunks = [(p, c) for p, c, w in EXTEND if w == W]
        geo = AC.geometry([p + c for p, c in chunks], [c for _, c in chunks], bs=BS, seed=W)
        cases = [WC.census(geo, NH, NKV, D, W, kv8=kv8), WC.needle(geo, NH, NKV, D, W, kv8=kv8)]
        # the strong needle at the lo of the first row and of a middle row as well
        mid = torch.tensor([[q // 2] * NKV for q in geo.qlen])
        cases += [WC.needle(geo, NH, NKV, D, W, target=torch.zeros_like(mid), kv8=kv8, seed=1),
                  WC.needle(geo, NH, NKV, D, W, target=mid, kv8=kv8, seed=2)]
        for case in cases:
            AC.assert_exact(case, run_ref(case, True), f"R.attn_extend W {W}")
            check_mutants(case)


def test_kv_starts_extend_cases():
    D = 64
    geo = AC.geometry([40 + 22, 100 + 30, 17], [22, 30, 17], bs=BS, seed=9)
    for W, starts in ((0, [17, 33, 0]), (21, [30, 99, 0]), (64, [1, 16, 0])):
        for case in (WC.census(geo, NH, NKV, D, W, starts), WC.needle(geo, NH, NKV, D, W, starts)):
            AC.assert_exact(case, run_ref(case, True), f"R.attn_extend W {W} starts {starts}")
            check_mutants(case)


def test_released_pages_are_poison_and_redirected():
    geo = AC.geometry([100, 33, 5], bs=BS, seed=2)
    W = 20
    for case in (WC.census(geo, NH, NKV, 64, W), WC.needle(geo, NH, NKV, 64, W)):
        for b, lo in enumerate(WC.seq_lo(geo, W).tolist()):
            n = lo // BS
            assert n == max(0, geo.ctx[b] - W) // BS
            assert bool((case.geo.table[b, :n] == int(geo.unowned[0])).all())
            assert bool((case.geo.table[b, n:] == geo.table[b, n:]).all())
            for pg in geo.table[b, :n].tolist():
                for cache in (case.k_cache, case.v_cache):
                    assert bool((cache[pg].float() == AC.POISON).all())
    assert int(WC.seq_lo(geo, W)[0]) // BS == 5  # the case has released pages at all
