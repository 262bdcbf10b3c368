"""Exact key-set tests of the decode and extend attention kernels with a sliding window and / or a first readable key
(window / kv_starts): the windowed closed forms of tests/attn_window_cases.py (tests/test_attn_window_cases_cpu.py
shows they catch one key too many or too few at the lower edge), at every window and context on an edge of a page, a
wave-load, a partition or a tile, for every head-group branch and both cache types. Pages wholly below a window are
poison and their table entries point at an unowned poison page: nothing below the window's first page may be read.
Every output is a view into a NaN-filled buffer, as in tests/test_attn_exact_gpu.py."""
import pytest
import torch

import attn_cases as AC
import attn_window_cases as WC
from llmss_amd.ops import hip as H

pytestmark = pytest.mark.gpu
dev = "cuda"

CACHES = [pytest.param(False, id="bf16"), pytest.param(True, id="fp8")]
DECODE_HEADS = [(4, 4, 16), (4, 2, 16), (8, 2, 16), (16, 1, 16), (16, 2, 16), (8, 2, 32)]  # G = 1 2 4 16 8 (every GB)
EXTEND_HEADS = [(4, 4), (6, 2), (8, 1), (48, 1)]
EXTEND = [(0, 17, 8), (100, 130, 16), (200, 1, 63), (200, 1, 64), (200, 1, 65), (63, 1, 64), (64, 1, 64), (65, 1, 64),
          (40, 22, 21), (40, 22, 22), (40, 22, 23), (255, 2, 1)]  # (prefix, chunk, W)


class NanOut:
    """out= as a view into a NaN-filled buffer that is taller and wider than the result."""

    def __init__(self, T, W):
        self.T, self.W = T, W
        self.buf = torch.full((T + 3, W + 72), float("nan"), dtype=torch.bfloat16, device=dev)
        self.out = self.buf[2: 2 + T, 8: 8 + W]

    def check(self, what):
        outside = torch.ones_like(self.buf, dtype=torch.bool)
        outside[2: 2 + self.T, 8: 8 + self.W] = False
        assert bool(self.buf[outside].isnan().all()), f"{what}: wrote outside its [{self.T}, {self.W}] output"


# ---------------------------------------------------------------------------------------------- decode
def decode_launch(case, splits, what, max_ctx=None):
    geo = case.geo
    W = case.extra["window"]
    ctx_lens = torch.cat([geo.ctx_lens, torch.tensor([1 << 20, 7], dtype=torch.int32)]).to(dev)
    ks = WC.kv_starts_dev(case, dev)
    if ks is not None:
        ks = torch.cat([ks, torch.zeros(2, dtype=torch.int32, device=dev)])
    o = NanOut(geo.B, case.nh * case.D)
    H.attn_decode(case.q, case.k_cache, case.v_cache, geo.table.to(dev), ctx_lens, case.nh, case.nkv, case.D,
                  case.scale, max_ctx or max(geo.ctx), out=o.out, splits=splits, window=W, kv_starts=ks)
    tag = f"{what} W {W} splits {splits}"
    AC.assert_exact(case, o.out, tag)
    o.check(tag)


def window_contexts(W, bs, STEP, parts):
    cs = {1, W - 1, W, W + 1, W + bs, 2 * W + 1}
    for P in parts:
        cs |= {P, P + 1, P + STEP + 1}
    return sorted(c for c in cs if c >= 1)


@pytest.mark.parametrize("kv8", CACHES)
@pytest.mark.parametrize("nh,nkv,bs", [pytest.param(*h, id="-".join(map(str, h))) for h in DECODE_HEADS])
@pytest.mark.parametrize("D", [64, 128, 256])
def test_decode_window_exact(D, nh, nkv, bs, kv8):
    STEP = 4 * 64 // (D // 8)
    for W in sorted({1, bs - 1, bs, bs + 1, STEP, 256, 257}):
        span = H.decode_span(1 << 20, bs, W)
        dflt = H.decode_splits(16, nkv, span, bs)
        ctx = window_contexts(W, bs, STEP, {256, 272, dflt[1]})
        geo = AC.geometry(ctx, bs=bs, seed=D + nh + W)
        cover = geo.table.shape[1] * bs
        dflt = H.decode_splits(len(ctx), nkv, H.decode_span(max(ctx), bs, W), bs)
        cases = [WC.census(geo, nh, nkv, D, W, digit_pass=p, kv8=kv8, device=dev) for p in (0, 1)]
        cases.append(WC.needle(geo, nh, nkv, D, W, kv8=kv8, device=dev))
        # the strong needle on the last key and on / next to the partition edges inside the window
        lo = WC.seq_lo(geo, W)
        strong = torch.zeros(geo.B, nkv, dtype=torch.int64)
        for b, n in enumerate(geo.ctx):
            cands = [n - 1, int(lo[b]) + 1] + [int(lo[b]) // bs * bs + e for e in (255, 256, 271, 272, dflt[1])]
            for k in range(nkv):
                strong[b, k] = AC.pick([c for c in cands if c >= int(lo[b])] + [int(lo[b])], n, b + k)
        cases.append(WC.needle(geo, nh, nkv, D, W, strong=strong, kv8=kv8, device=dev, seed=1))
        for i, case in enumerate(cases):
            for splits in ((1, cover), None, dflt, (3, 256), (3, 272)):
                decode_launch(case, splits, f"case {i}")


@pytest.mark.parametrize("kv8", CACHES)
@pytest.mark.parametrize("nh,nkv", [(4, 2), (16, 2)])
def test_decode_kv_starts_exact(nh, nkv, kv8):
    """kv_starts alone, then together with a window that binds for some rows (W = 290: starts 0 and 1) or for all
    but the last (W = 8)."""
    D, bs, n = 128, 16, 300
    starts = [0, 1, bs - 1, bs, bs + 1, n - 1]
    geo = AC.geometry([n] * len(starts), bs=bs, seed=7)
    cover = geo.table.shape[1] * bs
    for W in (0, 290, 8):
        cases = [WC.census(geo, nh, nkv, D, W, starts, digit_pass=p, kv8=kv8, device=dev) for p in (0, 1)]
        cases.append(WC.needle(geo, nh, nkv, D, W, starts, kv8=kv8, device=dev))
        for i, case in enumerate(cases):
            for splits in ((1, cover), None, (3, 256), (3, 272)):
                decode_launch(case, splits, f"starts case {i}")


@pytest.mark.parametrize("kv8", CACHES)
def test_decode_long_window(kv8):
    """A window of more than 4096 keys in one partition: more pages than the LDS staging holds, so the page ids come
    straight from the block table - none of them from below the window."""
    D, nh, nkv, n, W = 128, 8, 1, 8300, 4100
    geo = AC.geometry([n], bs=16, seed=11)
    cases = [WC.census(geo, nh, nkv, D, W, base=128, kv8=kv8, device=dev), WC.needle(geo, nh, nkv, D, W, kv8=kv8,
                                                                                      device=dev)]
    for i, case in enumerate(cases):
        decode_launch(case, (1, 4128), f"long case {i}")


@pytest.mark.parametrize("kv8", CACHES)
def test_unwindowed_call_is_unchanged(kv8):
    """window = 0 with kv_starts = None is the call without the arguments, bit for bit (the same kernel)."""
    geo = AC.geometry([1000, 37, 300], bs=16, seed=3)
    case = AC.random_case(geo, 8, 2, 128, kv8=kv8, device=dev, seed=1)
    args = (case.q, case.k_cache, case.v_cache, geo.table.to(dev), geo.ctx_lens.to(dev), 8, 2, 128, case.scale, 1000)
    for splits in (None, (1, 1008), (3, 512)):
        assert torch.equal(H.attn_decode(*args, splits=splits), H.attn_decode(*args, splits=splits, window=0,
                                                                              kv_starts=None))
    geo = AC.geometry([1064, 300], [64, 8], bs=16, seed=4)
    case = AC.random_case(geo, 8, 2, 128, kv8=kv8, device=dev, seed=2)
    args = (case.q, case.k_cache, case.v_cache, geo.table.to(dev), geo.cu_q.to(dev), geo.ctx_lens.to(dev), 64, 8, 2,
            128, case.scale)
    assert torch.equal(H.attn_extend(*args), H.attn_extend(*args, window=0, kv_starts=None))


def test_window_arguments_are_validated():
    geo = AC.geometry([40, 50], bs=16)
    case = AC.census(geo, 4, 2, 64, device=dev)
    args = (case.q, case.k_cache, case.v_cache, geo.table.to(dev), geo.ctx_lens.to(dev), 4, 2, 64, case.scale, 50)
    good = torch.zeros(2, dtype=torch.int32, device=dev)
    for bad in (good.long(), good.cpu(), good[:1], torch.zeros(4, dtype=torch.int32, device=dev)[::2]):
        with pytest.raises(ValueError, match="kv_starts"):
            H.attn_decode(*args, kv_starts=bad)
    with pytest.raises(ValueError, match="window"):
        H.attn_decode(*args, window=-1)
    with pytest.raises(ValueError, match="cover"):
        H.attn_decode(*args, window=8, splits=(1, 16))  # the span is window + one page


# ---------------------------------------------------------------------------------------------- extend
def extend_launch(case, max_qlen, what, twin=False):
    geo, nh, nkv, D = case.geo, case.nh, case.nkv, case.D
    args = (case.q, case.k_cache, case.v_cache, geo.table.to(dev), geo.cu_q.to(dev), geo.ctx_lens.to(dev), max_qlen,
            nh, nkv, D, case.scale)
    kw = dict(window=case.extra["window"], kv_starts=WC.kv_starts_dev(case, dev))
    o = NanOut(geo.T, nh * D)
    H.attn_extend(*args, out=o.out, **kw)
    AC.assert_exact(case, o.out, what)
    o.check(what)
    if twin:  # the fp8 twin is an extra output: the bf16 one stays bit-identical
        dense = torch.full((geo.T, nh * D), float("nan"), dtype=torch.bfloat16, device=dev)
        H.attn_extend(*args, out=dense, fp8_out=True, **kw)
        assert torch.equal(dense, o.out), f"{what}: fp8_out changes the bf16 output"


def extend_cases(geo, nh, nkv, D, W, kv8, starts=None, base=64, passes=(0, 1)):
    cases = [WC.census(geo, nh, nkv, D, W, starts, digit_pass=p, base=base, kv8=kv8, device=dev) for p in passes]
    mid = torch.tensor([[q // 2] * nkv for q in geo.qlen])
    for rot, target in enumerate((None, torch.zeros_like(mid), mid)):  # the strong needle at the lo of these rows
        cases.append(WC.needle(geo, nh, nkv, D, W, starts, target=target, kv8=kv8, device=dev, seed=rot))
    return cases


@pytest.mark.parametrize("kv8", CACHES)
@pytest.mark.parametrize("nh,nkv", EXTEND_HEADS)
@pytest.mark.parametrize("D", [64, 128, 256])
def test_extend_window_exact(D, nh, nkv, kv8):
    twin = H.extend_fp8_twin_ok(nh, nkv)
    for W in sorted({w for _, _, w in EXTEND}):
        chunks = [(p, c) for p, c, w in EXTEND if w == W]
        geo = AC.geometry([p + c for p, c in chunks], [c for _, c in chunks], bs=16, seed=D + nh + W)
        for i, case in enumerate(extend_cases(geo, nh, nkv, D, W, kv8)):
            extend_launch(case, max(geo.qlen), f"W {W} case {i}", twin)
    # a first readable key inside the first page, alone and under a window
    geo = AC.geometry([40 + 22, 100 + 30, 17], [22, 30, 17], bs=16, seed=D + nh)
    for W, starts in ((0, [17, 33, 0]), (21, [30, 99, 0]), (64, [1, 16, 0])):
        for i, case in enumerate(extend_cases(geo, nh, nkv, D, W, kv8, starts)):
            extend_launch(case, 30, f"W {W} starts {starts} case {i}", twin)


@pytest.mark.parametrize("kv8", CACHES)
def test_extend_long_context_window(kv8):
    """More than 512 pages per sequence, the window in the last ones: the staged page ids start at the window's first
    page (5 pages here), not at page 0."""
    D, nh, nkv, W = 128, 8, 1, 64
    geo = AC.geometry([8208, 8208], [8, 1], bs=16, seed=12)
    assert (8208 + 15) // 16 > 512
    for i, case in enumerate(extend_cases(geo, nh, nkv, D, W, kv8, base=128, passes=(0,))):
        extend_launch(case, 8, f"long case {i}", True)


# ------------------------------------------------------------ random data, error relative to the signal
def signal_bound(case, out, what):
    """The rule of tests/test_attn_exact_gpu.py signal_bound: the kernel's largest (row, head) error relative to the
    RMS of the fp32 windowed oracle is at most 4 x that of the same oracle with P and the output rounded to bf16. The
    emulation is the yardstick; the kernel is never used for it."""
    ref = WC.oracle(case)
    emu = AC.signal_error(WC.oracle(case, emulate=True), ref, case.nh, case.D)
    got = AC.signal_error(out, ref, case.nh, case.D)
    print(f"{what}: kernel {got:.4g}, bf16 emulation {emu:.4g}, bound {4 * emu:.4g}")
    assert got <= 4 * emu, f"{what}: error / signal {got:.4g} > 4 x {emu:.4g}"


@pytest.mark.parametrize("kv8", CACHES)
def test_window_signal_relative(kv8):
    """Random q / K / V, W = 512, D = 128, 8 / 2 heads: decode at ctx 1500, an 8-row chunk ending at 1500 and a 64-row
    chunk ending at 1064."""
    W = 512
    geo = AC.geometry([1500], bs=16, seed=1)
    case = WC.random_case(geo, 8, 2, 128, W, kv8=kv8, device=dev, seed=5)
    for splits in (None, (1, 1504), (3, 256)):
        out = H.attn_decode(case.q, case.k_cache, case.v_cache, case.geo.table.to(dev), geo.ctx_lens.to(dev), 8, 2, 128,
                            case.scale, 1500, splits=splits, window=W)
        signal_bound(case, out, f"decode splits {splits}")
    geo = AC.geometry([1500, 1064], [8, 64], bs=16, seed=2)
    case = WC.random_case(geo, 8, 2, 128, W, kv8=kv8, device=dev, seed=6)
    out = H.attn_extend(case.q, case.k_cache, case.v_cache, case.geo.table.to(dev), geo.cu_q.to(dev),
                        geo.ctx_lens.to(dev), 64, 8, 2, 128, case.scale, window=W)
    signal_bound(case, out, "extend")
