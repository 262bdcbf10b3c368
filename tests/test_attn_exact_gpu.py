"""Exact key-set tests of the decode, extend and prefill attention kernels: structured inputs whose correct output
is known in closed form (tests/attn_cases.py; tests/test_attn_cases_cpu.py shows the checks catch a single wrong
key), at every context, chunk and length on an edge of a partition, tile, page, unroll chunk or workgroup, for every
head-group dispatch branch, cache type and tuning variant. Every output is a view into a NaN-filled buffer: the
kernel must write all of its rows and nothing else."""
import pytest
import torch

import attn_cases as AC
from llmss_amd.ops import hip as H

pytestmark = pytest.mark.gpu
dev = "cuda"

CACHES = [pytest.param(False, id="bf16"), pytest.param(True, id="fp8")]
DECODE_HEADS = [(4, 4), (4, 2), (6, 2), (8, 2), (12, 2), (16, 2), (24, 2), (16, 1)]  # G = 1 2 3 4 6 8 12 16
EXTEND_HEADS = [(4, 4), (4, 2), (6, 2), (10, 2), (12, 2), (8, 1), (12, 1), (16, 1), (48, 1), (96, 1)]
PREFILL_HEADS = [(4, 4), (4, 2), (6, 2), (8, 2), (16, 2), (8, 1)]  # GH = 1 2 (1|2) 4 8 8
BS32_HEADS = (6, 2)  # the one head shape per D that also runs with 32-token pages
EXTEND_CHUNKS = [(0, 1), (0, 63), (0, 64), (0, 65), (63, 1), (64, 1), (65, 1), (15, 17), (40, 22), (100, 130),
                 (200, 1), (255, 2)]  # (prefix, chunk); 22 rows cross a workgroup at rows_per_wg = 21
EXTEND_DECODE_CTX = [1, 15, 16, 17, 63, 64, 65, 127, 128, 129, 200, 257]
PREFILL_LENS = [1, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 200]
PREFILL_BATCH8 = [1, 64, 65, 129, 16, 33, 200, 128]  # 8 sequences: npair % 8 == 0, the XCD-grouped order
PREFILL_VARIANTS = [(1, 0), (2, 0), (3, 4), (3, 8)]  # (version, waves)


def with_bs32(heads):
    return [pytest.param(nh, nkv, 16, id=f"{nh}-{nkv}") for nh, nkv in heads] + [
        pytest.param(*BS32_HEADS, 32, id=f"{BS32_HEADS[0]}-{BS32_HEADS[1]}-bs32")]


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
def decode_plan(D, nkv, bs):
    """(contexts, default splits): every context on or next to an edge of a wave-load (STEP tokens), of two unroll
    chunks (CH = STEP * tokens in flight, 1 / 2 / 4), of a partition P and of the whole split range, for every
    split the test launches."""
    STEP = 4 * 64 // (D // 8)
    cs = {1, STEP - 1, STEP, STEP + 1}
    for tokens in (1, 2, 4):
        CH = STEP * tokens
        cs |= {2 * CH - 1, 2 * CH, 2 * CH + 1}
    parts = [(3, 256), (3, 272)]
    for _ in range(3):  # the default split depends on the batch and its longest context: iterate to the fixed point
        all_cs = set(cs)
        for n, P in parts:
            all_cs |= {P - 1, P, P + 1, P + STEP + 1, n * P}
        dflt = H.decode_splits(len(all_cs), nkv, max(all_cs), bs)
        if dflt in parts:
            break
        parts = parts[:2] + [dflt]
    ctx = sorted(all_cs)
    assert H.decode_splits(len(ctx), nkv, ctx[-1], bs) == dflt and dflt[0] > 1
    return ctx, dflt


def decode_launches(case, geo, splits_list, what):
    """One launch per split over the sequences that split covers (contexts ascend), with a block table and a
    ctx_lens longer than the batch."""
    ctx_lens = torch.cat([geo.ctx_lens, torch.tensor([1 << 20, 7], dtype=torch.int32)]).to(dev)
    table = geo.table.to(dev)
    assert case.q.stride(0) == case.q.shape[1] + AC.PAD  # the poisoned pad columns
    for nsplit, P in splits_list:
        B = sum(c <= nsplit * P for c in geo.ctx)
        o = NanOut(B, case.nh * case.D)
        H.attn_decode(case.q[:B], case.k_cache, case.v_cache, table, ctx_lens, case.nh, case.nkv, case.D,
                      case.scale, min(geo.ctx[B - 1], nsplit * P), out=o.out, splits=(nsplit, P))
        tag = f"{what} splits ({nsplit}, {P})"
        AC.assert_exact(case, o.out, tag)
        o.check(tag)


@pytest.mark.parametrize("kv8", CACHES)
@pytest.mark.parametrize("nh,nkv,bs", with_bs32(DECODE_HEADS))
@pytest.mark.parametrize("D", [64, 128, 256])
def test_decode_exact(D, nh, nkv, bs, kv8):
    ctx, dflt = decode_plan(D, nkv, bs)
    geo = AC.geometry(ctx, bs=bs, seed=D + nh)
    cover = geo.table.shape[1] * bs
    splits_list = [(1, cover), dflt, (3, 256), (3, 272)]
    edges = (64, 256, 272, 512, 544, dflt[1], 2 * dflt[1])
    cases = [AC.census(geo, nh, nkv, D, p, kv8=kv8, device=dev) for p in (0, 1)]
    cases += [AC.needle(geo, nh, nkv, D, AC.decode_needles(geo, nkv, edges, rot), kv8=kv8, device=dev, seed=rot)
              for rot in range(3)]
    try:
        for unroll in ((0, 2, 12) if kv8 else (0, 1, 2, 4, 12, 14)):
            H.lib().attn_decode_set_unroll(unroll)
            for i, case in enumerate(cases):
                decode_launches(case, geo, splits_list, f"unroll {unroll} case {i}")
    finally:
        H.lib().attn_decode_set_unroll(0)


@pytest.mark.parametrize("kv8", CACHES)
def test_decode_long_partition(kv8):
    """One partition longer than 4096 tokens: more pages than the LDS staging holds (npg = 257 > 256), so every
    token's page id comes straight from the block table."""
    D, nh, nkv, n = 128, 8, 1, 4100
    geo = AC.geometry([n], bs=16, seed=11)
    assert (n + 15) // 16 > 256
    cases = [AC.census(geo, nh, nkv, D, 0, base=128, kv8=kv8, device=dev)]
    cases += [AC.needle(geo, nh, nkv, D, [[t]], kv8=kv8, device=dev) for t in (0, 4097, n - 1)]
    for i, case in enumerate(cases):
        decode_launches(case, geo, [(1, 4112)], f"long case {i}")


def test_decode_refuses_bad_out():
    """out is validated before the launch: dtype, unit inner stride, at least [B, nh * D]."""
    D, nh, nkv = 64, 4, 2
    geo = AC.geometry([5, 17], bs=16)
    case = AC.census(geo, nh, nkv, D, device=dev)
    args = (case.q, case.k_cache, case.v_cache, geo.table.to(dev), geo.ctx_lens.to(dev), nh, nkv, D, case.scale, 17)
    good = torch.empty(2, nh * D, dtype=torch.bfloat16, device=dev)
    for bad, msg in ((good.float(), "bfloat16"), (good.t().contiguous().t(), "contiguous"), (good[:1], "out shape"),
                     (good[:, : nh * D - 8], "out shape"), (good.cpu(), "GPU")):
        with pytest.raises(ValueError, match=msg):
            H.attn_decode(*args, out=bad)
    AC.assert_exact(case, H.attn_decode(*args, out=good), "dense out")


# ---------------------------------------------------------------------------------------------- extend
def extend_launch(case, geo, max_qlen, what, twin=False):
    nh, nkv, D = case.nh, case.nkv, case.D
    args = (case.q, case.k_cache, case.v_cache, geo.table.to(dev), geo.cu_q.to(dev), geo.ctx_lens.to(dev), max_qlen,
            nh, nkv, D, case.scale)
    assert case.q.stride(0) == case.q.shape[1] + AC.PAD  # the poisoned pad columns
    o = NanOut(geo.T, nh * D)
    H.attn_extend(*args, out=o.out)
    AC.assert_exact(case, o.out, what)
    o.check(what)
    if twin:  # the fp8 twin is an extra output: the bf16 one stays bit-identical
        dense = torch.full((geo.T, nh * D), float("nan"), dtype=torch.bfloat16, device=dev)
        H.attn_extend(*args, out=dense, fp8_out=True)
        assert torch.equal(dense, o.out), f"{what}: fp8_out changes the bf16 output"


def extend_cases(geo, nh, nkv, D, kv8, edges, rots, base=64, passes=(0, 1)):
    cases = [AC.census(geo, nh, nkv, D, p, base=base, kv8=kv8, device=dev) for p in passes]
    for rot in range(rots):
        strong, weak = AC.chunk_needles(geo, nkv, edges, rot)
        cases.append(AC.needle(geo, nh, nkv, D, strong, weak, kv8=kv8, device=dev, seed=rot))
    return cases


@pytest.mark.parametrize("kv8", CACHES)
@pytest.mark.parametrize("nh,nkv,bs", with_bs32(EXTEND_HEADS))
@pytest.mark.parametrize("D", [64, 128, 256])
def test_extend_exact(D, nh, nkv, bs, kv8):
    G = nh // nkv
    GE = max(ge for ge in range(1, min(G, 64) + 1) if G % ge == 0)  # slots of one row; 64 // GE rows a workgroup
    twin = H.extend_fp8_twin_ok(nh, nkv)
    geo = AC.geometry([p + c for p, c in EXTEND_CHUNKS], [c for _, c in EXTEND_CHUNKS], bs=bs, seed=D + nh)
    for i, case in enumerate(extend_cases(geo, nh, nkv, D, kv8, (16, 32, 64, 64 // GE, 2 * (64 // GE)), 3)):
        extend_launch(case, geo, max(geo.qlen), f"chunks case {i}", twin)
    # the same kernel as the decode step of a GQA model: one row per sequence
    geo = AC.geometry(EXTEND_DECODE_CTX, bs=bs, seed=D + nh + 1)
    for i, case in enumerate(extend_cases(geo, nh, nkv, D, kv8, (), 1)):
        extend_launch(case, geo, 1, f"decode batch case {i}", twin)


@pytest.mark.parametrize("kv8", CACHES)
def test_extend_long_context(kv8):
    """More than 512 pages per sequence (npg = 513): page ids straight from the block table."""
    D, nh, nkv = 128, 8, 1
    geo = AC.geometry([8208, 8208], [8, 1], bs=16, seed=12)
    assert (8208 + 15) // 16 > 512
    cases = [AC.census(geo, nh, nkv, D, 0, base=128, kv8=kv8, device=dev)]
    # weak needle at key 0, then in page 512 just before the chunk; the strong one inside the chunk
    cases.append(AC.needle(geo, nh, nkv, D, [[8203], [8207]], [[0], [0]], kv8=kv8, device=dev))
    cases.append(AC.needle(geo, nh, nkv, D, [[8200], [8207]], [[8195], [8193]], kv8=kv8, device=dev, seed=1))
    for i, case in enumerate(cases):
        extend_launch(case, geo, 8, f"long case {i}", True)


# --------------------------------------------------------------------------------------------- prefill
@pytest.mark.parametrize("nh,nkv", PREFILL_HEADS)
@pytest.mark.parametrize("D", [64, 128, 256])
def test_prefill_exact(D, nh, nkv):
    cases = []
    for lens in (PREFILL_LENS, PREFILL_BATCH8):
        geo = AC.packed_geometry(lens)
        cases += [AC.census(geo, nh, nkv, D, p, device=dev) for p in (0, 1)]
        for rot in range(2):
            strong, weak = AC.chunk_needles(geo, nkv, (16, 32, 64, 128), rot)
            cases.append(AC.needle(geo, nh, nkv, D, strong, weak, device=dev, seed=rot))
    try:
        for version, waves in PREFILL_VARIANTS:
            H.lib().attn_prefill_set_version(version)
            H.lib().attn_prefill_set_waves(waves)
            for i, case in enumerate(cases):
                geo = case.geo
                assert case.qkv.stride(0) == case.qkv.shape[1] + AC.PAD  # the poisoned pad columns
                for slack in (0, 70):  # max_seqlen exact, then larger than every sequence: blocks with q0 >= len
                    what = f"v{version} waves {waves} case {i} max_seqlen +{slack}"
                    o = NanOut(geo.T, nh * D)
                    H.attn_prefill(case.qkv, geo.cu_q.to(dev), max(geo.ctx) + slack, nh, nkv, D, case.scale, out=o.out)
                    AC.assert_exact(case, o.out, what)
                    o.check(what)
    finally:
        H.lib().attn_prefill_set_version(3)
        H.lib().attn_prefill_set_waves(0)


# ------------------------------------------------------------ random data, error relative to the signal
def signal_bound(case, out, what):
    """The kernel's largest (row, head) error, relative to the RMS of the fp32 oracle for that (row, head), is at
    most 4 x the same figure of the oracle with P and the output rounded to bf16 (4: the summation order of split
    partitions and token slots differs). The emulation is the yardstick; the kernel is never used for it."""
    ref = AC.oracle(case)
    emu = AC.signal_error(AC.oracle(case, emulate=True), ref, case.nh, case.D)
    got = AC.signal_error(out, ref, case.nh, case.D)
    print(f"{what}: kernel {got:.4g}, bf16 emulation {emu:.4g}, bound {4 * emu:.4g}")
    assert got <= 4 * emu, f"{what}: error / signal {got:.4g} > 4 x {emu:.4g}"


@pytest.mark.parametrize("kv8", CACHES)
def test_decode_signal_relative(kv8):
    """Contexts 1000, 1100, 1536, D = 128, 8 / 2 heads: the output RMS is ~0.05, where atol 2e-2 is blind.
    bf16 emulation, measured: 0.0112 (bf16 cache), 0.0125 (fp8 cache)."""
    geo = AC.geometry([1000, 1100, 1536], bs=16, seed=1)
    case = AC.random_case(geo, 8, 2, 128, kv8=kv8, device=dev, seed=5)
    for splits in (None, (1, 1536), (3, 512)):
        out = H.attn_decode(case.q, case.k_cache, case.v_cache, geo.table.to(dev), geo.ctx_lens.to(dev), 8, 2, 128,
                            case.scale, 1536, splits=splits)
        signal_bound(case, out, f"decode splits {splits}")


@pytest.mark.parametrize("kv8", CACHES)
def test_extend_signal_relative(kv8):
    """(prefix, chunk) = (1000, 64) and (1500, 8), D = 128, 8 / 2 heads.
    bf16 emulation, measured: 0.0134 (bf16 cache), 0.0128 (fp8 cache)."""
    geo = AC.geometry([1064, 1508], [64, 8], bs=16, seed=2)
    case = AC.random_case(geo, 8, 2, 128, kv8=kv8, device=dev, seed=5)
    out = H.attn_extend(case.q, case.k_cache, case.v_cache, geo.table.to(dev), geo.cu_q.to(dev), geo.ctx_lens.to(dev),
                        64, 8, 2, 128, case.scale)
    signal_bound(case, out, "extend")


def test_prefill_signal_relative():
    """Lengths 1100 and 37, D = 128, 4 / 2 heads. bf16 emulation, measured: 0.0160."""
    geo = AC.packed_geometry([1100, 37])
    case = AC.random_case(geo, 4, 2, 128, device=dev, seed=5)
    try:
        for version, waves in PREFILL_VARIANTS:
            H.lib().attn_prefill_set_version(version)
            H.lib().attn_prefill_set_waves(waves)
            out = H.attn_prefill(case.qkv, geo.cu_q.to(dev), 1100, 4, 2, 128, case.scale)
            signal_bound(case, out, f"prefill v{version} waves {waves}")
    finally:
        H.lib().attn_prefill_set_version(3)
        H.lib().attn_prefill_set_waves(0)
