"""The GEMM plan, host side only (the extension loads without a GPU): ops/plans.py against the native table and
resolver (csrc/gemm_plan.h, ``gemm_resolve``), and the recorded predictor rows of the dispatch before it was
restructured (tests/golden/gemm_plan_rows.txt, written by tests/plan_cases.py) replayed through this build."""
import ast
import os

import pytest

import plan_cases as PC
from llmss_amd.ops import autotune as A
from llmss_amd.ops import hip as H
from llmss_amd.ops import plans as P

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gemm_plan_rows.txt")
BIG_WS = 1 << 40


def _rows():
    with open(GOLDEN) as f:
        return [line.rstrip("\n").split(" = ") for line in f]


def test_constants_stay_importable_where_they_were():
    assert A.PACKED == H.PACKED_HINT == P.PACKED == 2048 << 8
    assert H.W8A8_FLAG == P.W8A8 == 1 << 20 and H.W8A8_ILV == P.ILV == 512 << 8
    assert H.MID_TILE_BN == {7: 48, 8: 128, 9: 128, 10: 256, 11: 128, 12: 256, 13: 192, 14: 32, 15: 96}
    assert A.ILV_MIN_M == 128 and A.FINALISTS == 6 and A.packed_twin is P.packed_twin


@pytest.mark.parametrize("t", P.TILES, ids=lambda t: f"{t.family}{t.code}")
def test_python_tile_table_matches_the_native_one(t):
    lib = H.lib()
    dec = t.family == "dec"
    M = 64 if dec else 512
    e = lib.gemm_resolve(M, 4096, 4096, nt_hint=P.tile_hint(t.code, P.D2, P.DEC if dec else 0), split_hint=1,
                         ws_bytes=BIG_WS)
    assert (e["family"], e["tile"], e["bm"], e["bn"], e["threads"]) == (t.family, t.code, t.bm, t.bn, t.threads)
    # packed variant: the native resolver takes the packed bit exactly on the tiles the table marks
    def packed_ok():
        try:
            return lib.gemm_resolve(64, 4096, 4096, nt_hint=P.tile_hint(t.code, P.D2, P.PACKED | (P.DEC if dec else 0)),
                                    split_hint=1, ws_bytes=BIG_WS, has_packed=True)["packed"]
        except RuntimeError:
            return False
    assert packed_ok() == t.packed
    # K % 8: accepted exactly on the tiles marked k8
    def k8_ok():
        try:
            lib.gemm_resolve(M, 4096, 4096 + 8, nt_hint=P.tile_hint(t.code, P.D2, P.DEC if dec else 0), split_hint=1,
                             ws_bytes=BIG_WS)
            return True
        except RuntimeError:
            return False
    assert k8_ok() == t.k8
    q = lib.gemm_resolve(M, 4096, 4096, nt_hint=P.tile_hint(t.code, P.D2, P.DEC if dec else 0), split_hint=1,
                         ws_bytes=BIG_WS, qkv_D=128, rope=False)
    assert (not q["qkv_cannot"]) == t.qkv


def test_native_table_has_no_tile_python_lacks():
    lib = H.lib()
    for dec in (False, True):
        for code in range(1, 16):
            try:
                e = lib.gemm_resolve(64, 4096, 4096, nt_hint=P.tile_hint(code, P.D2, P.DEC if dec else 0), split_hint=1,
                                     ws_bytes=BIG_WS)
            except RuntimeError:
                assert P.tile(code, dec) is None, (code, dec)
                continue
            assert P.tile(code, dec) is not None and P.tile(code, dec).bn == e["bn"], (code, dec)


@pytest.mark.parametrize("M", PC.MS)
def test_decode_and_packed_twin_match_the_native_resolver_on_every_candidate(M):
    lib = H.lib()
    n = 0
    for N, K, glu, fp8 in PC.SHAPES:
        for nt, s in PC.pairs(A, M, N, K, glu, fp8):
            h = P.decode(nt)
            if h.w8a8 or not nt:
                continue
            try:
                e = lib.gemm_resolve(M, N, K, fp8=fp8, glu=glu, nt_hint=nt, split_hint=s, ws_bytes=BIG_WS,
                                     has_packed=True)
            except RuntimeError:
                e = None
            if e is not None and nt & P.STREAM_MASK:
                assert (e["nt"], e["variant"]) == (max(h.nt, 2) if glu else h.nt, h.variant or 2)
            elif e is not None and not fp8:  # (fp8 weights run 8-wave / gemm_mid hints on the 128x128 tile)
                t = P.tile(h.tile, h.dec)
                assert (e["tile"], e["bm"], e["bn"], e["packed"]) == (h.tile, t.bm, t.bn, h.packed), hex(nt)
                assert e["ilv"] == (h.ilv and t.family == "mid")
                assert (e["family"] == "stream_k") == (h.streamk and t.family == "tiled")
            # packed_twin: exactly the plans the resolver runs with the packed bit added, on the same tile
            twin = P.packed_twin(M, nt, fp8)
            if h.packed:
                continue
            try:
                ep = lib.gemm_resolve(M, N, K, fp8=fp8, glu=glu, nt_hint=nt | P.PACKED, split_hint=s, ws_bytes=BIG_WS,
                                      has_packed=True)
            except RuntimeError:
                ep = None
            # (the interleaved ring and default-policy weights are refused by the gemm_mid launcher, not the resolver)
            if ep is not None and not (h.ilv or h.default_w):
                assert twin == nt | P.PACKED, hex(nt)
                assert e is not None and (ep["tile"], ep["split"], ep["finish"]) == (e["tile"], e["split"], e["finish"])
            if twin is not None:
                assert ep is not None and ep["packed"], hex(nt)
            n += 1
    assert n > 100


def test_describe_names_every_candidate():
    for nt, s in PC.pairs(A, 64, 12288, 4096, False, False) + PC.pairs(A, 512, 10240, 8192, False, True):
        d = P.describe(nt, s)
        assert d and "bad tile" not in d, (hex(nt), d)
    assert P.describe(P.tile_hint(11, P.D3, P.COMBINE | P.PACKED), 4) == "mid 64x128 3 stages split 4 combine packed"
    assert P.describe(P.w8a8_hint(13, 4, P.ILV), 2) == "mid 64x192 4 stages split 2 w8a8 ilv"


def test_recorded_rows_cover_every_field():
    """The sample keeps every M x shape, every hint bit and tile code of the candidate lists, every workspace size."""
    keys = [k.split() for k, _ in _rows()]
    assert {(int(k[1]), int(k[2]), int(k[3])) for k in keys} == {(M, N, K) for M in PC.MS for N, K, _, _ in PC.SHAPES}
    full = {nt for M in PC.MS for N, K, glu, fp8 in PC.SHAPES for nt, _ in PC.pairs(A, M, N, K, glu, fp8)}
    got = {int(k[6], 16) for k in keys if k[0] == "slabs"} | {int(k[5], 16) for k in keys if k[0] == "plan"}
    bits = lambda hs: {b for h in hs for b in range(24) if h >> b & 1}
    tiles = lambda hs: {(P.decode(h).tile, P.decode(h).dec, P.decode(h).w8a8) for h in hs}
    assert bits(got) == bits(full) and tiles(got) == tiles(full)
    for kind in ("slabs", "f8slabs"):
        assert {int(k[-1]) for k in keys if k[0] == kind} == set(PC.WS)
    assert {int(k[5]) for k in keys if k[0] == "f8slabs"} == set(range(16))
    assert os.path.getsize(GOLDEN) <= 200_000


def test_recorded_rows_replay_unchanged():
    lib = H.lib()
    rows = _rows()
    assert len(rows) > 3000
    bad = [(k, v, got) for k, v in rows if (got := PC.replay(lib, k)) != ast.literal_eval(v)]
    assert not bad, bad[:10]
