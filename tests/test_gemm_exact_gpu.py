"""Every GEMM plan family against inputs whose bf16 output is known to the bit (tests/gemm_cases.py; the checks
are proven able to fail in tests/test_gemm_cases_cpu.py): tolerance 0 on the integer, probe and saturated cases, the
derived bracket on the midrange activations. Outputs are NaN-filled before every call. RoPE and the fused QKV epilogue
run with quarter-turn tables, where rotation is a signed permutation."""
import pytest
import torch

import gemm_cases as G
from llmss_amd.ops import hip as H
from llmss_amd.ops import reference as R

pytestmark = pytest.mark.gpu
dev = "cuda"
PLANS = G.plans()


def _dev(t):
    return None if t is None else t.to(dev)


def _x(c):
    return H.MxAct(c.mx[0].to(dev), c.mx[1].to(dev)) if c.mx is not None else c.x.to(dev)


def run(c, p, **extra):
    """One case through one plan; the output buffer starts as NaN."""
    kw = dict(p.kw)
    kw.update(extra)
    y = torch.full((c.shape[0], c.nout), float("nan"), dtype=torch.bfloat16, device=dev)
    if p.api == "w8a8":
        return H.linear_w8a8(_x(c), c.w.to(dev), c.w_scale.to(dev), _dev(c.bias), act=c.act, glu=c.glu, out=y, **kw)
    return H.linear(_x(c), c.w.to(dev), _dev(c.bias), act=c.act, glu=c.glu, w_scale=_dev(c.w_scale), out=y, **kw)


@pytest.mark.parametrize("p", PLANS, ids=[p.id for p in PLANS])
def test_plan_exact(p):
    """Per plan: integer operands with no activation + bias and relu + bias, saturated GELU (tanh, erf), saturated
    SwiGLU + bias where the plan has a SwiGLU epilogue, the x and w one-hot probes, one midrange case per activation."""
    for c in G.battery(p):
        G.assert_exact(c, run(c, p), p.id)


def _split_plans():
    """Every plan with a split and a separate reduce; whether such a call leaves slabs is the library's decision."""
    want = {("tiled", "bf16"), ("mid", "bf16"), ("dec", "bf16"), ("stream", "bf16"), ("tiled", "w8a16"),
            ("stream", "w8a16"), ("w8a8", "w8a8"), ("w8a8-mid", "w8a8"), ("mx-in", "mx")}
    out = []
    for p in PLANS:
        kw = dict(p.kw)
        comb = p.api == "linear" and (kw.get("nt_hint", 0) >> 8) & 256
        if (p.family, p.flavour) in want and kw.get("split_hint", kw.get("split", 1)) > 1 and not comb:
            out.append(p)
    return out


SPLIT_PLANS = _split_plans()


@pytest.mark.parametrize("p", SPLIT_PLANS, ids=[p.id for p in SPLIT_PLANS])
def test_partial_slabs_exact(p):
    """partial_ok=True: where gemm_partial_slabs / gemm_f8f8_partial_slabs say the call leaves S slabs, it returns a
    PartialSum of S slabs, every fp32 slab holds integers of the case's grid, and the slabs summed in fp32 equal the
    exact integer sum (the bias is added after the sum, by the consumer); where they say 0 (a split clamped to one
    k-step), the finished output is exact. The workspace is NaN-poisoned first, as in tests/test_kernels_gpu.py."""
    c = G.integer_case(p.M, p.N, p.K, p.flavour, "none", True, p.K > 64)
    M, N, K = c.shape
    ws = H._GEMM_WS.get(64 << 20, dev)
    ws.fill_(float("nan"))
    kw = dict(p.kw)
    if p.api == "w8a8":
        S = H.lib().gemm_f8f8_partial_slabs(M, N, K, False, 0, kw["tile"], kw["split"], ws.numel() * 4)
        r = H.linear_w8a8(_x(c), c.w.to(dev), c.w_scale.to(dev), _dev(c.bias), partial_ok=True, **kw)
    else:
        S = H.lib().gemm_partial_slabs(M, N, K, c.w_scale is not None, False, 0, kw["nt_hint"], kw["split_hint"],
                                       ws.numel() * 4)
        r = H.linear(_x(c), c.w.to(dev), _dev(c.bias), w_scale=_dev(c.w_scale), partial_ok=True, **kw)
    if S == 0:
        assert not isinstance(r, H.PartialSum), p.id
        G.assert_exact(c, r, p.id)
        return
    assert isinstance(r, H.PartialSum) and r.S == S > 1, (p.id, S)
    slabs = r.buf[: r.S * M * N].view(r.S, M, N).clone()
    units = G._units(c)
    grid = slabs.cpu().double() / units
    assert torch.equal(grid, grid.round()), f"{p.id}: a slab holds a value off the integer grid"
    want = (c.z - c.bias64).float()
    assert torch.equal(want.double(), c.z - c.bias64)
    assert torch.equal(slabs.sum(0).cpu(), want), p.id
    assert torch.equal((slabs.sum(0).cpu() + c.bias.float()).to(torch.bfloat16), c.expected), p.id


def _mx_out(c, tile):
    M, F2 = c.shape[0], c.shape[1]
    mx = H.linear_w8a8(c.x.to(dev), c.w.to(dev), c.w_scale.to(dev), c.bias.to(dev), glu=True, tile=tile, depth=3,
                       split=1, mx_out=True)
    assert isinstance(mx, H.MxAct) and mx.q.shape == (M, F2 // 2) and mx.s.shape == (M, F2 // 64)
    rq, rs = R.quant_mx_fp8(c.expected.float())
    assert torch.equal(mx.s.cpu(), rs), f"{c.what}: block scales"
    assert torch.equal(mx.q.cpu(), rq), f"{c.what}: e4m3 bytes"
    return mx


@pytest.mark.parametrize("tile", [8, 11, 10, 13, 9, 12])
@pytest.mark.parametrize("M", [37, 129, 257])
def test_mx_output_and_down_projection_exact(tile, M):
    """mx_out=True on saturated SwiGLU + bias: (q, s) bit-equal to the CPU MX quantisation of the exact output, for the
    general case and for the one whose MX form is lossless; the down projection fed with the latter MxAct is exact on
    every gemm_mid tile; fed with the former, whose e4m3 values span more than the fp8 MFMA adds exactly, it stays
    within the allowance gemm_cases.mx_wide_down_case derives."""
    F2, K, Nd = 256, 1024, 136
    wide_mx, wide = _mx_out(G.swiglu_case(M, F2, K, "w8a8"), tile), G.mx_wide_down_case(M, F2, K, Nd)
    for dt, depth, split, ilv in [(8, 3, 1, False), (11, 4, 3, True), (14, 4, 1, False), (12, 3, 1, False)]:
        y = torch.full((M, Nd), float("nan"), dtype=torch.bfloat16, device=dev)
        H.linear_w8a8(wide_mx, wide.w.to(dev), wide.w_scale.to(dev), None, out=y, tile=dt, depth=depth, split=split,
                      ilv=ilv)
        G.assert_exact(wide, y, f"wide down tile {dt} depth {depth} split {split} ilv {ilv}")
    mx = _mx_out(G.mx_swiglu_case(M, F2, K), tile)
    down = G.mx_down_case(M, F2, K, Nd)
    for dt, depth, split, ilv in [(8, 3, 1, False), (8, 4, 1, True), (11, 4, 3, True), (10, 3, 1, False),
                                  (13, 5, 2, True), (14, 4, 1, False), (15, 3, 3, True), (7, 4, 1, False),
                                  (9, 3, 2, False), (12, 3, 1, False)]:
        y = torch.full((M, Nd), float("nan"), dtype=torch.bfloat16, device=dev)
        H.linear_w8a8(mx, down.w.to(dev), down.w_scale.to(dev), None, out=y, tile=dt, depth=depth, split=split, ilv=ilv)
        G.assert_exact(down, y, f"down tile {dt} depth {depth} split {split} ilv {ilv}")


# ------------------------------------------------------------------------------------ RoPE / KV write
ROPE = [("neox", 128, 128, 4, 2), ("gptj", 64, 32, 4, 2), ("neox", 64, 32, 4, 1), ("gptj", 64, 64, 2, 2)]


def _nan_caches(rc):
    kc = torch.full((rc.nb, rc.nkv, rc.bs, rc.D), float("nan"), dtype=torch.bfloat16, device=dev)
    return kc, torch.full_like(kc, float("nan"))


@pytest.mark.parametrize("style,D,rot,nh,nkv", ROPE)
@pytest.mark.parametrize("T", [1, 19, 130])
def test_rope_cache_exact(style, D, rot, nh, nkv, T):
    """H.rope_cache == R.rope_cache to the bit under quarter-turn tables: neox, gptj, partial rotation, a skipped
    slot, NaN caches whose unwritten rows stay NaN."""
    rc = G.rope_case(T, nh, nkv, D, rot, style)
    kc, vc = _nan_caches(rc)
    q = rc.qkv.to(dev)
    H.rope_cache(q, rc.positions.to(dev), rc.cos.to(dev), rc.sin.to(dev), kc, vc, rc.slots.to(dev), nh, nkv, D, rot,
                 style)
    wq, wk, wv = G.rope_expected(rc, rc.qkv)
    assert not torch.equal(wq, rc.qkv) or T == 1
    G.assert_same_bits(q, wq, "qkv")
    G.assert_same_bits(kc, wk, "k cache")
    G.assert_same_bits(vc, wv, "v cache")


QKV_HINTS = ([(f"mid{t}", (t | 16) << 8, G.MID_DIMS[t]) for t in G.MID_DIMS]
             + [(f"tile{t}", (t | 16) << 8, G.TILE_DIMS[t]) for t in (1, 2, 3)]
             + [(f"dec{c}", (c | 16 | 1024) << 8, (64, G.DEC_BN[c])) for c in G.DEC_BN])
QKV_STYLES = [("neox", 32, 32, 8, 4), ("gptj", 64, 32, 4, 2), ("neox", 64, 32, 4, 2), ("none", 64, 0, 4, 2)]


@pytest.mark.parametrize("name,hint,dims", QKV_HINTS, ids=[h[0] for h in QKV_HINTS])
@pytest.mark.parametrize("split", [1, 3])
@pytest.mark.parametrize("style,D,rot,nh,nkv", QKV_STYLES)
def test_linear_qkv_exact(name, hint, dims, split, style, D, rot, nh, nkv):
    """The fused QKV epilogue with integer operands: q and every cache row it writes are bit-equal to the exact GEMM +
    R.rope_cache; unwritten cache rows stay NaN. The hints carry no combine bit: launch_gemm_qkv (csrc/gemm.hip) turns a
    split plan into an in-launch combine itself, because the epilogue needs finished sums. Plans the epilogue cannot take
    (neox on a tile narrower than a head) return None."""
    bm, bn = dims
    T = 33 if name.startswith("dec") else G.ROWS[bm][-1]
    N, K = (nh + 2 * nkv) * D, 336
    c = G.integer_case(T, N, K, "bf16", "none", True, True)
    do_rope = style != "none"
    st = "gptj" if style == "gptj" else "neox"
    rc = G.rope_case(T, nh, nkv, D, rot if do_rope else D, st)
    kc, vc = _nan_caches(rc)
    y = H.linear_qkv(c.x.to(dev), c.w.to(dev), c.bias.to(dev), rc.positions.to(dev), rc.cos.to(dev), rc.sin.to(dev),
                     kc, vc, rc.slots.to(dev), nh, nkv, D, rot, st, do_rope, nt_hint=hint, split_hint=split)
    if do_rope and st == "neox" and bn % D:
        assert y is None
        return
    assert y is not None
    wq, wk, wv = G.rope_expected(rc, c.expected, do_rope=do_rope)
    G.assert_same_bits(y, wq, f"{name} qkv")
    G.assert_same_bits(kc, wk, f"{name} k cache")
    G.assert_same_bits(vc, wv, f"{name} v cache")
