"""Panel-packed weights for the decode GEMMs (hint bit 2048, csrc/gemm.hip kPackedHint).

* the device packer (csrc/pack.hip) equals the reference packer bit for bit;
* a packed plan's output is bit-identical to the same (kernel, tile, depth, split) on the row-major weight, for every
  gemm_dec width and every gemm_mid decode tile the autotuner lists, through every epilogue, into NaN-filled buffers
  (nothing past M or N is written); integer and saturated SwiGLU cases tie the packed plans to the exact oracle too;
* a packed hint that cannot be honoured raises."""
import pytest
import torch

import gemm_cases as G
from llmss_amd.ops import hip as H
from llmss_amd.ops import reference as R

pytestmark = pytest.mark.gpu
dev = "cuda"
PK = H.PACKED_HINT

# (id, nt_hint): gemm_dec widths 16 / 32 / 48 / 64 at the autotuner's depth code, and its (tile, depth) list of the
# 64-row gemm_mid tiles (ops/autotune.py candidates, M <= 64)
KERNELS = [(f"dec{bn}", (code | 32 | 1024) << 8) for code, bn in ((1, 16), (2, 32), (3, 48), (4, 64))] + \
          [(f"mid{t}d{d}", (t | d) << 8) for t, d in ((10, 16), (11, 16), (11, 32), (13, 16), (13, 32), (14, 32),
                                                       (14, 48), (15, 16), (15, 32), (7, 32), (7, 48))]
MS, NS, KS = (1, 7, 64), (16, 40, 80, 208), (64, 192, 200, 520)
SPLITS = (1, 2, 4)
PACK_SHAPES = [(16, 64), (40, 200), (80, 192), (208, 72)]

_cache = {}


def _operands(M, N, K):
    """Seeded bf16 x [M, K], w [N, K], bias [N] on the GPU and the packed twin of w, made once per shape."""
    key = (N, K)
    if key not in _cache:
        g = torch.Generator().manual_seed(7 * N + K)
        w = (torch.randn(N, K, generator=g) * K ** -0.5).to(torch.bfloat16).to(dev)
        b = torch.randn(N, generator=g).to(torch.bfloat16).to(dev)
        x = (torch.randn(64, K, generator=g) * 0.5).to(torch.bfloat16).to(dev)
        _cache[key] = (x, w, b, H.pack_panels(w))
    x, w, b, wp = _cache[key]
    return x[:M], w, b, wp


def _bits(t):
    return t.contiguous().view(torch.int16)


def _nan_out(M, n):
    """A NaN-filled [M + 1, n + 8] buffer and its [M, n] corner, the kernel's output."""
    buf = torch.full((M + 1, n + 8), float("nan"), dtype=torch.bfloat16, device=dev)
    return buf, buf[:M, :n]


def _check_pair(a, b, what):
    (ba, ya), (bb, yb) = a, b
    assert torch.isfinite(ya.float()).all(), f"{what}: the row-major plan left output unwritten"
    assert torch.equal(_bits(ya), _bits(yb)), f"{what}: packed output differs from the row-major plan's"
    M, n = ya.shape
    for buf in (ba, bb):
        assert buf[M:].isnan().all() and buf[:, n:].isnan().all(), f"{what}: wrote past M or N"


def _shapes(ns=NS):
    for M in MS:
        for N in ns:
            for K in KS:
                for s in SPLITS:
                    if s <= -(-K // 64):
                        yield M, N, K, s


# ------------------------------------------------------------------------------------ packer
@pytest.mark.parametrize("N,K", PACK_SHAPES)
def test_native_packer_equals_reference(N, K):
    g = torch.Generator().manual_seed(N * 1000 + K)
    w = torch.randn(N, K, generator=g).to(torch.bfloat16)
    got = H.pack_panels(w.to(dev))
    assert torch.equal(_bits(got).cpu(), _bits(R.pack_panels(w)))
    assert torch.equal(_bits(R.unpack_panels(got.cpu(), N, K)), _bits(w))


def test_native_packer_strided_source():
    g = torch.Generator().manual_seed(5)
    big = torch.randn(48, 264, generator=g).to(torch.bfloat16)
    for r0, c0, N, K in ((3, 8, 40, 200), (0, 3, 40, 200), (5, 0, 16, 64)):  # aligned rows, odd start, dense block
        w = big[r0:r0 + N, c0:c0 + K]
        got = H.pack_panels(big.to(dev)[r0:r0 + N, c0:c0 + K])
        assert torch.equal(_bits(got).cpu(), _bits(R.pack_panels(w))), (r0, c0, N, K)


# ------------------------------------------------------------------------------------ bit identity of plans
@pytest.mark.parametrize("name,hint", KERNELS, ids=[k[0] for k in KERNELS])
def test_plain_and_bias_gelu_identical(name, hint):
    for M, N, K, s in _shapes():
        x, w, b, wp = _operands(M, N, K)
        for bias, act in ((None, "none"), (b, "gelu_tanh")):
            r = _nan_out(M, N)
            H.linear(x, w, bias, act=act, out=r[1], nt_hint=hint, split_hint=s)
            p = _nan_out(M, N)
            H.linear(x, w, bias, act=act, out=p[1], nt_hint=hint | PK, split_hint=s, w_packed=wp)
            _check_pair(r, p, f"{name} M{M} N{N} K{K} s{s} {act}")


@pytest.mark.parametrize("name,hint", KERNELS, ids=[k[0] for k in KERNELS])
def test_swiglu_identical(name, hint):
    """SwiGLU needs N % 32 == 0, so the weight has 2 x (16, 48, 80, 208) rows: output widths that are no multiple of
    the tile. A tile that cannot pair gate and up columns refuses the row-major plan and the packed plan alike."""
    for M, N, K, s in _shapes((32, 96, 160, 416)):
        x, w, b, wp = _operands(M, N, K)
        r, p = _nan_out(M, N // 2), _nan_out(M, N // 2)
        try:
            H.linear(x, w, b, glu=True, out=r[1], nt_hint=hint, split_hint=s)
        except RuntimeError as e:
            assert "SwiGLU" in str(e)
            with pytest.raises(RuntimeError, match="SwiGLU"):
                H.linear(x, w, b, glu=True, out=p[1], nt_hint=hint | PK, split_hint=s, w_packed=wp)
            continue
        H.linear(x, w, b, glu=True, out=p[1], nt_hint=hint | PK, split_hint=s, w_packed=wp)
        _check_pair(r, p, f"{name} M{M} N{N} K{K} s{s} swiglu")


@pytest.mark.parametrize("name,hint", KERNELS, ids=[k[0] for k in KERNELS])
def test_partial_slabs_and_add_norm_identical(name, hint):
    """partial_ok: the fp32 split-K slabs the consumer sums are equal bit for bit, the partial-slab query answers the
    same for both hints, and add_norm over them gives the same rows and residual."""
    ws = H._GEMM_WS.get(64 << 20, dev)
    for M, N, K, s in _shapes():
        x, w, b, wp = _operands(M, N, K)
        q = [H.lib().gemm_partial_slabs(M, N, K, False, False, 0, h, s, ws.numel() * 4) for h in (hint, hint | PK)]
        assert q[0] == q[1], (name, M, N, K, s, q)
        g = torch.Generator().manual_seed(M + N)
        res0 = torch.randn(M, N, generator=g).to(torch.bfloat16).to(dev)
        nw = torch.randn(N, generator=g).to(torch.bfloat16).to(dev)
        outs = []
        for h, twin in ((hint, None), (hint | PK, wp)):
            ws.fill_(float("nan"))
            r = H.linear(x, w, b, nt_hint=h, split_hint=s, partial_ok=True, w_packed=twin)
            if q[0] == 0:
                assert not isinstance(r, H.PartialSum)
                outs.append((r.clone(),))
                continue
            assert isinstance(r, H.PartialSum) and r.S == q[0]
            slabs = r.buf[: r.S * M * N].clone()
            y, res = H.add_norm_partial(r, nw, None, 1e-5, True, res0.clone())
            outs.append((slabs, y.clone(), res.clone()))
        for a, c in zip(*outs):
            assert torch.isfinite(a.float()).all()
            assert torch.equal(a.view(torch.int16 if a.dtype == torch.bfloat16 else torch.int32),
                               c.view(torch.int16 if c.dtype == torch.bfloat16 else torch.int32)), (name, M, N, K, s)


@pytest.mark.parametrize("name,hint", KERNELS, ids=[k[0] for k in KERNELS])
def test_inlaunch_combine_identical(name, hint):
    for M, N, K, s in _shapes():
        if s == 1:
            continue
        x, w, b, wp = _operands(M, N, K)
        r, p = _nan_out(M, N), _nan_out(M, N)
        H.linear(x, w, b, act="gelu_tanh", out=r[1], nt_hint=hint | (256 << 8), split_hint=s)
        H.linear(x, w, b, act="gelu_tanh", out=p[1], nt_hint=hint | (256 << 8) | PK, split_hint=s, w_packed=wp)
        _check_pair(r, p, f"{name} M{M} N{N} K{K} s{s} combine")


@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("name,hint", KERNELS, ids=[k[0] for k in KERNELS])
def test_qkv_epilogue_identical(name, hint, D):
    """linear_qkv (RoPE + paged KV write in the epilogue; a split plan combines in the launch): q rows and every cache
    row equal, unwritten cache rows still NaN; plans the epilogue cannot take return None for both."""
    nh, nkv = 2, 1
    N = (nh + 2 * nkv) * D
    for style, rot in (("gptj", D // 2), ("neox", D)):
        for M in MS:
            rc = G.rope_case(M, nh, nkv, D, rot, style)
            for K in KS:
                for s in SPLITS:
                    if s > -(-K // 64):
                        continue
                    x, w, b, wp = _operands(M, N, K)
                    got = []
                    for h, twin in ((hint, None), (hint | PK, wp)):
                        kc = torch.full((rc.nb, nkv, rc.bs, D), float("nan"), dtype=torch.bfloat16, device=dev)
                        vc = torch.full_like(kc, float("nan"))
                        y = H.linear_qkv(x, w, b, rc.positions.to(dev), rc.cos.to(dev), rc.sin.to(dev), kc, vc,
                                         rc.slots.to(dev), nh, nkv, D, rot, style, True, nt_hint=h, split_hint=s,
                                         w_packed=twin)
                        got.append((y, kc, vc))
                    what = f"{name} D{D} {style} M{M} K{K} s{s}"
                    if got[0][0] is None:
                        assert got[1][0] is None, what
                        continue
                    assert got[1][0] is not None and torch.isfinite(got[0][0].float()).all(), what
                    written = int((~got[0][1].isnan()).sum())
                    assert written == int((rc.slots >= 0).sum()) * nkv * D, what
                    for a, c in zip(got[0], got[1]):
                        assert torch.equal(_bits(a), _bits(c)), what


@pytest.mark.parametrize("name,hint", KERNELS, ids=[k[0] for k in KERNELS])
def test_packed_plans_exact(name, hint):
    """The packed plans against the exact oracle (tests/gemm_cases.py), not only against their siblings."""
    cases = [(G.integer_case(33, 208, 336, "bf16", "none", True, True), 1),
             (G.integer_case(7, 40, 200, "bf16", "relu", True, True), 2),
             (G.swiglu_case(33, 416, 336, "bf16"), 1)]
    for c, s in cases:
        M, N, K = c.shape
        w = c.w.to(dev)
        y = torch.full((M, c.nout), float("nan"), dtype=torch.bfloat16, device=dev)
        try:
            H.linear(c.x.to(dev), w, c.bias.to(dev), act=c.act, glu=c.glu, out=y, nt_hint=hint | PK, split_hint=s,
                     w_packed=H.pack_panels(w))
        except RuntimeError as e:
            assert c.glu and "SwiGLU" in str(e), (name, c.what, e)  # a tile that cannot pair gate / up columns
            continue
        G.assert_exact(c, y, f"{name} packed split {s}")


# ------------------------------------------------------------------------------------ refusals
def test_refusals_raise():
    x, w, b, wp = _operands(64, 208, 192)
    dec, mid = (3 | 32 | 1024) << 8, (15 | 16) << 8
    y = torch.empty(64, 208, dtype=torch.bfloat16, device=dev)
    H.linear(x, w, None, out=y, nt_hint=dec | PK, w_packed=wp)  # honoured
    with pytest.raises(RuntimeError, match="packed"):  # the bit without the packed copy
        H.linear(x, w, None, out=y, nt_hint=dec | PK)
    # M = 65
    x65 = torch.zeros(65, 192, dtype=torch.bfloat16, device=dev)
    y65 = torch.empty(65, 208, dtype=torch.bfloat16, device=dev)
    for h in (dec, mid):
        with pytest.raises(RuntimeError, match="M <= 64"):
            H.linear(x65, w, None, out=y65, nt_hint=h | PK, w_packed=wp)
    # kernels without the variant: gemm_tiled 64x64, stream-K, the 128-row gemm_mid tile, the streaming kernel
    for h in ((3 | 16) << 8, (3 | 16 | 128) << 8, (8 | 16) << 8):
        with pytest.raises(RuntimeError, match="packed"):
            H.linear(x, w, None, out=y, nt_hint=h | PK, w_packed=wp)
    with pytest.raises(RuntimeError, match="packed"):
        H.linear(x[:16], w, None, out=y[:16], nt_hint=(2 + 16 * 2) | PK, w_packed=wp)
    with pytest.raises(RuntimeError, match="packed"):  # the interleaved ring
        H.linear(x, w, None, out=y, nt_hint=mid | (512 << 8) | PK, w_packed=wp)
    # fp8 weights
    q, sc = H.quant_fp8_rows(w)
    for h in (dec, mid):
        with pytest.raises(RuntimeError, match="packed|bf16"):
            H.linear(x, q, None, w_scale=sc, out=y, nt_hint=h | PK, w_packed=wp)
    # a packed buffer of the wrong shape never reaches the kernel
    with pytest.raises(ValueError, match="w_packed"):
        H.linear(x, w, None, out=y, nt_hint=dec | PK, w_packed=wp[:-1])


def test_tuned_packed_plan_without_twin_runs_the_sibling():
    """A tuned plan with the bit serves callers with a twin (packed) and without one (row-major sibling, same bits)."""
    M, N, K = 7, 208, 192
    x, w, b, wp = _operands(M, N, K)
    hint = (15 | 16) << 8
    lib = H.lib()
    prev = lib.gemm_tuned_get(M, N, K, False, 0)
    try:
        lib.gemm_tuned_set(M, N, K, False, 0, hint | PK, 2)
        assert lib.gemm_tuned_get(M, N, K, False, 0) == (hint | PK, 2)
        a = H.linear(x, w, b)
        c = H.linear(x, w, b, w_packed=wp)
        e = H.linear(x, w, b, nt_hint=hint, split_hint=2)
        assert torch.equal(_bits(a), _bits(e)) and torch.equal(_bits(c), _bits(e))
    finally:
        lib.gemm_tuned_set(M, N, K, False, 0, *(prev or (0, 0)))
