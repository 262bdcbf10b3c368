"""Proof that the exact GEMM suite (tests/gemm_cases.py, run on the GPU by tests/test_gemm_exact_gpu.py) can fail:
an fp64 evaluation of every case passes, and the same evaluation with one kernel mistake built in fails - on exactly
the elements the mistake touches wherever that set is well defined (the probes, whose outputs are bf16 numbers). One
test restates the toleranced check of tests/test_kernels_gpu.py and shows which of these mistakes it lets through."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import gemm_cases as G
from llmss_amd.ops import reference as R

SHAPES = [(37, 136, 336), (65, 160, 704), (17, 136, 1024)]  # 5 full k-steps + 16, 11 k-steps, 16 k-steps
FP8 = ("w8a16", "w8a8", "mx")


def emulate(c, mut="honest"):
    """fp64 evaluation of a case the way R.linear defines it, optionally with one mistake. Returns (bf16 output, z)."""
    xq, xsc, wq, ws, b = c.xq, c.xsc, c.wq, c.ws, c.bias64
    (M, K), N = xq.shape, wq.shape[0]
    act, mode = c.act, "rne"
    if mut == "w_scale_shift":
        ws = ws.roll(1)
    elif mut == "x_scale_shift":
        xsc = xsc.roll(1, 0)
    elif mut == "mx_block_shift":
        xsc = xsc.roll(32, 1)
    elif mut == "bias_shift":
        b = b.roll(1)
    elif mut in ("drop_k", "double_k"):  # one k of the last row, one that matters
        k = int((xq[M - 1] != 0).nonzero()[-1])
        xq = xq.clone()
        xq[M - 1, k] *= 0 if mut == "drop_k" else 2
    elif mut == "drop_tail_col":  # the partial last k-step of one column
        assert K % 64
        n = int((wq[:, K - K % 64:] != 0).any(1).nonzero()[-1])
        wq = wq.clone()
        wq[n, K - K % 64:] = 0
    x, w = xq * xsc, wq * ws[:, None]
    if mut == "bf16_slabs":
        ks = [K * i // 3 // 16 * 16 for i in range(3)] + [K]
        acc = sum(G.round_bf16(x[:, a:e] @ w[:, a:e].t()).double() for a, e in zip(ks, ks[1:]))
    elif mut == "bf16_acc":
        acc = torch.zeros(M, N, dtype=torch.float64)
        for k0 in range(0, K, 64):
            acc = G.round_bf16(acc + x[:, k0:k0 + 64] @ w[:, k0:k0 + 64].t()).double()
    else:
        acc = x @ w.t()
    if mut == "bias_after_round":
        z = G.round_bf16(acc).double() + b
    else:
        z = acc if b is None else acc + b
    if mut == "trunc":
        mode = "trunc"
    elif mut == "away":
        mode = "away"
    if c.ref64 is not None:  # midrange: the activation of the gate / of z
        name = "silu" if c.glu else {"erf_for_tanh": "gelu", "tanh_for_erf": "gelu_tanh"}.get(mut, act)
        zz = R.glu_split(z, -1)[0] if c.glu else z
        return G.round_bf16(G.act64_mid(zz, name), mode), z
    if c.glu:
        g, u = R.glu_split(z, -1)
        if mut == "glu_swapped":
            g, u = u, g
        elif mut == "glu_next_pair":
            u = u.roll(-16, 1)
        return G.round_bf16(F.silu(g) * u, mode), z
    return G.round_bf16(G.act64(z, act), mode), z


def must_fail(c, mut, exact_set=False, may_miss=False):
    """``may_miss``: the mistake may leave this case's sums as they are (bf16 slabs of a short K at +-4 are exact);
    the case must fail whenever a sum changed."""
    out, z = emulate(c, mut)
    bad = G.mismatch(c, out)
    if may_miss and torch.equal(z, c.z):
        assert not bool(bad.any())
        return
    assert bool(bad.any()), f"{mut} passes {c.what} {c.shape}"
    with pytest.raises(AssertionError, match="elements wrong"):
        G.assert_exact(c, out, mut)
    if not c.glu and c.ref64 is None:
        touched = z != c.z
        if not bool(touched.any()):  # a mistake of the rounding, not of the sum
            return
        assert not bool((bad & ~touched).any()), f"{mut}: an untouched element fails"
        if exact_set:
            assert torch.equal(bad, touched), f"{mut}: {int(bad.sum())} fail, {int(touched.sum())} touched"


def flavour_shapes(flavours=G.FLAVOURS):
    return [(f, s) for f in flavours for s in SHAPES if not (f == "mx" and s[2] % 128)]


# ------------------------------------------------------------------------------------ the honest oracle
def test_every_case_of_every_plan_builds_and_the_honest_oracle_passes():
    """Builds every case the GPU file runs (the builders assert the 2^24 bound, the inexact and tie shares, anchor
    exactness and saturation) and passes each through the fp64 evaluation."""
    seen, kinds, fams = set(), set(), set()
    for p in G.plans():
        fams.add(p.family)
        for c in G.battery(p):
            if id(c) in seen:
                continue
            seen.add(id(c))
            if (c.what, c.shape[2]) not in kinds:  # one evaluation per builder, flavour, activation and K
                kinds.add((c.what, c.shape[2]))
                G.assert_exact(c, emulate(c)[0], p.id)
    assert fams == {"default", "stream", "tiled", "pingpong", "mid", "dec", "streamk", "w8a8", "w8a8-mid", "mx-in"}
    assert len(seen) > 1000


@pytest.mark.parametrize("M", [37, 257])
def test_mx_output_cases(M):
    up, down = G.mx_swiglu_case(M, 256, 1024), G.mx_down_case(M, 256, 1024, 136)
    G.assert_exact(up, emulate(up)[0])
    G.assert_exact(down, emulate(down)[0])
    must_fail(down, "mx_block_shift")
    must_fail(down, "trunc")
    must_fail(up, "glu_swapped")


@pytest.mark.parametrize("M", [37, 257])
def test_mx_wide_down_case_still_catches_wrong_scales(M):
    """The toleranced wide-span down projection: the exact sum passes, so does a sum that drops every product more
    than 2^12 below its block's largest; a scale from the neighbouring block or row and a dropped k fail."""
    c = G.mx_wide_down_case(M, 256, 1024, 136)
    G.assert_exact(c, emulate(c)[0])
    x, w = c.xq * c.xsc, c.wq
    prod = x.reshape(M, 1, -1, 32) * w.reshape(1, 136, -1, 32)
    keep = prod.abs() * G.FP8_MFMA_SPAN >= prod.abs().amax(-1, keepdim=True)
    lossy = (prod * keep).sum((-1, -2)) * c.ws[None, :]
    assert not torch.equal(lossy, c.z)
    G.assert_exact(c, G.round_bf16(lossy), "products below the window dropped")
    for mut in ("mx_block_shift", "w_scale_shift", "drop_k", "double_k"):
        out = emulate(c, mut)[0]
        assert float(G.mismatch(c, out).double().mean()) > (0.2 if "shift" in mut else 0.0), mut
        assert bool(G.mismatch(c, out).any()), mut


def test_assert_exact_compares_values_and_reports_the_pattern():
    c = G.integer_case(37, 136, 336, "bf16")
    out = c.expected.clone()
    zero = (out == 0).nonzero()
    assert zero.numel(), "the case has no zero output"
    out[tuple(zero[0])] = -0.0
    G.assert_exact(c, out)  # -0 == 0
    out[5, 7] = float("nan")
    with pytest.raises(AssertionError, match=r"1 of 5032 elements wrong, first at \(m=5, n=7\)"):
        G.assert_exact(c, out)
    out = c.expected.clone()
    out[32:, 128:] = 7777.0
    with pytest.raises(AssertionError, match=r"rows \[32, 33, 34, 35, 36\], columns \[128, 129, 130, 131, 132, 133, 134, 135\]"):
        G.assert_exact(c, out)


def test_rounding_helpers_against_torch():
    v = torch.randn(4096, dtype=torch.float64, generator=torch.Generator().manual_seed(0)).float().double() * 300
    assert torch.equal(G.round_bf16(v), v.float().to(torch.bfloat16))
    ties = torch.tensor([257.0, 259.0, -257.0, -259.0, 514.0, 518.0])
    assert G.round_bf16(ties).tolist() == [256.0, 260.0, -256.0, -260.0, 512.0, 520.0]
    assert G.round_bf16(ties, "away").tolist() == [258.0, 260.0, -258.0, -260.0, 516.0, 520.0]
    assert G.round_bf16(ties + 0.5, "trunc").tolist() == [256.0, 258.0, -256.0, -258.0, 512.0, 516.0]
    assert G.bf16_down(ties).tolist() == [256.0, 258.0, -258.0, -260.0, 512.0, 516.0]
    assert G.bf16_up(ties).tolist() == [258.0, 260.0, -256.0, -258.0, 516.0, 520.0]


# ------------------------------------------------------------------------------------ mutants
@pytest.mark.parametrize("flavour,shape", flavour_shapes())
@pytest.mark.parametrize("mut", ["trunc", "away", "bf16_slabs", "bf16_acc", "bias_after_round", "bias_shift", "drop_k",
                                 "double_k"])
def test_integer_cases_catch(mut, flavour, shape):
    must_fail(G.integer_case(*shape, flavour), mut, may_miss=mut in ("bf16_slabs", "bf16_acc") and shape[2] < 704)
    if mut in ("trunc", "away", "bias_shift"):
        must_fail(G.integer_case(*shape, flavour, act="relu"), mut)
        must_fail(G.saturated_gelu_case(*shape, flavour, "gelu"), mut)
        must_fail(G.swiglu_case(shape[0], 160, shape[2], flavour), mut)


@pytest.mark.parametrize("flavour", G.FLAVOURS[:3])
def test_partial_last_k_step_dropped_in_one_column(flavour):
    must_fail(G.integer_case(37, 136, 336, flavour), "drop_tail_col")
    must_fail(G.probe_case(37, 136, 336, flavour), "drop_tail_col", exact_set=True)
    must_fail(G.probe_case(37, 136, 336, flavour, mirror=True), "drop_tail_col", exact_set=flavour != "w8a8")


@pytest.mark.parametrize("flavour,shape", flavour_shapes())
@pytest.mark.parametrize("mirror", [False, True])
@pytest.mark.parametrize("mut", ["drop_k", "double_k"])
def test_probes_catch_one_k_on_exactly_its_row(mut, mirror, flavour, shape):
    must_fail(G.probe_case(*shape, flavour, mirror=mirror), mut, exact_set=not (mirror and flavour == "w8a8"))


@pytest.mark.parametrize("flavour,shape", flavour_shapes())
def test_probe_with_bias_catches_a_shifted_bias(flavour, shape):
    must_fail(G.probe_case(*shape, flavour, bias=True), "bias_shift")


@pytest.mark.parametrize("flavour,shape", flavour_shapes(FP8))
def test_scale_from_the_neighbouring_row(flavour, shape):
    for c in (G.integer_case(*shape, flavour), G.saturated_gelu_case(*shape, flavour, "gelu_tanh"),
              G.swiglu_case(shape[0], 160, shape[2], flavour)):
        must_fail(c, "w_scale_shift")
    must_fail(G.probe_case(*shape, flavour), "w_scale_shift", exact_set=True)
    if flavour == "w8a8":
        must_fail(G.integer_case(*shape, flavour), "x_scale_shift")
        must_fail(G.probe_case(*shape, flavour), "x_scale_shift", exact_set=True)
    if flavour == "mx":
        must_fail(G.integer_case(*shape, flavour), "mx_block_shift")
        must_fail(G.probe_case(*shape, flavour, mirror=True), "mx_block_shift", exact_set=True)


@pytest.mark.parametrize("flavour,shape", flavour_shapes())
@pytest.mark.parametrize("mut", ["glu_swapped", "glu_next_pair"])
def test_swiglu_pairing(mut, flavour, shape):
    must_fail(G.swiglu_case(shape[0], 160, shape[2], flavour), mut)


@pytest.mark.parametrize("flavour,shape", flavour_shapes())
def test_midrange_bracket(flavour, shape):
    """The float32 emulation of csrc/common.h passes the bracket; the other GELU does not."""
    M, _, K = shape
    for act, N in (("gelu_tanh", 136), ("gelu", 136), ("silu", 160)):
        c = G.midrange_case(M, N, K, flavour, act)
        zz = R.glu_split(c.z, -1)[0] if c.glu else c.z
        with np.errstate(over="ignore"):
            out32 = torch.from_numpy(G.act32(zz.numpy(), act)).to(torch.bfloat16)
        G.assert_exact(c, out32, "float32 emulation")
        G.assert_exact(c, emulate(c)[0], "fp64")
        assert 0 < c.A <= 4 * G.midrange_a0(act)
        if act != "silu":
            must_fail(c, "erf_for_tanh" if act == "gelu_tanh" else "tanh_for_erf")


def test_recorded_a0():
    """The A0 values the gemm_cases docstring records."""
    for act, a0 in (("gelu_tanh", 3.19e-07), ("gelu", 3.83e-07), ("silu", 5.81e-07)):
        assert G.midrange_a0(act) == pytest.approx(a0, rel=0.02), act


# ------------------------------------------------------------------------------------ today's toleranced check
def _close_bad(a, b, atol, rtol=0.02):
    """tests/test_kernels_gpu.py close(): |err| <= atol + rtol |ref| (the formula only)."""
    a, b = a.float(), b.float()
    return int((~((a - b).abs() <= atol + rtol * b.abs())).sum())


def test_the_toleranced_check_lets_these_mutants_through():
    """Gaussian operands at (37, 256, 336), as test_gemm_tiled_variants draws them: truncation, round-half-away, bf16
    slabs, a bf16 accumulator per k-step and erf-for-tanh GELU all pass close(got, ref, 2e-2), and every one of them
    fails the exact cases above."""
    M, N, K = 37, 256, 336
    g = torch.Generator().manual_seed(0)
    x = torch.randn(M, K, generator=g).to(torch.bfloat16).double()
    w = (torch.randn(N, K, generator=g) * K ** -0.5).to(torch.bfloat16).double()
    b = (torch.randn(N, generator=g) * 0.1).to(torch.bfloat16).double()
    c = G.Case("gaussian", "bf16", "none", False, x, torch.ones_like(x), w, torch.ones(N, dtype=torch.float64), b, None,
               None, None, None, None, None, None, 1.0)
    c.z = G.pre_activation(c)
    ref = emulate(c)[0]
    for mut in ("trunc", "away", "bf16_slabs", "bf16_acc"):
        out = emulate(c, mut)[0]
        assert mut == "away" or not torch.equal(out, ref), mut  # Gaussian sums hold no exact tie
        assert _close_bad(out, ref, 2e-2) == 0, mut
    t, e = G.round_bf16(G.act64(c.z, "gelu_tanh")), G.round_bf16(G.act64(c.z, "gelu"))
    assert not torch.equal(t, e) and _close_bad(e, t, 2e-2) == 0


# ------------------------------------------------------------------------------------ RoPE / KV write
@pytest.mark.parametrize("style,D,rot,nh,nkv", [("gptj", 64, 32, 4, 2), ("neox", 64, 32, 4, 1), ("neox", 128, 128, 4, 2)])
def test_rope_mutants(style, D, rot, nh, nkv):
    rc = G.rope_case(19, nh, nkv, D, rot, style)
    want = G.rope_expected(rc, rc.qkv)
    for t in want[1:]:
        assert bool(t.isnan().any()) and not bool(t.isnan().all())  # a skipped slot, untouched rows
    assert set(rc.cos.unique().tolist()) == {-1.0, 0.0, 1.0} and torch.equal(rc.cos.abs() + rc.sin.abs(),
                                                                              torch.ones_like(rc.cos))

    def differs(**mut):
        got = G.rope_expected(rc, rc.qkv, **mut)
        n = 0
        for a, b, name in zip(got, want, ("qkv", "k cache", "v cache")):
            try:
                G.assert_same_bits(a, b, name)
            except AssertionError:
                n += 1
        return n

    assert differs() == 0
    assert differs(style="neox" if style == "gptj" else "gptj") >= 2  # q and the k cache
    assert differs(sin=-rc.sin) >= 2
    assert differs(kv_swapped=True) == 2
    if rot + 2 <= D:
        cos, sin = G.quarter_turn_tables(64, rot + 2)
        assert torch.equal(cos[:, : rot // 2], rc.cos)
        assert differs(rot=rot + 2, cos=cos, sin=sin) >= 2
