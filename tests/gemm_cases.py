"""GEMM inputs whose correct bf16 output is known to the bit (tests/test_gemm_cases_cpu.py proves that the checks
fail on every kernel mistake they are meant to catch; tests/test_gemm_exact_gpu.py runs them against the HIP kernels).

integer    x, w and bias are integers times a power of two, and sum_k |x||w| + |bias| stays below 2^24 units of the
           smallest term: every product and every partial sum is exact in fp32, in any order, under any K split, on
           the bf16 and on the fp8 MFMA. The only rounding left is the final round-to-nearest-even to bf16, so the
           output must equal the oracle with tolerance 0. Flavours: bf16 x bf16, W8A16 (e4m3 weight bytes, per-row
           power-of-two scales), W8A8 per token (activations the quantiser reproduces exactly), MX (e8m0 block scales).
probe      x one-hot (row m holds one non-zero at k = sigma(m)), w arbitrary: the output is w[:, sigma(m)] (times a
           power-of-two scale, plus the bias). The mirror makes w one-hot at k = tau(n). probe_ks(K) lists 0, K - 1,
           every element of a partial last 64-element k-step, and the first and last element of every 16-element
           k-group (which are also the ends of every 32-group and 64-step); one case reaches M (or N) of them, and
           probe_cases() steps an offset until every one has been visited (asserted), on the x and on the w side.
saturated  epilogues that are exact without knowing the kernel's formula: ReLU; GELU (tanh and erf) with every
           |z| >= 32, where the result is z or 0; SwiGLU with gate >= 37, where silu(g) == g even in fp64, so the
           output is RNE_bf16(g * u).
midrange   the only toleranced cases: pre-activations on the grid 2^-4 in [-8, 8]; the output must lie in
           [bf16_down(ref64 - A), bf16_up(ref64 + A)] with A = 4 * A0, A0 = max |act32(z) - act64(z)| over the grid,
           act32 = csrc/common.h's formula evaluated in numpy float32 in the same operation order (the factor 4: the
           device's fast exp is good to a couple of ulps, numpy's is correctly rounded). Recorded A0 over the whole
           grid (midrange_a0; test_gemm_cases_cpu.py asserts them): gelu_tanh 3.19e-07, gelu (erf) 3.83e-07,
           silu 5.81e-07. A case uses the A0 of its own z values, which is no larger.
rope       cos / sin tables with entries in {0, +-1} (quarter turns that vary with position and frequency index):
           the rotation is a signed permutation, exact in any arithmetic.

Everything here is a seeded CPU tensor; nothing imports the GPU.
"""
import functools
from dataclasses import dataclass
from typing import Optional

import numpy as np
import torch
import torch.nn.functional as F

from llmss_amd.ops import reference as R

LIMIT = float(1 << 24)
FLAVOURS = ("bf16", "w8a16", "w8a8", "mx")
ANCHOR_COL = 3  # w8a8 cases whose anchor sits in one column for every row
# The fp8 MFMA does not add the 32 products of one block-scaled group in full fp32. Measured on an MI355X through the
# gemm_mid MX kernel (+B and -B cancelling at k = 0, 1, one small value v elsewhere, weights 1, B in {8, 256, 448},
# block scales 2^0 .. 2^12): with v in B's 32-element block the result is v exactly for B / v = 2^3 .. 2^12 and 0
# for B / v = 2^14 .. 2^17.8, whatever the block scale; with v in another block it is exact up to B / v = 2^29.8. So a
# product more than 2^12 below the largest product of its 32-block may be dropped, and blocks add up in fp32. The
# cases that run on the fp8 MFMA (w8a8, mx) keep |largest product| / |lowest set bit of any product| of a whole row
# at or below 2^12, the widest span measured exact; the builders assert it. mx_wide_down_case derives its allowance
# from the same figure.
FP8_MFMA_SPAN = 4096.0


# ------------------------------------------------------------------------------------ bf16 grid
def _ord(b: torch.Tensor) -> torch.Tensor:
    """bf16 -> int32 key that is monotone in the value (-0 and +0 share key 0)."""
    i = b.view(torch.int16).to(torch.int32)
    return torch.where(i >= 0, i, -(i & 0x7FFF))


def _unord(k: torch.Tensor) -> torch.Tensor:
    i = torch.where(k >= 0, k, (-k) | 0x8000)
    return ((i + 0x8000) % 0x10000 - 0x8000).to(torch.int16).view(torch.bfloat16)


def bf16_down(v: torch.Tensor) -> torch.Tensor:
    """Largest bf16 <= v (v fp64)."""
    k = _ord(v.float().to(torch.bfloat16))
    k = torch.where(_unord(k).double() > v, k - 1, k)
    k = torch.where(_unord(k + 1).double() <= v, k + 1, k)
    return _unord(k)


def bf16_up(v: torch.Tensor) -> torch.Tensor:
    """Smallest bf16 >= v (v fp64)."""
    return _unord(-_ord(bf16_down(-v)))


def round_bf16(v: torch.Tensor, mode: str = "rne") -> torch.Tensor:
    """fp64 -> bf16 with ONE rounding: rne (what the kernels do), trunc (toward zero), away (ties away from zero)."""
    d, u = bf16_down(v), bf16_up(v)
    if mode == "trunc":
        return torch.where(v >= 0, d, u)
    lo, hi = v - d.double(), u.double() - v
    tie = (lo == hi) & (_ord(d) != _ord(u))
    if mode == "away":
        pick_up = torch.where(tie, v > 0, hi < lo)
    else:
        pick_up = torch.where(tie, (_ord(u) & 1) == 0, hi < lo)
    return torch.where(pick_up, u, d)


def lowest_set_bit(v: torch.Tensor) -> torch.Tensor:
    """The largest power of two that divides each element (dyadic fp64 values; inf for 0)."""
    out = torch.full_like(v, float("inf"))
    for b in range(-40, 41):
        out = torch.where((v != 0) & ((v / 2.0 ** b) == (v / 2.0 ** b).round()), torch.full_like(v, 2.0 ** b), out)
    return out


def e4m3_bytes(v: torch.Tensor) -> torch.Tensor:
    """Values that e4m3 holds exactly -> their bytes."""
    q = v.float().to(torch.float8_e4m3fn)
    assert torch.equal(q.float().double(), v.double()), "not exact in e4m3"
    return q.view(torch.uint8)


def act64(z: torch.Tensor, act: str) -> torch.Tensor:
    return R._act(z, act)


# ------------------------------------------------------------------------------------ the case
@dataclass
class Case:
    what: str
    flavour: str
    act: str
    glu: bool
    # exact fp64 factors: z = (xq * xsc) @ (wq * ws[:, None])^T + bias64
    xq: torch.Tensor            # [M, K]
    xsc: torch.Tensor           # [M, K] activation scale of every element (ones for bf16 activations)
    wq: torch.Tensor            # [N, K]
    ws: torch.Tensor            # [N]
    bias64: Optional[torch.Tensor]
    # what the kernel is given
    x: Optional[torch.Tensor]   # bf16 [M, K]; None for MX activations
    mx: Optional[tuple]         # (q uint8 [M, K], s uint8 [M, K / 32])
    w: torch.Tensor             # bf16 [N, K] or e4m3 bytes
    w_scale: Optional[torch.Tensor]
    bias: Optional[torch.Tensor]
    z: torch.Tensor             # [M, N] fp64 pre-activation, exact
    expected: torch.Tensor      # bf16 [M, nout]
    unit: float                 # the case's grid (smallest term), for messages
    ref64: Optional[torch.Tensor] = None  # midrange: the fp64 activation and its allowance A
    A: float = 0.0

    @property
    def shape(self):
        return (self.xq.shape[0], self.wq.shape[0], self.xq.shape[1])

    @property
    def nout(self):
        return self.expected.shape[1]


def pre_activation(c: Case, xq=None, xsc=None, wq=None, ws=None, bias="same") -> torch.Tensor:
    """z of the case, or of the case with some factors replaced (the CPU mutants)."""
    xq = c.xq if xq is None else xq
    xsc = c.xsc if xsc is None else xsc
    wq = c.wq if wq is None else wq
    ws = c.ws if ws is None else ws
    b = c.bias64 if isinstance(bias, str) else bias
    z = (xq * xsc) @ (wq * ws[:, None]).t()
    return z if b is None else z + b


def epilogue64(z: torch.Tensor, act: str, glu: bool) -> torch.Tensor:
    if glu:
        g, u = R.glu_split(z, -1)
        return F.silu(g) * u
    return act64(z, act)


def finish(c: Case, z: torch.Tensor, mode: str = "rne") -> torch.Tensor:
    """The honest oracle's last step: fp64 epilogue, one rounding."""
    return round_bf16(epilogue64(z, c.act, c.glu), mode)


def mismatch(c: Case, out: torch.Tensor) -> torch.Tensor:
    """[M, nout] bool: elements of ``out`` the case rejects. Values are compared, so -0 == 0; NaN never passes."""
    got = out.detach().cpu()
    assert tuple(got.shape) == tuple(c.expected.shape), (c.what, tuple(got.shape), tuple(c.expected.shape))
    g = got.double()
    if c.ref64 is None:
        return ~(g == c.expected.double())
    lo, hi = bf16_down(c.ref64 - c.A).double(), bf16_up(c.ref64 + c.A).double()
    return ~((g >= lo) & (g <= hi))


def assert_exact(c: Case, out: torch.Tensor, what: str = "") -> None:
    bad = mismatch(c, out)
    if not bool(bad.any()):
        return
    idx = bad.nonzero()
    g = out.detach().cpu().double()
    ref = c.expected.double() if c.ref64 is None else c.ref64
    diff = (g - ref).abs().nan_to_num(float("inf"))[bad].max().item() / c.unit
    m0, n0 = idx[0].tolist()
    raise AssertionError(
        f"{what} {c.what} {c.shape}: {int(bad.sum())} of {bad.numel()} elements wrong, first at (m={m0}, n={n0}): got "
        f"{g[m0, n0].item()!r}, want {ref[m0, n0].item()!r}; rows {idx[:, 0].unique().tolist()[:16]}, columns "
        f"{idx[:, 1].unique().tolist()[:16]}; largest difference {diff:.4g} units of {c.unit:g}")


# ------------------------------------------------------------------------------------ operand builders
def _w_scale(N: int) -> torch.Tensor:
    return torch.ldexp(torch.ones(N, dtype=torch.float64), torch.arange(N) % 5 - 2)  # neighbours differ by >= 2x


def _bias_pattern(N: int) -> torch.Tensor:
    return (torch.arange(N) % 17 - 8).double()  # period coprime to 8, 16, 32: a shifted read changes the result


def _row_exp(M: int) -> torch.Tensor:
    return torch.arange(M) % 3 - 1


def _mx_exp(M: int, K: int) -> torch.Tensor:
    return (torch.arange(M)[:, None] + 3 * torch.arange(K // 32)[None, :]) % 5 - 2  # range 4 along every row


def _activations(flavour: str, xi: torch.Tensor, anchor: bool = True, fixed_anchor: bool = False):
    """Integer activations ``xi`` [M, K] (|xi| <= 8 for the fp8 flavours) -> (xq, xsc, x bf16 or None, mx or None).
    w8a8: row m is scaled by 2^e(m), and one anchor entry per row is +-448 * 2^e(m), so the per-token quantiser's
    scale amax / 448 is exactly 2^e(m) and every entry is exact in e4m3 (asserted with the CPU quantiser).
    ``fixed_anchor``: +448 in column ANCHOR_COL of every row (sign-definite cases), else the column and sign vary."""
    M, K = xi.shape
    if flavour in ("bf16", "w8a16"):
        x = xi.to(torch.bfloat16)
        assert torch.equal(x.double(), xi)
        return xi, torch.ones_like(xi), x, None
    assert float(xi.abs().max()) <= 8
    if flavour == "w8a8":
        xq = xi.clone()
        if anchor:
            rows = torch.arange(M)
            if fixed_anchor:
                xq[:, ANCHOR_COL] = 448.0
            else:
                xq[rows, (7 * rows + 3) % K] = torch.where(rows % 2 == 0, 448.0, -448.0).double()
        xsc = torch.ldexp(torch.ones(M, dtype=torch.float64), _row_exp(M))[:, None].expand(M, K).contiguous()
        x = (xq * xsc).to(torch.bfloat16)
        assert torch.equal(x.double(), xq * xsc)
        q, s = R.quant_fp8_rows(x)
        assert torch.equal(s.double(), xsc[:, 0]), "per-token scale is not the intended power of two"
        assert torch.equal(R.dequant_fp8(q, s).double(), x.double()), "activations are not exact in e4m3"
        return xq, xsc, x, None
    assert flavour == "mx" and K % 32 == 0
    e = _mx_exp(M, K)
    assert int(e.max() - e.min()) >= 4
    xsc = torch.ldexp(torch.ones(M, K // 32, dtype=torch.float64), e).repeat_interleave(32, 1)
    mx = (e4m3_bytes(xi), (e + 127).to(torch.uint8))
    assert torch.equal(R.dequant_mx_fp8(*mx).double(), xi * xsc)
    return xi, xsc, None, mx


def _weights(flavour: str, wi: torch.Tensor, scaled: bool = True):
    N = wi.shape[0]
    if flavour == "bf16":
        w = wi.to(torch.bfloat16)
        assert torch.equal(w.double(), wi)
        return wi, torch.ones(N, dtype=torch.float64), w, None
    ws = _w_scale(N) if scaled else torch.ones(N, dtype=torch.float64)
    return wi, ws, e4m3_bytes(wi), ws.float()


def _make(what, flavour, act, glu, xi, wi, bias64, fixed_anchor=False) -> Case:
    xq, xsc, x, mx = _activations(flavour, xi, True, fixed_anchor)
    wq, ws, w, w_scale = _weights(flavour, wi)
    bias = None
    if bias64 is not None:
        bias = bias64.to(torch.bfloat16)
        assert torch.equal(bias.double(), bias64)
    c = Case(what, flavour, act, glu, xq, xsc, wq, ws, bias64, x, mx, w, w_scale, bias, None, None, 1.0)
    c.z = pre_activation(c)
    return c


def _units(c: Case) -> torch.Tensor:
    """[M, N] grid of every output: the smallest term's power of two. Integer operands: xq, wq and the bias are
    integers, the scales powers of two."""
    u = c.xsc.min(1).values[:, None] * c.ws[None, :]
    return u if c.bias64 is None else torch.minimum(u, torch.ones_like(u))


def _assert_exact_sums(c: Case) -> None:
    """sum_k |x||w| + |bias| below 2^24 units per output (the fp8 kernels scale after the sum: the unscaled sum too):
    otherwise the case proves nothing."""
    mag = pre_activation(c, xq=c.xq.abs(), wq=c.wq.abs(), bias=None if c.bias64 is None else c.bias64.abs())
    units = _units(c)
    assert float((mag / units).max()) < LIMIT, (c.what, float((mag / units).max()))
    assert float((c.xq.abs() @ c.wq.abs().t()).max()) < LIMIT
    assert torch.equal(c.z / units, (c.z / units).round())
    assert torch.equal(c.z.float().double(), c.z)
    if c.flavour in ("w8a8", "mx"):
        x = c.xq * c.xsc
        span = x.abs().max(1).values * c.wq.abs().max() / (lowest_set_bit(x).min(1).values * lowest_set_bit(c.wq).min())
        assert float(span[span == span].max()) <= FP8_MFMA_SPAN, (c.what, float(span.max()))
    c.unit = float(units.min())


def rounding_shares(v: torch.Tensor):
    """(share of values bf16 cannot hold, share that are exact ties: odd multiples of half a spacing)."""
    d, u = bf16_down(v).double(), bf16_up(v).double()
    inexact = d != u
    tie = inexact & ((v - d) == (u - v))
    return inexact.double().mean().item(), tie.double().mean().item()


# ------------------------------------------------------------------------------------ integer cases
@functools.lru_cache(maxsize=None)
def integer_case(M: int, N: int, K: int, flavour: str = "bf16", act: str = "none", bias: bool = True,
                 rounding: bool = True, seed: int = 0) -> Case:
    """Signed integer operands, act in (none, relu). ``rounding``: the case claims to test the final rounding, so at
    least 5 % of its outputs are not bf16 numbers and at least 1 % are exact ties; the builder picks the amplitude
    (+-4, +-8 or +-16 for bf16 operands) that gets there and asserts the shares."""
    assert act in ("none", "relu")
    amps = (4, 8, 16) if flavour in ("bf16", "w8a16") else (4, 8)
    b64 = _bias_pattern(N) if bias else None
    last = None
    for a, draw in [(a, d) for a in amps for d in range(4)]:  # a few draws per amplitude: a single short row is noisy
        g = torch.Generator().manual_seed(1000 * seed + 10 * a + draw)
        xi = torch.randint(-a, a + 1, (M, K), generator=g).double()
        wi = torch.randint(-min(a, 8), min(a, 8) + 1, (N, K), generator=g).double()
        c = _make(f"integer/{flavour}/{act}/+-{a}", flavour, act, False, xi, wi, b64)
        _assert_exact_sums(c)
        last = rounding_shares(epilogue64(c.z, act, False))  # shares of the OUTPUTS (after ReLU about half are 0)
        if not rounding or (last[0] >= 0.05 and last[1] >= 0.01):
            break
    else:
        raise AssertionError(f"integer case ({M}, {N}, {K}) {flavour}: inexact / tie shares {last} below 5 % / 1 %")
    c.expected = finish(c, c.z)
    assert torch.equal(c.expected, epilogue64(c.z, act, False).float().to(torch.bfloat16))  # z is exact in fp32
    return c


# ------------------------------------------------------------------------------------ saturated epilogues
@functools.lru_cache(maxsize=None)
def saturated_gelu_case(M: int, N: int, K: int, flavour: str = "bf16", act: str = "gelu_tanh", seed: int = 0) -> Case:
    """Every |z| >= 32: operands >= 1, the sign of weight row n and of its bias fixed per column, |bias| >= 32."""
    assert act in ("gelu_tanh", "gelu")
    a = 4 if K > 128 else 8
    g = torch.Generator().manual_seed(2000 + seed)
    sgn = torch.where(torch.arange(N) % 3 == 1, -1.0, 1.0).double()
    xi = torch.randint(1, a + 1, (M, K), generator=g).double()
    wi = torch.randint(1, a + 1, (N, K), generator=g).double() * sgn[:, None]
    b64 = sgn * (32 + torch.arange(N) % 17).double()
    c = _make(f"saturated/{flavour}/{act}", flavour, act, False, xi, wi, b64, fixed_anchor=True)
    _assert_exact_sums(c)
    assert float(c.z.abs().min()) >= 32
    c.expected = finish(c, c.z)
    want = round_bf16(torch.where(c.z > 0, c.z, torch.zeros_like(c.z)))
    assert torch.equal(c.expected.double(), want.double()), "GELU is not saturated"  # z or 0, whatever the formula
    assert (c.z < 0).any() and (c.z > 0).any()
    return c


@functools.lru_cache(maxsize=None)
def swiglu_case(M: int, N: int, K: int, flavour: str = "bf16", seed: int = 0) -> Case:
    """SwiGLU with a bias, exact: x >= 1 and gate weights >= 1, gate bias +32, so gate >= 37 and silu(g) == g in fp32
    and in fp64; up weights and up bias signed; g * u is exact in fp32, so the output is RNE_bf16(g * u)."""
    assert N % 32 == 0
    g = torch.Generator().manual_seed(3000 + seed)
    gate_col = (torch.arange(N) % 32) < 16
    b64 = torch.where(gate_col, torch.full((N,), 32.0, dtype=torch.float64), _bias_pattern(N))
    for a in (8, 4, 2, 1):
        xi = torch.randint(1, min(a, 2) + 1, (M, K), generator=g).double()
        wi = torch.where(gate_col[:, None], torch.randint(1, min(a, 2) + 1, (N, K), generator=g),
                         torch.randint(-a, a + 1, (N, K), generator=g)).double()
        if flavour == "w8a8":  # the anchor meets a zero up weight: it enlarges the gate only
            wi[~gate_col, ANCHOR_COL] = 0
        c = _make(f"saturated/{flavour}/swiglu+bias/+-{a}", flavour, "none", True, xi, wi, b64, fixed_anchor=True)
        gt, up = R.glu_split(c.z, -1)
        if torch.equal((gt * up).float().double(), gt * up) and float((gt * up).abs().max()) < LIMIT * c.ws.max():
            break
    else:
        raise AssertionError("no amplitude keeps g * u exact in fp32")
    _assert_exact_sums(c)
    assert float(gt.min()) >= 37
    assert torch.equal(F.silu(gt), gt) and torch.equal(F.silu(gt.float()), gt.float()), "silu(g) != g"
    c.expected = finish(c, c.z)
    assert torch.equal(c.expected, (gt * up).float().to(torch.bfloat16))
    assert rounding_shares(gt * up)[0] >= 0.05
    return c


# ------------------------------------------------------------------------------------ probes
def probe_ks(K: int) -> list:
    """0, K - 1, every element of a partial last 64-step, then the first and last element of every 16-group."""
    ks = [0, K - 1] + list(range(K - K % 64, K))
    for g0 in range(0, K, 16):
        ks += [g0, min(g0 + 15, K - 1)]
    return list(dict.fromkeys(ks))


def _gaussian_bf16(shape, g) -> torch.Tensor:
    """Gaussian bf16 values with |w| >= 2^-8 (never zero; w + bias stays exact in fp32)."""
    w = torch.randn(shape, generator=g).to(torch.bfloat16).double()
    return torch.where(w.abs() < 2.0 ** -8, torch.where(w < 0, -(2.0 ** -8), 2.0 ** -8), w)


def _gaussian_e4m3(shape, g) -> torch.Tensor:
    w = (torch.randn(shape, generator=g) * 4).clamp(-448, 448).to(torch.float8_e4m3fn).double()
    return torch.where(w.abs() < 2.0 ** -6, torch.where(w < 0, -(2.0 ** -6), 2.0 ** -6), w)


@functools.lru_cache(maxsize=None)
def probe_case(M: int, N: int, K: int, flavour: str = "bf16", mirror: bool = False, bias: bool = False,
               seed: int = 0, offset: int = 0) -> Case:
    """x one-hot at sigma(m) = probe_ks[(m + offset) % len] (w8a8: the one entry is +-448 * 2^e(m), its own anchor;
    mx: 1 under the block scale), w arbitrary; ``mirror``: w one-hot at tau(n) = probe_ks[(n + offset) % len], x
    arbitrary on the flavour's grid. One case reaches M (N) positions: probe_cases() steps the offset until every
    position of probe_ks(K) has been visited."""
    g = torch.Generator().manual_seed(4000 + seed)
    ks = torch.tensor(probe_ks(K))
    b64 = _bias_pattern(N) / 4 if bias else None
    if not mirror:
        sig = ks[(torch.arange(M) + offset) % len(ks)]
        xi = torch.zeros(M, K, dtype=torch.float64)
        one = torch.where(torch.arange(M) % 2 == 0, 448.0, -448.0).double() if flavour == "w8a8" else torch.ones(M).double()
        xi[torch.arange(M), sig] = one
        wi = _gaussian_bf16((N, K), g) if flavour == "bf16" else _gaussian_e4m3((N, K), g)
        xq, xsc, x, mx = (_activations(flavour, xi, anchor=False) if flavour != "w8a8" else _w8a8_raw(xi))
    else:
        tau = ks[(torch.arange(N) + offset) % len(ks)]
        wi = torch.zeros(N, K, dtype=torch.float64)
        wi[torch.arange(N), tau] = 1.0
        if flavour in ("bf16", "w8a16"):
            xi = _gaussian_bf16((M, K), g)
            xq, xsc, x, mx = xi, torch.ones_like(xi), xi.to(torch.bfloat16), None
        elif flavour == "w8a8":
            xq, xsc, x, mx = _activations(flavour, torch.randint(-8, 9, (M, K), generator=g).double())
        else:
            xi = _gaussian_e4m3((M, K), g)
            e = _mx_exp(M, K)
            xq, xsc = xi, torch.ldexp(torch.ones(M, K // 32, dtype=torch.float64), e).repeat_interleave(32, 1)
            x, mx = None, (e4m3_bytes(xi), (e + 127).to(torch.uint8))
    wq, ws, w, w_scale = _weights(flavour, wi)
    c = Case(f"probe/{flavour}/{'w' if mirror else 'x'} one-hot{'/bias' if bias else ''}", flavour, "none", False, xq,
             xsc, wq, ws, b64, x, mx, w, w_scale, None if b64 is None else b64.to(torch.bfloat16), None, None, 2.0 ** -16)
    c.z = pre_activation(c)
    assert torch.equal(c.z.float().double(), c.z), "probe sums are not exact in fp32"
    assert float((c.xq.abs() @ c.wq.abs().t()).max()) < LIMIT
    c.expected = finish(c, c.z)
    if not bias:
        assert torch.equal(c.expected.double(), c.z), "a probe output is not a bf16 number"
    return c


def probe_cases(M: int, N: int, K: int, flavour: str, mirror: bool) -> list:
    """Offset probe cases that together put a one-hot at every position of probe_ks(K) (asserted): ceil(len / M) x
    probes, ceil(len / N) w probes."""
    n = len(probe_ks(K))
    rows = N if mirror else M
    cs = [probe_case(M, N, K, flavour, mirror=mirror, offset=o) for o in range(0, n, rows)]
    hot = torch.zeros(K, dtype=torch.bool)
    for c in cs:
        hot |= ((c.wq if mirror else c.xq) != 0).any(0)
    want = torch.zeros(K, dtype=torch.bool)
    want[torch.tensor(probe_ks(K))] = True
    assert torch.equal(hot, want), "the one-hot positions are not exactly probe_ks(K)"
    return cs


def _w8a8_raw(xi):
    """w8a8 one-hot rows: the entry +-448 is the row's amax, so the per-token scale is 2^e(m) exactly."""
    M, K = xi.shape
    xsc = torch.ldexp(torch.ones(M, dtype=torch.float64), _row_exp(M))[:, None].expand(M, K).contiguous()
    x = (xi * xsc).to(torch.bfloat16)
    q, s = R.quant_fp8_rows(x)
    assert torch.equal(s.double(), xsc[:, 0]) and torch.equal(R.dequant_fp8(q, s).double(), xi * xsc)
    return xi, xsc, x, None


# ------------------------------------------------------------------------------------ midrange activations
def _f32(v):
    return np.float32(v)


def act32(z: np.ndarray, act: str) -> np.ndarray:
    """csrc/common.h gelu_tanh / gelu_erf / silu in numpy float32, operation by operation."""
    x = z.astype(np.float32)
    if act == "gelu_tanh":
        u = _f32(0.7978845608028654) * (x + _f32(0.044715) * x * x * x)
        t = _f32(1) - _f32(2) / (np.exp(_f32(2) * u) + _f32(1))
        return _f32(0.5) * x * (_f32(1) + t)
    if act == "gelu":
        erf = torch.special.erf(torch.from_numpy(x * _f32(0.7071067811865476))).numpy()
        return _f32(0.5) * x * (_f32(1) + erf)
    assert act == "silu"
    return x / (_f32(1) + np.exp(-x))


def act64_mid(z: torch.Tensor, act: str) -> torch.Tensor:
    return F.silu(z) if act == "silu" else act64(z, act)


def midrange_a0(act: str, z: Optional[torch.Tensor] = None) -> float:
    """max |act32(z) - act64(z)| over z (default: the whole grid 2^-4 in [-8, 8])."""
    z = torch.arange(-128, 129).double() / 16 if z is None else z.double().reshape(-1)
    with np.errstate(over="ignore"):
        a32 = torch.from_numpy(act32(z.numpy(), act).astype(np.float64))
    return float((a32 - act64_mid(z, act)).abs().max())


@functools.lru_cache(maxsize=None)
def midrange_case(M: int, N: int, K: int, flavour: str = "bf16", act: str = "gelu_tanh", seed: int = 0) -> Case:
    """z on the grid 2^-4 in [-8, 8]: 8 non-zero activations of magnitude <= 2 per row, integer weights in +-8, the
    2^-4 in the activations (bf16 / w8a16: the values; w8a8: the per-token scale; mx: the block scale) and weight
    scales of 1. act = silu: SwiGLU whose up half is exactly 1 (up weights 0, up bias 1), so the output is silu(g)."""
    g = torch.Generator().manual_seed(5000 + seed)
    glu = act == "silu"
    xi = torch.zeros(M, K, dtype=torch.float64)
    for m in range(M):
        cols = torch.randperm(K, generator=g)[:8]
        xi[m, cols] = (torch.randint(1, 3, (8,), generator=g) * (2 * torch.randint(0, 2, (8,), generator=g) - 1)).double()
    wi = torch.randint(-8, 9, (N, K), generator=g).double()
    b64 = None
    if glu:
        up_col = (torch.arange(N) % 32) >= 16
        wi[up_col] = 0
        b64 = up_col.double()
    if flavour in ("bf16", "w8a16"):
        xq, xsc = xi / 16, torch.ones_like(xi)
        x, mx = xq.to(torch.bfloat16), None
    elif flavour == "w8a8":  # the anchor +-448 / 16 meets a zero weight column
        xi[:, ANCHOR_COL] = 448.0
        wi[:, ANCHOR_COL] = 0
        xq, xsc = xi, torch.full_like(xi, 1 / 16)
        x, mx = (xq * xsc).to(torch.bfloat16), None
        q, s = R.quant_fp8_rows(x)
        assert torch.equal(s.double(), xsc[:, 0]) and torch.equal(R.dequant_fp8(q, s).double(), xq * xsc)
    else:
        xq, xsc = xi, torch.full_like(xi, 1 / 16)
        x, mx = None, (e4m3_bytes(xi), torch.full((M, K // 32), 127 - 4, dtype=torch.uint8))
    if flavour == "bf16":
        w, w_scale = wi.to(torch.bfloat16), None
    else:
        w, w_scale = e4m3_bytes(wi), torch.ones(N)
    c = Case(f"midrange/{flavour}/{act}", flavour, "none" if glu else act, glu, xq, xsc, wi,
             torch.ones(N, dtype=torch.float64), b64, x, mx, w, w_scale,
             None if b64 is None else b64.to(torch.bfloat16), None, None, 2.0 ** -4)
    c.z = pre_activation(c)
    zz = R.glu_split(c.z, -1)[0] if glu else c.z
    assert float(zz.abs().max()) <= 8 and torch.equal(zz * 16, (zz * 16).round())
    span = 2 if zz.numel() >= 256 else 1  # a single short row covers less of the grid
    assert float(zz.min()) <= -span and float(zz.max()) >= span and zz.unique().numel() >= min(32, zz.numel() // 3)
    if glu:
        assert torch.equal(R.glu_split(c.z, -1)[1], torch.ones_like(zz))
    c.ref64 = act64_mid(zz, act)
    c.A = 4 * midrange_a0(act, zz)
    c.expected = round_bf16(c.ref64)
    return c


# ------------------------------------------------------------------------------------ RoPE / KV write
@dataclass
class RopeCase:
    what: str
    qkv: torch.Tensor     # bf16 [T, (nh + 2 nkv) D], integers
    positions: torch.Tensor
    cos: torch.Tensor
    sin: torch.Tensor
    slots: torch.Tensor   # one skipped (-1)
    nh: int
    nkv: int
    D: int
    rot: int
    style: str
    bs: int
    nb: int


def quarter_turn_tables(max_pos: int, rot: int):
    """cos / sin of (p + 3 j) quarter turns: entries in {0, +-1}, varying with position p and frequency index j."""
    q = (torch.arange(max_pos)[:, None] + 3 * torch.arange(rot // 2)[None, :]) % 4
    cos = torch.tensor([1.0, 0.0, -1.0, 0.0])[q]
    sin = torch.tensor([0.0, 1.0, 0.0, -1.0])[q]
    return cos.contiguous(), sin.contiguous()


@functools.lru_cache(maxsize=None)
def rope_case(T: int, nh: int, nkv: int, D: int, rot: int, style: str, seed: int = 0) -> RopeCase:
    g = torch.Generator().manual_seed(6000 + seed)
    bs, nb = 16, (T + 15) // 16 + 3
    qkv = torch.randint(-100, 101, (T, (nh + 2 * nkv) * D), generator=g).to(torch.bfloat16)
    pos = torch.randint(0, 64, (T,), generator=g)
    cos, sin = quarter_turn_tables(64, max(rot, 2))
    slots = torch.randperm(nb * bs, generator=g)[:T]
    if T > 1:
        slots[min(3, T - 1)] = -1
    return RopeCase(f"rope/{style}/D{D}/rot{rot}", qkv, pos, cos, sin, slots, nh, nkv, D, rot, style, bs, nb)


def rope_expected(rc: RopeCase, qkv: torch.Tensor, do_rope: bool = True, **mut):
    """(qkv, k_cache, v_cache) after R.rope_cache on NaN caches; ``mut`` swaps in a wrong style / sin / rot / slot."""
    q = qkv.clone()
    kc = torch.full((rc.nb, rc.nkv, rc.bs, rc.D), float("nan"), dtype=torch.bfloat16)
    vc = torch.full_like(kc, float("nan"))
    a = dict(style=rc.style, cos=rc.cos, sin=rc.sin, rot=rc.rot)
    a.update({k: v for k, v in mut.items() if k in a})
    if mut.get("kv_swapped"):
        kc, vc = vc, kc
    R.rope_cache(q, rc.positions, a["cos"], a["sin"], kc, vc, rc.slots, rc.nh, rc.nkv, rc.D, a["rot"], a["style"],
                 do_rope=do_rope)
    if mut.get("kv_swapped"):
        kc, vc = vc, kc
    return q, kc, vc


def assert_same_bits(got: torch.Tensor, want: torch.Tensor, what: str) -> None:
    """Bit equality up to the sign of zero, NaN only where NaN is wanted."""
    g, w = got.detach().cpu().double(), want.double()
    bad = ~((g == w) | (g.isnan() & w.isnan()))
    if bool(bad.any()):
        idx = bad.nonzero()
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.numel()} elements differ, first at {idx[0].tolist()}: "
                             f"got {g[tuple(idx[0])].item()!r}, want {w[tuple(idx[0])].item()!r}")


# ------------------------------------------------------------------------------------ MX output -> down projection
@functools.lru_cache(maxsize=None)
def mx_swiglu_case(M: int, F2: int, K: int, seed: int = 0) -> Case:
    """A saturated SwiGLU + bias case (w8a8) whose output MX-fp8 holds without loss, with a different e8m0 scale in
    each of a row's 32-output blocks: gate = its bias, 32 * 2^j with j = the block's index mod 4 (gate weights 0), up =
    2^e(m) * (+-2 * x[m, k(n)]) + bias, an integer of magnitude <= 16. The down projection fed with it then multiplies
    small integers times powers of two, as the integer cases do.

    The general swiglu_case is NOT fed to the down projection: its MX activations span 2^18 inside one 128-element
    MFMA, and v_mfma_scale_f32_16x16x128_f8f6f4 (csrc/gemm_mid.hip hands it the bytes and block scales untouched) is
    not exact there (FP8_MFMA_SPAN above): measured on an MI355X, 0.4-0.8 % of such outputs differ from the exact sum,
    by up to 18 % where large terms cancel, with every block scale set to 1 as well. This case stays within the span;
    mx_wide_down_case checks the general one within the allowance that the instruction's arithmetic needs."""
    assert F2 % 128 == 0 and K > 16
    g = torch.Generator().manual_seed(8000 + seed)
    n = torch.arange(F2)
    gate_col = (n % 32) < 16
    block = (n // 64) % 4
    b64 = torch.where(gate_col, 32.0 * 2.0 ** block.double(), _bias_pattern(F2))
    xi = torch.randint(0, 3, (M, K), generator=g).double()
    wi = torch.zeros(F2, K, dtype=torch.float64)
    up_rows = n[~gate_col]
    kcol = 4 + up_rows % 11
    wi[up_rows, kcol] = torch.where(up_rows % 3 == 0, -2.0, 2.0).double()
    xq, xsc, x, mx = _activations("w8a8", xi, True, fixed_anchor=True)
    assert ANCHOR_COL < 4
    ws = torch.ones(F2, dtype=torch.float64)
    c = Case("saturated/w8a8/swiglu+bias/MX-exact", "w8a8", "none", True, xq, xsc, wi, ws, b64, x, None, e4m3_bytes(wi),
             ws.float(), b64.to(torch.bfloat16), None, None, 1.0)
    c.z = pre_activation(c)
    _assert_exact_sums(c)
    gt, up = R.glu_split(c.z, -1)
    assert float(gt.min()) >= 32 and torch.equal(F.silu(gt.float()), gt.float()), "silu(g) != g in fp32"
    assert torch.equal(up, up.round()) and float(up.abs().max()) <= 16 and up.unique().numel() >= 16
    c.expected = round_bf16(gt * up)
    assert torch.equal(c.expected, finish(c, c.z)) and torch.equal(c.expected.double(), gt * up)
    q, s = R.quant_mx_fp8(c.expected.float())
    assert torch.equal(R.dequant_mx_fp8(q, s).double(), gt * up), "the MX output loses bits"
    spread = s.to(torch.int32).max(1).values - s.to(torch.int32).min(1).values
    assert int(spread.min()) >= 2 and int(spread.max()) >= 3, "block scales do not vary along the row"
    return c


@functools.lru_cache(maxsize=None)
def mx_down_case(M: int, F2: int, K: int, Nd: int, seed: int = 0) -> Case:
    """The down projection behind mx_swiglu_case(M, F2, K): activations R.quant_mx_fp8(that case's output), weights
    integers in +-2 with power-of-two row scales; the usual bound of 2^24 units per output."""
    up = mx_swiglu_case(M, F2, K, seed)
    q, s = R.quant_mx_fp8(up.expected.float())
    e = s.to(torch.int32) - 127
    xsc = torch.ldexp(torch.ones(e.shape, dtype=torch.float64), e).repeat_interleave(32, 1)
    xq = q.view(torch.float8_e4m3fn).double()
    assert torch.equal(xq, xq.round()) and float(xq.abs().max()) <= 448
    g = torch.Generator().manual_seed(7000 + seed)
    wi = torch.randint(-2, 3, (Nd, xq.shape[1]), generator=g).double()
    wq, ws, w, w_scale = _weights("mx", wi)
    c = Case("mx_out/down projection", "mx", "none", False, xq, xsc, wq, ws, None, None, (q, s), w, w_scale, None, None,
             None, 1.0)
    c.z = pre_activation(c)
    _assert_exact_sums(c)
    c.expected = finish(c, c.z)
    assert rounding_shares(c.z)[0] >= 0.05
    return c


@functools.lru_cache(maxsize=None)
def mx_wide_down_case(M: int, F2: int, K: int, Nd: int, seed: int = 0) -> Case:
    """The down projection on the MX output of the GENERAL swiglu_case (e4m3 values over their whole range), toleranced:
    a product more than 2^12 below the largest product of its 32-element block may be dropped by the fp8 MFMA
    (FP8_MFMA_SPAN), so output (m, n) may be off by sum over blocks of 32 * 2^-12 * max_k |x_mk w_nk|; the output must
    lie in [bf16_down(z - B), bf16_up(z + B)]. A scale from the neighbouring block or row moves outputs by far more."""
    up = swiglu_case(M, F2, K, "w8a8", seed)
    q, s = R.quant_mx_fp8(up.expected.float())
    e = s.to(torch.int32) - 127
    xsc = torch.ldexp(torch.ones(e.shape, dtype=torch.float64), e).repeat_interleave(32, 1)
    xq = q.view(torch.float8_e4m3fn).double()
    g = torch.Generator().manual_seed(7000 + seed)
    wi = torch.randint(-2, 3, (Nd, xq.shape[1]), generator=g).double()
    wq, ws, w, w_scale = _weights("mx", wi)
    c = Case("mx_out/down projection, wide span", "mx", "none", False, xq, xsc, wq, ws, None, None, (q, s), w, w_scale,
             None, None, None, 1.0)
    c.z = pre_activation(c)
    assert torch.equal(c.z.float().double(), c.z)
    xb, wb = (xq * xsc).abs().reshape(M, 1, -1, 32), wi.abs().reshape(1, Nd, -1, 32)
    c.A = (xb * wb).amax(-1).sum(-1) * ws[None, :] * 32 / FP8_MFMA_SPAN
    c.ref64 = c.z
    c.expected = round_bf16(c.z)
    assert float((c.A / c.z.abs().clamp_min(1e-300)).median()) < 0.25  # the allowance is small against most outputs
    return c


# ------------------------------------------------------------------------------------ the plans the GPU file runs
KS = (16, 64, 80, 112, 336, 704, 1024)  # 1, 1, 2 (partial), 2 (partial), 6 (partial), 11 and 16 64-element k-steps
MID_DIMS = {7: (64, 48), 8: (128, 128), 9: (256, 128), 10: (64, 256), 11: (64, 128), 12: (128, 256), 13: (64, 192),
            14: (64, 32), 15: (64, 96)}  # csrc/gemm_mid.hip mid_layout
TILE_DIMS = {1: (128, 128), 2: (64, 128), 3: (64, 64), 4: (256, 256), 5: (256, 128), 6: (256, 64)}
DEC_BN = {1: 16, 2: 32, 3: 48, 4: 64, 5: 96}  # csrc/gemm_dec.hip
ROWS = {64: (37, 65), 128: (129,), 256: (257,)}  # at / one above a row-tile boundary, and a ragged tile


@dataclass(frozen=True)
class Plan:
    family: str
    name: str
    flavour: str
    M: int
    N: int      # one full tile + 8 columns
    Ng: int     # one full tile + the next multiple of 32 columns (SwiGLU), 0: the plan has no SwiGLU epilogue
    K: int
    api: str    # "linear": nt_hint / split_hint; "w8a8": tile / depth / split / ilv of linear_w8a8
    kw: tuple

    @property
    def id(self):
        return f"{self.family}-{self.name}-{self.flavour}-{self.M}x{self.N}x{self.K}"


def _k(i: int, ks=KS) -> int:
    return ks[i % len(ks)]


def plans() -> list:
    P = []

    def add(family, name, flavour, M, bn, K, api="linear", glu=True, **kw):
        P.append(Plan(family, name, flavour, M, bn + 8, (bn + 63) // 32 * 32 if glu else 0, K, api, tuple(sorted(kw.items()))))

    # default-planned H.linear: bf16, and fp8 weights (W8A16 up to 128 rows, W8A8 above)
    for i, M in enumerate((1, 16, 17, 37, 64, 65, 129, 257)):
        add("default", "auto", "bf16", M, 128, _k(i + 2))
        add("default", "auto", "w8a16" if M <= 128 else "w8a8", M, 128, _k(i + 3))
    # weight-streaming kernels: nt + 16 * variant
    i = 0
    for variant in (1, 2):
        for nt in (1, 2):
            for M in (1, 16, 17, 49, 64):
                for split in (1, 3):
                    i += 1
                    add("stream", f"v{variant}nt{nt}s{split}", "bf16", M, 128, _k(i, (80, 336, 112, 704, 16, 1024)),
                        nt_hint=nt + 16 * variant, split_hint=split)
    for variant in (1, 2):
        for M in (1, 17, 64):
            for split in (1, 3):
                i += 1
                add("stream", f"v{variant}nt2s{split}", "w8a16", M, 128, _k(i, (336, 80, 704)),
                    nt_hint=2 + 16 * variant, split_hint=split)
    # tiled kernels: tile | ring-stage bits, split-K with a separate reduce
    stage_bits = {2: 0, 3: 16, 4: 32, 6: 48}
    for tile in (1, 2, 3, 5, 6):
        bm, bn = TILE_DIMS[tile]
        for stages in (2, 3, 4, 6):
            if (tile in (1, 5) and stages > 3) or (tile in (2, 6) and stages > 4):
                continue  # clamped to a depth already listed
            for split in (1, 3, 8):
                for M in ROWS[bm]:
                    i += 1
                    K = _k(i) if split == 1 else _k(i, (112, 704, 336) if split == 3 else (80, 704, 1024))
                    add("tiled", f"t{tile}st{stages}s{split}", "bf16", M, bn, K,
                        nt_hint=(tile | stage_bits[stages]) << 8, split_hint=split)
    for tile in (1, 2, 3, 5, 6):  # split-K combined in the launch (bit 256)
        bm, bn = TILE_DIMS[tile]
        for split in (3, 8):
            i += 1
            add("tiled", f"t{tile}st3s{split}c256", "bf16", ROWS[bm][-1], bn, _k(i, (336, 704, 80, 1024)),
                nt_hint=(tile | 16 | 256) << 8, split_hint=split)
    for K in (64, 80, 704, 1024):  # the 256x256 ping-pong kernel: 1, 2 (partial), 11 and 16 K-tiles
        add("pingpong", "t4", "bf16", 257, 256, K, nt_hint=4 << 8, split_hint=1)
    # gemm_mid: tile x depth x plain / interleaved; splits reduced separately and combined in the launch (bit 256)
    for tile, (bm, bn) in MID_DIMS.items():
        for M in ROWS[bm]:
            for depth in (16, 32, 48):
                for ilv in (0, 512):
                    i += 1
                    add("mid", f"t{tile}d{depth}i{ilv}s1", "bf16", M, bn, _k(i), glu=tile != 7,
                        nt_hint=(tile | depth | ilv) << 8, split_hint=1)
            for split, comb in ((3, 0), (8, 0), (3, 256), (8, 256)):
                i += 1
                add("mid", f"t{tile}s{split}c{comb}", "bf16", M, bn, _k(i, (112, 704, 336, 80, 1024)),
                    glu=tile != 7 or not comb, nt_hint=(tile | 16 | (512 if i % 2 else 0) | comb) << 8, split_hint=split)
    # gemm_dec: code x depth (bit 1024), splits separate and combined
    for code, bn in DEC_BN.items():
        for M in (1, 17, 33, 64):
            for depth in (0, 16, 32):
                i += 1
                add("dec", f"c{code}d{depth}s1", "bf16", M, bn, _k(i), glu=bn % 32 == 0,
                    nt_hint=(code | depth | 1024) << 8, split_hint=1)
        for M in (17, 64):
            for split, comb in ((3, 0), (8, 0), (3, 256), (8, 256)):
                i += 1
                K = _k(i, (336, 704, 80, 1024))
                add("dec", f"c{code}s{split}c{comb}", "bf16", M, bn, K,
                    glu=bn % 32 == 0 or (not comb and K > 64), nt_hint=(code | 16 | 1024 | comb) << 8, split_hint=split)
    # stream-K (bit 128): split_hint = workgroups per CU
    for tile, stages in ((1, 2), (1, 3), (2, 2), (2, 4), (3, 3), (3, 4)):
        bm, bn = TILE_DIMS[tile]
        for per_cu in (1, 2, 3):
            i += 1
            add("streamk", f"t{tile}st{stages}p{per_cu}", "bf16", ROWS[bm][-1], bn, _k(i, (336, 704, 1024, 80)),
                nt_hint=(tile | stage_bits[stages] | 128) << 8, split_hint=per_cu)
    # W8A16 tiled
    for tile, stages in ((3, 2), (3, 3), (3, 4), (2, 2), (2, 3), (1, 2)):
        bm, bn = TILE_DIMS[tile]
        for split in (1, 3):
            i += 1
            add("tiled", f"t{tile}st{stages}s{split}", "w8a16", ROWS[bm][i % len(ROWS[bm])], bn, _k(i, (336, 80, 704, 1024)),
                nt_hint=(tile | stage_bits[stages]) << 8, split_hint=split)
    # linear_w8a8: tiles 1-4 and the gemm_mid tiles (K % 128 == 0), plain and software-pipelined
    for tile, depth in ((1, 3), (1, 2), (2, 4), (2, 3), (3, 4), (3, 2)):
        bm, bn = TILE_DIMS[tile]
        for split in (1, 3):
            i += 1
            add("w8a8", f"t{tile}d{depth}s{split}", "w8a8", ROWS[bm][i % len(ROWS[bm])], bn, _k(i, (336, 80, 704, 1024, 112)),
                api="w8a8", tile=tile, depth=depth, split=split)
    add("w8a8", "t4", "w8a8", 257, 256, 1024, api="w8a8", tile=4, depth=0, split=1)
    for tile, (bm, bn) in MID_DIMS.items():
        for depth, ilv, split in ((3, False, 1), (4, True, 1), (3, True, 3), (4, False, 3)):
            i += 1
            add("w8a8-mid", f"t{tile}d{depth}i{int(ilv)}s{split}", "w8a8", ROWS[bm][i % len(ROWS[bm])], bn, 1024, api="w8a8",
                glu=tile != 7, tile=tile, depth=depth, split=split, ilv=ilv)
            add("mx-in", f"t{tile}d{depth}i{int(ilv)}s{split}", "mx", ROWS[bm][i % len(ROWS[bm])], bn, 1024, api="w8a8",
                glu=tile != 7, tile=tile, depth=depth, split=split, ilv=ilv)
    return P


def battery(p: Plan) -> list:
    """The cases one plan runs: integer (no activation + bias, relu + bias), saturated GELU (tanh, erf) and SwiGLU +
    bias, the x and w probes at as many offsets as it takes to visit every position of probe_ks(K), one x probe with a
    bias, one midrange case per activation."""
    M, N, K, f = p.M, p.N, p.K, p.flavour
    rounding = K > 64  # only the single-step K values check the sums alone
    cs = [integer_case(M, N, K, f, "none", True, rounding), integer_case(M, N, K, f, "relu", True, rounding),
          saturated_gelu_case(M, N, K, f, "gelu_tanh"), saturated_gelu_case(M, N, K, f, "gelu"),
          probe_case(M, N, K, f, bias=True), *probe_cases(M, N, K, f, False), *probe_cases(M, N, K, f, True),
          midrange_case(M, N, K, f, "gelu_tanh"), midrange_case(M, N, K, f, "gelu")]
    if p.Ng:
        cs += [swiglu_case(M, p.Ng, K, f), midrange_case(M, p.Ng, K, f, "silu")]
    return cs
