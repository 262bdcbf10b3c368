"""Attention inputs whose correct output is known in closed form, so a test can tell exactly WHICH keys a
kernel included (tests/test_attn_cases_cpu.py proves the checks fail on a one-key error;
tests/test_attn_exact_gpu.py runs them against the HIP kernels).

census  q = 0: every score is 0, every probability 1 (exact in fp32 and in bf16), so the output of a row is
        the histogram of the V rows of the keys it attended, divided by their number. V of key t is multi-hot
        at a column that depends on a digit of t, the kv head and the sequence.
needle  every query head is one vector u; K = 0 except one "needle" key per (sequence, kv head) that scores 64
        nats above the rest, so the output is that key's V row to the bit. Stronger forbidden needles sit just
        past the context and in a page no sequence owns.

Every cache row that no sequence owns at a position < ctx, and every pad column of a strided q / qkv, is POISON
(finite: a kernel may load it and multiply it by a zero probability).
"""
from dataclasses import dataclass, field
from typing import Optional

import torch

from llmss_amd.ops import reference as R

POISON = 9984.0  # 1e4 as bf16 holds it
MAX_COUNT = 80  # census: a one-key error moves an entry by 1/n > (2^-7 + 2^-8) c/n only while c < 85
PAD = 64        # pad columns of the strided q / qkv
TAIL = 2.1e-23  # needle, fp8 rows: what 2^14 keys 64 nats below the needle can add (needle_bad)


@dataclass
class Geometry:
    """Paged layout of B sequences: sequence b holds keys [0, ctx[b]) and its last qlen[b] keys are the query
    rows of this step (decode: qlen = 1)."""
    ctx: list
    qlen: list
    bs: int
    nb: int
    table: torch.Tensor      # [B + 2, maxb] int32; rows >= B and entries past the spare page: an unowned page
    unowned: torch.Tensor    # page ids no sequence owns
    seq_id: torch.Tensor     # [N] sequence of key i (keys of all sequences back to back)
    pos: torch.Tensor        # [N] its position
    slot: torch.Tensor       # [N] its cache row (page * bs + offset)
    key_start: torch.Tensor  # [B] index of each sequence's key 0
    past_slot: torch.Tensor  # [B] cache row of position ctx (mapped by the table, out of context)
    cu_q: torch.Tensor       # [B + 1] int32
    row_seq: torch.Tensor    # [T] sequence of query row r
    row_pos: torch.Tensor    # [T] its position

    @property
    def B(self):
        return len(self.ctx)

    @property
    def T(self):
        return int(self.row_seq.numel())

    @property
    def ctx_lens(self):
        return torch.tensor(self.ctx, dtype=torch.int32)


def geometry(ctx, qlen=None, bs=16, seed=0) -> Geometry:
    """Block-table rows cut from one randperm, one spare page after each sequence's last page."""
    g = torch.Generator().manual_seed(seed)
    B = len(ctx)
    qlen = [1] * B if qlen is None else list(qlen)
    assert all(1 <= q <= c for q, c in zip(qlen, ctx))
    own = [(c + bs - 1) // bs + 1 for c in ctx]
    n_un = 3
    nb = sum(own) + n_un
    perm = torch.randperm(nb, generator=g).to(torch.int32)
    unowned = perm[nb - n_un:]
    table = torch.full((B + 2, max(own) + 1), int(unowned[0]), dtype=torch.int32)
    off = 0
    for b in range(B):  # per sequence, not per token
        table[b, : own[b]] = perm[off: off + own[b]]
        off += own[b]
    ctx_t, q_t = torch.tensor(ctx), torch.tensor(qlen)
    key_start = torch.cumsum(ctx_t, 0) - ctx_t
    seq_id = torch.repeat_interleave(torch.arange(B), ctx_t)
    pos = torch.arange(int(ctx_t.sum())) - key_start[seq_id]
    slot = table[seq_id, pos // bs].long() * bs + pos % bs
    past_slot = table[torch.arange(B), ctx_t // bs].long() * bs + ctx_t % bs
    cu = torch.zeros(B + 1, dtype=torch.int64)
    cu[1:] = torch.cumsum(q_t, 0)
    row_seq = torch.repeat_interleave(torch.arange(B), q_t)
    row_pos = (ctx_t - q_t)[row_seq] + torch.arange(int(q_t.sum())) - cu[row_seq]
    return Geometry(list(ctx), qlen, bs, nb, table, unowned, seq_id, pos, slot, key_start, past_slot,
                    cu.to(torch.int32), row_seq, row_pos)


def packed_geometry(lens) -> Geometry:
    """Prefill: sequences packed back to back, every key is a query row (no pages)."""
    B = len(lens)
    len_t = torch.tensor(lens)
    key_start = torch.cumsum(len_t, 0) - len_t
    seq_id = torch.repeat_interleave(torch.arange(B), len_t)
    pos = torch.arange(int(len_t.sum())) - key_start[seq_id]
    cu = torch.zeros(B + 1, dtype=torch.int32)
    cu[1:] = torch.cumsum(len_t, 0)
    e = torch.empty(0, dtype=torch.int64)
    return Geometry(list(lens), list(lens), 0, 0, e, e, seq_id, pos, torch.arange(pos.numel()), key_start, e, cu,
                    seq_id, pos)


@dataclass
class Case:
    kind: str                    # "census" | "needle"
    geo: Geometry
    nh: int
    nkv: int
    D: int
    kv8: bool
    q: Optional[torch.Tensor]    # paged: [T, nh*D] view of a poison-padded buffer
    k_cache: Optional[torch.Tensor]
    v_cache: Optional[torch.Tensor]
    qkv: Optional[torch.Tensor]  # packed: [T, (nh + 2 nkv) D] view of a poison-padded buffer
    expected: torch.Tensor       # [T, nh*D]: fp32 (census) or the exact bf16 rows (needle)
    extra: dict = field(default_factory=dict)

    @property
    def scale(self):
        return R.softmax_scale(self.D)


def _padded(x: torch.Tensor, device) -> torch.Tensor:
    """bf16 [T, W] as a view of a [T, W + PAD] buffer on ``device`` whose pad columns are poison."""
    T, W = x.shape
    full = torch.full((T, W + PAD), POISON, dtype=torch.bfloat16)
    full[:, :W] = x.to(torch.bfloat16)
    return full.to(device)[:, :W]  # moved whole: a moved view would arrive dense


def _to_cache(rows: torch.Tensor, geo: Geometry, kv8: bool, device) -> torch.Tensor:
    """[nb*bs, nkv, D] fp32 rows -> the paged cache [nb, nkv, bs, D] (bf16) or fp8 rows [.., D + 16]."""
    x = rows.view(geo.nb, geo.bs, rows.shape[1], rows.shape[2]).permute(0, 2, 1, 3).contiguous()
    return (R.kv_rows_quant(x) if kv8 else x.to(torch.bfloat16)).to(device)


def _stored(vals: torch.Tensor, kv8: bool) -> torch.Tensor:
    """The values a cache of this type holds for ``vals``, as bf16."""
    if kv8:
        return R.kv_rows_dequant(R.kv_rows_quant(vals), vals.shape[-1]).to(torch.bfloat16)
    return vals.to(torch.bfloat16)


def _finish(kind, geo, nh, nkv, D, kv8, device, q, kvals, vvals, expected, extra=None, krows=None, vrows=None):
    """Assemble a Case: paged (krows / vrows hold every cache row) or packed (kvals / vvals per key)."""
    if geo.bs:
        return Case(kind, geo, nh, nkv, D, kv8, _padded(q, device), _to_cache(krows, geo, kv8, device),
                    _to_cache(vrows, geo, kv8, device), None, expected.to(device), extra or {})
    T = geo.T
    qkv = torch.cat([q, kvals.reshape(T, nkv * D), vvals.reshape(T, nkv * D)], 1)
    return Case(kind, geo, nh, nkv, D, False, None, None, None, _padded(qkv, device), expected.to(device),
                extra or {})


# ---------------------------------------------------------------------------------------------- census
def census(geo: Geometry, nh, nkv, D, digit_pass=0, base=64, kv8=False, device="cpu", seed=0) -> Case:
    """digit_pass 0: digit = t % base (any dropped, extra or duplicated key); 1: (t // base) % base (a key
    replaced by one base * k positions away)."""
    g = torch.Generator().manual_seed(seed)
    N, T, G = geo.pos.numel(), geo.T, nh // nkv
    digit = geo.pos % base if digit_pass == 0 else (geo.pos // base) % base
    col = (digit[:, None] + 7 * torch.arange(nkv)[None, :] + 13 * geo.seq_id[:, None]) % base  # [N, nkv]
    vals = torch.zeros(N, nkv, D // base, base)
    vals.scatter_(3, col[:, :, None, None].expand(N, nkv, D // base, 1), 1.0)
    vals = vals.view(N, nkv, D)
    kvals = torch.randn(N, nkv, D, generator=g) * (POISON / 4)  # finite garbage: q = 0, it must not matter
    # closed form: histogram of keys [0, position] of the row's own sequence
    cs = vals.cumsum(0)
    first = geo.key_start[geo.row_seq]
    cnt = cs[first + geo.row_pos]
    cnt = cnt - torch.where((first > 0)[:, None, None], cs[(first - 1).clamp(min=0)], torch.zeros(()))
    assert float(cnt.max()) <= MAX_COUNT, f"census entry counts {float(cnt.max()):.0f} keys (> {MAX_COUNT})"
    expected = (cnt / (geo.row_pos + 1)[:, None, None]).repeat_interleave(G, 1).reshape(T, nh * D)
    q = torch.zeros(T, nh * D)
    krows = vrows = None
    if geo.bs:
        krows = torch.full((geo.nb * geo.bs, nkv, D), POISON)
        vrows = torch.full((geo.nb * geo.bs, nkv, D), POISON)
        krows[geo.slot], vrows[geo.slot] = kvals, vals
    return _finish("census", geo, nh, nkv, D, kv8, device, q, kvals, vals, expected, {"digit_pass": digit_pass}, krows,
                   vrows)


def census_bad(out: torch.Tensor, expected: torch.Tensor) -> torch.Tensor:
    """Elementwise failures: entries that count no key must be exactly 0, the others within 2^-7 relative
    (one bf16 rounding of the result, 2^-8, plus the fp32 divide). NaN fails."""
    o = out.float()
    ok = torch.where(expected == 0, o == 0, (o - expected).abs() <= expected * 2.0 ** -7)
    return ~ok


# ---------------------------------------------------------------------------------------------- needle
def needle(geo: Geometry, nh, nkv, D, strong, weak=None, kv8=False, device="cpu", seed=0) -> Case:
    """strong / weak: [B, nkv] key positions (weak: -1 = none). The weak needle scores 64 nats, the strong one
    128, the forbidden ones (position ctx, one unowned page; packed: none) 256. A row at position p returns
    V[strong] if strong <= p, else V[weak]."""
    g = torch.Generator().manual_seed(seed)
    N, T, G, B = geo.pos.numel(), geo.T, nh // nkv, geo.B
    strong = torch.as_tensor(strong).long().view(B, nkv)
    weak = torch.full_like(strong, -1) if weak is None else torch.as_tensor(weak).long().view(B, nkv)
    u = torch.randn(D, generator=g).to(torch.bfloat16).float()
    c = 64.0 / (R.softmax_scale(D) * float((u * u).sum()))
    kvals = torch.zeros(N, nkv, D)
    vvals = torch.randn(N, nkv, D, generator=g).to(torch.bfloat16).float()
    kv_idx = torch.arange(nkv)[None, :].expand(B, nkv)
    ctx_t = torch.tensor(geo.ctx)[:, None]
    assert bool(((strong >= 0) & (strong < ctx_t) & (weak < strong)).all())
    for where, mult in ((weak, 1.0), (strong, 2.0)):
        on = where >= 0
        kvals[(geo.key_start[:, None] + where)[on], kv_idx[on]] = mult * c * u
    # closed form: the selected key's V row as the cache stores it
    rp = geo.row_pos[:, None]
    st, wk = strong[geo.row_seq], weak[geo.row_seq]  # [T, nkv]
    sel = torch.where(st <= rp, st, wk)
    assert bool((sel >= 0).all()), "a row before the strong needle needs a weak one"
    stored = _stored(vvals, kv8 and bool(geo.bs))
    expected = stored[geo.key_start[geo.row_seq][:, None] + sel, kv_idx[:1].expand(T, nkv)]  # [T, nkv, D]
    expected = expected.repeat_interleave(G, 1).reshape(T, nh * D)
    q = u.repeat(T, nh)
    krows = vrows = None
    if geo.bs:
        krows = torch.full((geo.nb * geo.bs, nkv, D), POISON)
        vrows = torch.full((geo.nb * geo.bs, nkv, D), POISON)
        krows[geo.slot], vrows[geo.slot] = kvals, vvals
        krows[geo.past_slot] = 4.0 * c * u
        pg = int(geo.unowned[1])
        krows[pg * geo.bs: (pg + 1) * geo.bs] = 4.0 * c * u
    return _finish("needle", geo, nh, nkv, D, kv8, device, q, kvals, vvals, expected,
                   {"strong": strong, "weak": weak}, krows, vrows)


def _ordered(x: torch.Tensor) -> torch.Tensor:
    """bf16 -> int32 that orders like the values (adjacent values differ by 1; -0 == +0)."""
    i = x.contiguous().view(torch.int16).to(torch.int32)
    return torch.where(i < 0, -(i & 0x7FFF), i)


def needle_bad(out: torch.Tensor, expected: torch.Tensor, kv8: bool) -> torch.Tensor:
    """Elementwise failures: bf16 caches bit for bit, fp8 caches within one bf16 ulp (or TAIL of an exact zero).
    NaN fails."""
    if not kv8:
        return out != expected
    # an fp8 row often holds exact zeros, where an ulp means nothing: there the rest of the softmax shows. Every
    # other key weighs <= e^-64 = 1.6e-28 of the selected one; 2^14 keys of |V| <= 8 add up to < 2.1e-23 (TAIL)
    near = (_ordered(out) - _ordered(expected)).abs() <= 1
    tail = (out.float() - expected.float()).abs() <= TAIL
    return ~(near | tail) | out.isnan()


def bad_rows(case: Case, out: torch.Tensor) -> torch.Tensor:
    """[T, nh] bool: (row, head) pairs whose output misses the closed form."""
    exp = case.expected[: out.shape[0]]  # a launch over the first sequences only
    bad = census_bad(out, exp) if case.kind == "census" else needle_bad(out, exp, case.kv8)
    return bad.view(out.shape[0], case.nh, case.D).any(-1)


def assert_exact(case: Case, out: torch.Tensor, what: str = ""):
    bad = bad_rows(case, out)
    if bool(bad.any()):
        r, h = bad.nonzero()[0].tolist()
        geo = case.geo
        b = int(geo.row_seq[r])
        got = out[r].view(case.nh, case.D)[h].float()
        exp = case.expected[r].view(case.nh, case.D)[h].float()
        d = int((got - exp).abs().nan_to_num(float("inf")).argmax())
        raise AssertionError(
            f"{what} {case.kind}: {int(bad.sum())} (row, head) pairs wrong; first row {r} (sequence {b}, position "
            f"{int(geo.row_pos[r])}, ctx {geo.ctx[b]}) head {h}: column {d} got {float(got[d]):.6g}, expected "
            f"{float(exp[d]):.6g}; sequences {sorted({int(geo.row_seq[i]) for i in bad.any(1).nonzero()[:, 0]})}")


def random_case(geo: Geometry, nh, nkv, D, kv8=False, device="cpu", seed=0) -> Case:
    """Ordinary randn q / K / V (poison everywhere else) for the signal-relative error bound; no closed form."""
    g = torch.Generator().manual_seed(seed)
    N, T = geo.pos.numel(), geo.T
    q = torch.randn(T, nh * D, generator=g)
    kvals, vvals = torch.randn(N, nkv, D, generator=g), torch.randn(N, nkv, D, generator=g)
    krows = vrows = None
    if geo.bs:
        krows = torch.full((geo.nb * geo.bs, nkv, D), POISON)
        vrows = torch.full((geo.nb * geo.bs, nkv, D), POISON)
        krows[geo.slot], vrows[geo.slot] = kvals, vvals
    return _finish("random", geo, nh, nkv, D, kv8, device, q, kvals, vvals, torch.empty(0), None, krows, vrows)


def signal_error(x: torch.Tensor, ref: torch.Tensor, nh, D) -> float:
    """Largest error of a (row, head) relative to the RMS of the fp32 reference for that (row, head)."""
    T = ref.shape[0]
    err = (x.float().cpu() - ref).view(T, nh, D).abs().amax(-1)
    return float((err / ref.view(T, nh, D).pow(2).mean(-1).sqrt()).max())


# ------------------------------------------------------------------------ oracle variants with knobs
def oracle_rows(q, k, v, qpos, scale, mask_shift=0, emulate=False):
    """q [nh, R, D], k / v [nh, n, D] fp32: row r attends keys <= qpos[r] + mask_shift. ``emulate``: P and the
    output rounded to bf16, the row sum taken over the rounded P (what the MFMA kernels do)."""
    n = k.shape[1]
    s = torch.matmul(q, k.transpose(1, 2)) * scale
    s = s.masked_fill(torch.arange(n, device=q.device)[None, :] > (qpos[:, None] + mask_shift), float("-inf"))
    if not emulate:
        return torch.matmul(torch.softmax(s, -1), v)
    p = torch.exp(s - s.amax(-1, keepdim=True)).to(torch.bfloat16).float()
    return (torch.matmul(p, v) / p.sum(-1, keepdim=True)).to(torch.bfloat16).float()


def oracle(case: Case, mask_shift=0, emulate=False) -> torch.Tensor:
    """R.attn_decode / attn_extend / attn_prefill on a Case, with a shifted causal mask or bf16 emulation.
    Returns fp32 [T, nh*D]."""
    geo, nh, nkv, D = case.geo, case.nh, case.nkv, case.D
    G = nh // nkv
    out = torch.zeros(geo.T, nh * D)
    cu = geo.cu_q.tolist()
    for b in range(geo.B):
        a, e = cu[b], cu[b + 1]
        if geo.bs:
            qq = case.q[a:e].cpu().float()
            k = R.gather_kv(case.k_cache.cpu(), geo.table[b], geo.ctx[b]).float()
            v = R.gather_kv(case.v_cache.cpu(), geo.table[b], geo.ctx[b]).float()
        else:
            x = case.qkv[a:e].cpu().float()
            qq = x[:, : nh * D]
            k = x[:, nh * D: (nh + nkv) * D].view(e - a, nkv, D).transpose(0, 1)
            v = x[:, (nh + nkv) * D:].view(e - a, nkv, D).transpose(0, 1)
        qq = qq.view(e - a, nh, D).transpose(0, 1)
        o = oracle_rows(qq, k.repeat_interleave(G, 0), v.repeat_interleave(G, 0), geo.row_pos[a:e], case.scale,
                        mask_shift, emulate)
        out[a:e] = o.transpose(0, 1).reshape(e - a, nh * D)
    return out


# ------------------------------------------------------------------------------- needle placements
def pick(cands, n, k):
    """The k-th (rotating) of the candidate positions that lie in [0, n)."""
    c = sorted({x for x in cands if 0 <= x < n})
    return c[k % len(c)]


def decode_needles(geo: Geometry, nkv, edges, rot=0):
    """[B, nkv] needle positions rotating over key 0, ctx - 1, page edges and the given partition / tile edges
    (each edge e stands for the pair e - 1, e)."""
    out = torch.zeros(geo.B, nkv, dtype=torch.int64)
    for b, n in enumerate(geo.ctx):
        cands = [0, n - 1, geo.bs - 1, geo.bs, (n - 1) // geo.bs * geo.bs, (n - 1) // geo.bs * geo.bs - 1]
        for e in edges:
            cands += [e - 1, e]
        for k in range(nkv):
            out[b, k] = pick(cands, n, b + k + rot)
    return out


def chunk_needles(geo: Geometry, nkv, edges, rot=0):
    """(strong, weak) [B, nkv]: the strong needle on a row of the chunk, on and next to the given row edges; the
    weak one at key 0 (none where the strong one is key 0)."""
    strong = torch.zeros(geo.B, nkv, dtype=torch.int64)
    for b, (n, ql) in enumerate(zip(geo.ctx, geo.qlen)):
        cands = [0, 1, ql - 1]
        for e in edges:
            cands += [e - 1, e, e + 1]
        for k in range(nkv):
            strong[b, k] = n - ql + pick(cands, ql, b + k + rot)
    weak = torch.where(strong > 0, torch.zeros_like(strong), torch.full_like(strong, -1))
    return strong, weak
