"""Windowed closed forms on top of tests/attn_cases.py: the same census / needle inputs for an attention whose row at
position p reads keys [lo, p] only, lo = max(kv_starts[b], p - window + 1, 0) (sliding window, Hugging Face's rule: W
keys including the row's own; kv_starts: the first key of the table row that may be read).

census  the histogram over [lo, p], divided by p - lo + 1.
needle  graded needles per (sequence, kv head), 64 nats apart: a target row's strong needle (192 nats) sits at ITS lo
        (or where the caller puts it), a 256-nat forbidden needle at lo - 1, 128-nat needles every `window` keys from
        there (every full window holds exactly one) and a 64-nat one at the sequence's first readable key (rows whose
        window is cut short there). A row returns the V row of the strongest needle inside [lo, p] - for the rows that
        legitimately reach the forbidden one, that one.

Every page wholly below a sequence's lowest lo is POISON, in K and in V, and its block-table entry is redirected to an
unowned poison page: a kernel that dereferences the stale entry or loads the released page shows it. Only valid page
ids are used.
"""
import dataclasses

import torch

import attn_cases as AC
from llmss_amd.ops import reference as R

LEVELS = {"base": 1.0, "period": 2.0, "strong": 3.0, "forbidden": 4.0}  # x 64 nats


def _kvs(geo, kv_starts):
    return torch.zeros(geo.B, dtype=torch.int64) if kv_starts is None else torch.as_tensor(kv_starts).long()


def row_lo(geo, window, kv_starts=None, pos=None):
    """[T] first key of every query row (``pos``: the positions the window is taken from, default the row's own)."""
    pos = geo.row_pos if pos is None else pos
    lo = _kvs(geo, kv_starts)[geo.row_seq].clamp(min=0)
    return torch.maximum(lo, pos - window + 1) if window > 0 else lo


def seq_lo(geo, window, kv_starts=None):
    """[B] the lowest lo of each sequence's rows (its first row's)."""
    return row_lo(geo, window, kv_starts)[geo.cu_q[:-1].long()]


def _cache_rows(cache, geo, D):
    """[nb, nkv, bs, D(+16)] -> fp32 [nb * bs, nkv, D]"""
    x = R.kv_rows_dequant(cache, D) if cache.dtype == torch.uint8 else cache.float()
    return x.permute(0, 2, 1, 3).reshape(geo.nb * geo.bs, x.shape[1], D)


def _release(geo, window, kv_starts, krows, vrows):
    """Poison the pages wholly below each sequence's lowest lo and redirect their table entries."""
    table = geo.table.clone()
    bs = geo.bs
    for b, lo in enumerate(seq_lo(geo, window, kv_starts).tolist()):
        for i in range(lo // bs):
            pg = int(geo.table[b, i])
            krows[pg * bs: (pg + 1) * bs] = AC.POISON
            vrows[pg * bs: (pg + 1) * bs] = AC.POISON
            table[b, i] = geo.unowned[0]
    assert 0 <= int(table.min()) and int(table.max()) < geo.nb
    return dataclasses.replace(geo, table=table)


def _assemble(kind, geo, nh, nkv, D, kv8, device, q, krows, vrows, expected, extra, window, kv_starts):
    geo2 = _release(geo, window, kv_starts, krows, vrows)
    extra = dict(extra, window=int(window), kv_starts=None if kv_starts is None else _kvs(geo, kv_starts))
    return AC.Case(kind, geo2, nh, nkv, D, kv8, AC._padded(q, device), AC._to_cache(krows, geo, kv8, device),
                   AC._to_cache(vrows, geo, kv8, device), None, expected.to(device), extra)


def kv_starts_dev(case, device):
    ks = case.extra["kv_starts"]
    return None if ks is None else ks.to(torch.int32).to(device)


# ---------------------------------------------------------------------------------------------- census
def census(geo, nh, nkv, D, window, kv_starts=None, digit_pass=0, base=64, kv8=False, device="cpu", seed=0):
    c = AC.census(geo, nh, nkv, D, digit_pass, base=base, kv8=kv8, seed=seed)
    krows, vrows = _cache_rows(c.k_cache, geo, D), _cache_rows(c.v_cache, geo, D)
    vals = vrows[geo.slot]  # 0 / 1: exact in either cache type
    cs = torch.cat([torch.zeros(1, nkv, D), vals.cumsum(0)])
    first = geo.key_start[geo.row_seq]
    lo = row_lo(geo, window, kv_starts)
    n = geo.row_pos - lo + 1
    assert bool((n >= 1).all()), "a census row needs a key"
    cnt = cs[first + geo.row_pos + 1] - cs[first + lo]
    expected = (cnt / n[:, None, None]).repeat_interleave(nh // nkv, 1).reshape(geo.T, nh * D)
    return _assemble("census", geo, nh, nkv, D, kv8, device, torch.zeros(geo.T, nh * D), krows, vrows, expected,
                     {"digit_pass": digit_pass}, window, kv_starts)


# ---------------------------------------------------------------------------------------------- needle
def selection(case, lo, hi):
    """[T, nkv] index (into the sequence's keys) of the strongest needle inside [lo, hi] per row, -1: none;
    and whether it is the only one of its level there."""
    geo = case.geo
    npos, nlvl = case.extra["npos"][geo.row_seq], case.extra["nlvl"][geo.row_seq]  # [T, nkv, M]
    inside = (npos >= lo[:, None, None]) & (npos <= hi[:, None, None]) & (npos >= 0)
    lvl = torch.where(inside, nlvl, torch.zeros(()))
    top, arg = lvl.max(-1)
    sel = torch.where(top > 0, npos.gather(-1, arg[..., None])[..., 0], torch.full_like(arg, -1))
    unique = (lvl == top[..., None]).sum(-1) == 1
    return sel, unique | (top == 0)


def needle(geo, nh, nkv, D, window, kv_starts=None, target=None, strong=None, kv8=False, device="cpu", seed=0):
    """target [B, nkv]: the row (index inside the chunk) whose lo carries the strong needle, default the last row;
    strong [B, nkv]: another position for it (>= that lo). The forbidden needle stays at lo - 1."""
    B, T, G = geo.B, geo.T, nh // nkv
    qlen, ctx = torch.tensor(geo.qlen), torch.tensor(geo.ctx)
    target = (qlen - 1)[:, None].expand(B, nkv) if target is None else torch.as_tensor(target).long().view(B, nkv)
    lo_rows = row_lo(geo, window, kv_starts)
    lo_t = lo_rows[geo.cu_q[:-1].long()[:, None] + target]  # [B, nkv]
    strong = lo_t if strong is None else torch.as_tensor(strong).long().view(B, nkv)
    assert bool(((strong >= lo_t) & (strong < ctx[:, None])).all())
    first_key = _kvs(geo, kv_starts).clamp(min=0)
    placed = []  # per (b, k): {position: level}
    for b in range(B):
        for k in range(nkv):
            d = {int(first_key[b]): LEVELS["base"]}
            if window > 0:
                for p in range(int(lo_t[b, k]) % window, geo.ctx[b], window):
                    if p >= int(first_key[b]) and p != int(lo_t[b, k]):
                        d[p] = LEVELS["period"]
            d[int(strong[b, k])] = LEVELS["strong"]
            if int(lo_t[b, k]) >= 1:
                d[int(lo_t[b, k]) - 1] = LEVELS["forbidden"]
            placed.append(d)
    M = max(len(d) for d in placed)
    npos = torch.full((B, nkv, M), -1, dtype=torch.int64)
    nlvl = torch.zeros(B, nkv, M)
    for i, d in enumerate(placed):
        npos[i // nkv, i % nkv, : len(d)] = torch.tensor(sorted(d))
        nlvl[i // nkv, i % nkv, : len(d)] = torch.tensor([d[p] for p in sorted(d)])
    base = AC.needle(geo, nh, nkv, D, strong, torch.where(strong > 0, 0, -1), kv8=kv8, seed=seed)
    u = base.q[0, :D].float()
    c = 64.0 / (R.softmax_scale(D) * float((u * u).sum()))
    vrows = _cache_rows(base.v_cache, geo, D)
    krows = torch.full_like(vrows, AC.POISON)
    kvals = torch.zeros(geo.pos.numel(), nkv, D)
    on = npos >= 0
    kv_idx = torch.arange(nkv)[None, :, None].expand(B, nkv, M)
    kvals[(geo.key_start[:, None, None] + npos)[on], kv_idx[on]] = nlvl[on][:, None] * c * u
    krows[geo.slot] = kvals
    krows[geo.past_slot] = 4.0 * c * u  # as AC.needle: past the context and in a page no sequence owns
    pg = int(geo.unowned[1])
    krows[pg * geo.bs: (pg + 1) * geo.bs] = 4.0 * c * u
    case = AC.Case("needle", geo, nh, nkv, D, kv8, None, None, None, None, torch.empty(0),
                   {"npos": npos, "nlvl": nlvl, "strong": strong, "target": target})
    sel, unique = selection(case, lo_rows, geo.row_pos)
    assert bool((sel >= 0).all()) and bool(unique.all()), "every row needs exactly one strongest needle in its window"
    stored = vrows[geo.slot].to(torch.bfloat16)  # what the cache holds, as bf16
    expected = stored[geo.key_start[geo.row_seq][:, None] + sel, torch.arange(nkv)[None, :].expand(T, nkv)]
    expected = expected.repeat_interleave(G, 1).reshape(T, nh * D)
    return _assemble("needle", geo, nh, nkv, D, kv8, device, u.repeat(T, nh), krows, vrows, expected, case.extra,
                     window, kv_starts)


def random_case(geo, nh, nkv, D, window, kv_starts=None, kv8=False, device="cpu", seed=0):
    c = AC.random_case(geo, nh, nkv, D, kv8=kv8, seed=seed)
    krows, vrows = _cache_rows(c.k_cache, geo, D), _cache_rows(c.v_cache, geo, D)
    return _assemble("random", geo, nh, nkv, D, kv8, device, c.q.float(), krows, vrows, torch.empty(0), {}, window,
                     kv_starts)


# ------------------------------------------------------------------------------- windowed fp32 oracle
def oracle(case, lo_shift=0, last_row_window=False, emulate=False):
    """fp32 [T, nh*D]: row r attends keys [lo(r) + lo_shift, p(r)]. ``last_row_window``: the (wrong) window of the
    sequence's last row for every row. ``emulate``: P and the output rounded to bf16 (AC.oracle_rows). A row without
    a key gives 0."""
    geo, nh, nkv, D = case.geo, case.nh, case.nkv, case.D
    G = nh // nkv
    pos = torch.tensor(geo.ctx)[geo.row_seq] - 1 if last_row_window else None
    lo = row_lo(geo, case.extra["window"], case.extra["kv_starts"], pos) + lo_shift
    out = torch.zeros(geo.T, nh * D)
    cu = geo.cu_q.tolist()
    for b in range(geo.B):
        a, e = cu[b], cu[b + 1]
        qq = case.q[a:e].cpu().float().view(e - a, nh, D).transpose(0, 1)
        k = R.gather_kv(case.k_cache.cpu(), geo.table[b], geo.ctx[b]).float().repeat_interleave(G, 0)
        v = R.gather_kv(case.v_cache.cpu(), geo.table[b], geo.ctx[b]).float().repeat_interleave(G, 0)
        key = torch.arange(geo.ctx[b])[None, :]
        live = (key >= lo[a:e, None]) & (key <= geo.row_pos[a:e, None])
        s = (torch.matmul(qq, k.transpose(1, 2)) * case.scale).masked_fill(~live, float("-inf"))
        v = torch.where(live.any(0)[None, :, None], v, torch.zeros(()))  # poison x 0 stays out of the product
        if emulate:
            p = torch.exp(s - s.amax(-1, keepdim=True)).nan_to_num(0.0).to(torch.bfloat16).float()
            o = (torch.matmul(p, v) / p.sum(-1, keepdim=True)).nan_to_num(0.0).to(torch.bfloat16).float()
        else:
            o = torch.matmul(torch.softmax(s, -1).nan_to_num(0.0), v)
        out[a:e] = o.transpose(0, 1).reshape(e - a, nh * D)
    return out
