"""The decode staging blob (llmss_amd/engine/staging.py) on the CPU: its byte layout for the eight on/off combinations
of penalties, constraints and min_p against a table recorded from the hand-written offsets it replaced, what ``fill``
and ``reset`` write, the recorded blobs of that earlier ``fill`` (tests/golden/staging_fill.npz), and the slot pool."""
import itertools
import os
import random

import numpy as np
import pytest
import torch

from llmss_amd.engine import LLMEngine
from llmss_amd.engine.engine import _DecodeBuffers
from llmss_amd.engine.staging import LANES, SLOT_LANES, SlotPool
from llmss_amd.models.config import get_preset
from llmss_amd.models.decoder import DecoderLM
from llmss_amd.models.weights import random_weights

B, MB = 8, 4
CPU = torch.device("cpu")
COMBOS = list(itertools.product((False, True), repeat=3))  # (penalties, constraints, min_p)
ALWAYS = ("ids", "pos", "slots", "seeds", "ctx", "topk", "bt", "temp", "topp")
ORDER = ("ids", "pos", "slots", "seeds", "ctx", "topk", "bt", "pslot", "cslot", "cnout", "temp", "topp", "rep", "pres",
         "freq", "lnmp")
PADS = {"ids": 0, "pos": 0, "slots": -1, "seeds": 0, "ctx": 0, "topk": 1, "bt": 0, "pslot": -1, "cslot": -1,
        "cnout": 0, "temp": 0, "topp": 1, "rep": 1, "pres": 0, "freq": 0, "lnmp": -np.inf}
# (penalties, constraints, min_p) -> (blob bytes, lanes' (name, byte offset, bytes, dtype)): printed by the buffers
# with hand-written offsets, for _DecodeBuffers(8, 4, cpu, 0, penalties, constraints, min_p)
LAYOUT = {
    (False, False, False): (512, (
        ('ids', 0, 64, 'int64'), ('pos', 64, 64, 'int64'), ('slots', 128, 64, 'int64'), ('seeds', 192, 64, 'int64'),
        ('ctx', 256, 32, 'int32'), ('topk', 288, 32, 'int32'), ('bt', 320, 128, 'int32'), ('temp', 448, 32, 'float32'),
        ('topp', 480, 32, 'float32'),
    )),
    (False, False, True): (544, (
        ('ids', 0, 64, 'int64'), ('pos', 64, 64, 'int64'), ('slots', 128, 64, 'int64'), ('seeds', 192, 64, 'int64'),
        ('ctx', 256, 32, 'int32'), ('topk', 288, 32, 'int32'), ('bt', 320, 128, 'int32'), ('temp', 448, 32, 'float32'),
        ('topp', 480, 32, 'float32'), ('lnmp', 512, 32, 'float32'),
    )),
    (False, True, False): (576, (
        ('ids', 0, 64, 'int64'), ('pos', 64, 64, 'int64'), ('slots', 128, 64, 'int64'), ('seeds', 192, 64, 'int64'),
        ('ctx', 256, 32, 'int32'), ('topk', 288, 32, 'int32'), ('bt', 320, 128, 'int32'), ('cslot', 448, 32, 'int32'),
        ('cnout', 480, 32, 'int32'), ('temp', 512, 32, 'float32'), ('topp', 544, 32, 'float32'),
    )),
    (False, True, True): (608, (
        ('ids', 0, 64, 'int64'), ('pos', 64, 64, 'int64'), ('slots', 128, 64, 'int64'), ('seeds', 192, 64, 'int64'),
        ('ctx', 256, 32, 'int32'), ('topk', 288, 32, 'int32'), ('bt', 320, 128, 'int32'), ('cslot', 448, 32, 'int32'),
        ('cnout', 480, 32, 'int32'), ('temp', 512, 32, 'float32'), ('topp', 544, 32, 'float32'),
        ('lnmp', 576, 32, 'float32'),
    )),
    (True, False, False): (640, (
        ('ids', 0, 64, 'int64'), ('pos', 64, 64, 'int64'), ('slots', 128, 64, 'int64'), ('seeds', 192, 64, 'int64'),
        ('ctx', 256, 32, 'int32'), ('topk', 288, 32, 'int32'), ('bt', 320, 128, 'int32'), ('pslot', 448, 32, 'int32'),
        ('temp', 480, 32, 'float32'), ('topp', 512, 32, 'float32'), ('rep', 544, 32, 'float32'),
        ('pres', 576, 32, 'float32'), ('freq', 608, 32, 'float32'),
    )),
    (True, False, True): (672, (
        ('ids', 0, 64, 'int64'), ('pos', 64, 64, 'int64'), ('slots', 128, 64, 'int64'), ('seeds', 192, 64, 'int64'),
        ('ctx', 256, 32, 'int32'), ('topk', 288, 32, 'int32'), ('bt', 320, 128, 'int32'), ('pslot', 448, 32, 'int32'),
        ('temp', 480, 32, 'float32'), ('topp', 512, 32, 'float32'), ('rep', 544, 32, 'float32'),
        ('pres', 576, 32, 'float32'), ('freq', 608, 32, 'float32'), ('lnmp', 640, 32, 'float32'),
    )),
    (True, True, False): (704, (
        ('ids', 0, 64, 'int64'), ('pos', 64, 64, 'int64'), ('slots', 128, 64, 'int64'), ('seeds', 192, 64, 'int64'),
        ('ctx', 256, 32, 'int32'), ('topk', 288, 32, 'int32'), ('bt', 320, 128, 'int32'), ('pslot', 448, 32, 'int32'),
        ('cslot', 480, 32, 'int32'), ('cnout', 512, 32, 'int32'), ('temp', 544, 32, 'float32'),
        ('topp', 576, 32, 'float32'), ('rep', 608, 32, 'float32'), ('pres', 640, 32, 'float32'),
        ('freq', 672, 32, 'float32'),
    )),
    (True, True, True): (736, (
        ('ids', 0, 64, 'int64'), ('pos', 64, 64, 'int64'), ('slots', 128, 64, 'int64'), ('seeds', 192, 64, 'int64'),
        ('ctx', 256, 32, 'int32'), ('topk', 288, 32, 'int32'), ('bt', 320, 128, 'int32'), ('pslot', 448, 32, 'int32'),
        ('cslot', 480, 32, 'int32'), ('cnout', 512, 32, 'int32'), ('temp', 544, 32, 'float32'),
        ('topp', 576, 32, 'float32'), ('rep', 608, 32, 'float32'), ('pres', 640, 32, 'float32'),
        ('freq', 672, 32, 'float32'), ('lnmp', 704, 32, 'float32'),
    )),
}


def present(combo):
    return [row[0] for row in LAYOUT[combo][1]]


def inputs(n, salt):
    """n rows of distinct non-zero values for every lane (the recorded blobs were filled from the same)."""
    r = np.arange(1, n + 1)
    return {"ids": (100 * salt + r).astype(np.int64), "pos": (200 * salt + r).astype(np.int64),
            "slots": (300 * salt + r).astype(np.int64), "seeds": (2 ** 40 * salt + r).astype(np.int64),
            "ctx": (10 * salt + r).astype(np.int32), "topk": (20 * salt + r + 1).astype(np.int32),
            "bt": (1000 * salt + np.arange(1, n * MB + 1).reshape(n, MB)).astype(np.int32),
            "temp": (0.5 * salt + r / 8).astype(np.float32), "topp": (r / 16 + salt / 64).astype(np.float32),
            "pslot": (r + salt).astype(np.int32), "rep": (1 + r / 4 + salt).astype(np.float32),
            "pres": (r / 2 + salt / 4).astype(np.float32), "freq": (-r / 8 - salt).astype(np.float32),
            "cslot": (9 - r + salt).astype(np.int32), "cnout": (30 * salt + r).astype(np.int32),
            "lnmp": (-r / 3 - salt).astype(np.float32)}


def fill(buf, k, b_pad, vals, names, device_ids=False, optional=True):
    lanes = {n: vals[n] for n in names if n not in ALWAYS} if optional else {}
    buf.fill(k, b_pad, *(None if device_ids and n == "ids" else vals[n] for n in ALWAYS), **lanes)


def packed(names, vals, n, b_pad):
    """The blob packed by hand: lanes in ORDER, rows [0, n) from ``vals``, rows [n, b_pad) the pads, rows [b_pad, B)
    zero."""
    parts = []
    for name in ORDER:
        if name not in names:
            continue
        proto = inputs(1, 0)[name]
        rows = np.zeros((B,) + proto.shape[1:], dtype=proto.dtype)
        if n:
            rows[:n] = vals[name]
        rows[n:b_pad] = PADS[name]
        parts.append(rows.reshape(-1).view(np.uint8))
    return np.concatenate(parts)


@pytest.mark.parametrize("combo", COMBOS)
def test_layout(combo):
    buf = _DecodeBuffers(B, MB, CPU, 0, *combo)
    nbytes, rows = LAYOUT[combo]
    assert [l.name for l in buf.lanes] == [r[0] for r in rows]
    for name, off, size, dtype in rows:
        t = getattr(buf, name)
        assert (t.data_ptr() - buf.d.data_ptr(), t.numel() * t.element_size(), str(t.dtype)) == \
            (off, size, "torch." + dtype), name
    assert buf.d.numel() == nbytes == sum(r[2] for r in rows) == buf.h[0].numel() == buf.h[1].numel()
    assert buf.o32 == 256 and buf.of32 == dict((r[0], r[1]) for r in rows)["temp"]
    assert buf.bt.shape == (B, MB)
    for name in set(ORDER) - set(present(combo)) - {"lnmp"}:  # a disabled lane is absent; lnmp is None
        assert not hasattr(buf, name), name
    assert combo[2] or buf.lnmp is None
    assert hasattr(buf, "_logits_out") == (combo[0] or combo[1])


@pytest.mark.parametrize("combo", COMBOS)
def test_fill(combo):
    buf = _DecodeBuffers(B, MB, CPU, 0, *combo)
    names = present(combo)
    full, part = inputs(8, 1), inputs(3, 2)
    fill(buf, 0, 8, full, names)
    assert np.array_equal(buf.h[0].numpy(), packed(names, full, 8, 8))
    for name in names:
        assert (getattr(buf, name).numpy() != 0).all(), name  # the first fill left no zero anywhere
    fill(buf, 0, 8, part, names)
    want = packed(names, part, 3, 8)
    assert np.array_equal(buf.h[0].numpy(), want) and np.array_equal(buf.d.numpy(), want)
    assert not buf.h[1].numpy().any()  # the other staging set is untouched
    # the same step with the optional lanes not passed: they are all pad
    fill(buf, 0, 8, part, names, optional=False)
    for name in names:
        got = getattr(buf, name).numpy()
        if name in ALWAYS:
            assert np.array_equal(got[:3], part[name]) and (got[3:] == PADS[name]).all(), name
        else:
            assert (got == PADS[name]).all(), name
    # ids=None: the previous step's tokens, copied on the device; the host rows stay
    buf.out.copy_(torch.arange(50, 58))
    fill(buf, 0, 8, part, names, device_ids=True)
    assert buf.ids.tolist() == [50, 51, 52, 0, 0, 0, 0, 0]
    assert np.array_equal(buf.h[0].numpy(), want)
    z = part
    for bad in sorted(set(ORDER) - set(names)) + ["pen", "con", "min_p", "ids"]:
        with pytest.raises(TypeError):
            buf.fill(0, 8, *(z[n] for n in ALWAYS), **{bad: z["ctx"]})


def test_fill_below_the_largest_bucket():
    """Rows [b_pad, max_b) belong to no step of this bucket: fill leaves them alone."""
    buf = _DecodeBuffers(B, MB, CPU, 0, True, True, True)
    full, part = inputs(8, 1), inputs(2, 3)
    fill(buf, 1, 8, full, ORDER)
    fill(buf, 1, 4, part, ORDER)
    want = packed(ORDER, full, 8, 8).copy()
    new = packed(ORDER, part, 2, 4)
    for name, off, size, _ in LAYOUT[(True, True, True)][1]:
        half = size // 2
        want[off:off + half] = new[off:off + half]
    assert np.array_equal(buf.h[1].numpy(), want)


def test_fill_equals_recorded_blobs():
    """tests/golden/staging_fill.npz: the host and device blobs the buffers with hand-written offsets produced for
    three input sets. Equal byte for byte, except rep / pres / freq in padded rows, which that code left stale (a) or
    zero (b) and which now hold their pads."""
    gold = np.load(os.path.join(os.path.dirname(__file__), "golden", "staging_fill.npz"))

    def same(buf, k, tag, combo, pad_rows):
        mask = np.ones(buf.d.numel(), dtype=bool)
        for name, off, size, _ in LAYOUT[combo][1]:
            if name in ("rep", "pres", "freq"):
                lo, hi = pad_rows
                mask[off + 4 * lo:off + 4 * hi] = False
                assert (getattr(buf, name).numpy()[lo:hi] == PADS[name]).all()
        for got, key in ((buf.h[k].numpy(), tag + "_h"), (buf.d.numpy(), tag + "_d")):
            assert got.shape == gold[key].shape and np.array_equal(got[mask], gold[key][mask]), key
        return int((~mask).sum())

    # a: everything on - a full step, then 3 rows padded to 8
    combo = (True, True, True)
    buf = _DecodeBuffers(B, MB, CPU, 0, *combo)
    fill(buf, 0, 8, inputs(8, 1), ORDER)
    fill(buf, 0, 8, inputs(3, 2), ORDER)
    assert same(buf, 0, "a", combo, (3, 8)) == 3 * 5 * 4
    # b: penalties + min_p, 5 rows padded to 8 in set 1, ids copied on the device, optional lanes not passed
    combo = (True, False, True)
    buf = _DecodeBuffers(B, MB, CPU, 0, *combo)
    buf.out.copy_(torch.arange(11, 19))
    fill(buf, 1, 8, inputs(5, 3), present(combo), device_ids=True, optional=False)
    assert same(buf, 1, "b", combo, (0, 8)) == 3 * 8 * 4
    # c: constraints only, 2 rows padded to 4 of 8
    combo = (False, True, False)
    buf = _DecodeBuffers(B, MB, CPU, 0, *combo)
    fill(buf, 0, 4, inputs(2, 4), present(combo))
    assert same(buf, 0, "c", combo, (0, 0)) == 0


@pytest.mark.parametrize("combo", COMBOS)
def test_reset(combo):
    buf = _DecodeBuffers(B, MB, CPU, 0, *combo)
    fill(buf, 0, 8, inputs(8, 1), present(combo))
    buf.reset()
    for name in present(combo):
        got = getattr(buf, name)
        assert got.shape[0] == B and (got.numpy() == PADS[name]).all(), name
    assert np.array_equal(buf.d.numpy(), packed(present(combo), {}, 0, 8))
    assert {l.name: l.pad for l in LANES} == PADS and SLOT_LANES == ("pslot", "cslot")


def test_slot_pool():
    n = 6
    pool = SlotPool(n)
    rng = random.Random(3)

    def check():
        assert sorted(pool.free + list(pool.held.values())) == list(range(n))

    assert [pool.take(rid) for rid in (10, 11, 12, 13)] == [0, 1, 2, 3]
    assert pool.get(12) == 2 and pool.get(99) == -1 and pool.get(99, None) is None
    check()
    for rid in (12, 10, 13):  # released out of order: the lowest comes back first
        pool.release(rid)
        check()
    pool.release(77)  # unknown: a no-op
    pool.release(12)  # released twice: likewise
    check()
    assert [pool.take(rid) for rid in (20, 21, 22, 23, 24)] == [0, 2, 3, 4, 5]
    assert not pool.free
    with pytest.raises(IndexError):
        pool.take(25)
    assert 25 not in pool.held
    check()
    held = dict(pool.held)
    for _ in range(200):  # any order of takes and releases: always the lowest free slot, always a partition
        if pool.free and (not pool.held or rng.random() < 0.5):
            rid = rng.randrange(1000, 10 ** 6)
            low = min(pool.free)
            assert pool.take(rid) == low
            held[rid] = low
        else:
            rid = rng.choice(sorted(pool.held))
            pool.release(rid)
            del held[rid]
        assert pool.held == held
        check()


def test_engine_pools_are_the_aliased_attributes():
    cfg = get_preset("tiny-llama", hidden_size=64, num_heads=2, num_kv_heads=2, head_dim=32, rotary_dim=32,
                     intermediate_size=128, max_position_embeddings=64, num_layers=1)
    m = DecoderLM(cfg, random_weights(cfg, 1, 0, dtype=torch.float32, seed=1, std=0.05))
    eng = LLMEngine(m, max_num_seqs=4, block_size=4, num_blocks=32, penalties=True, constraints=True)
    assert eng._pen_free is eng._pen_pool.free and eng._pen_slot is eng._pen_pool.held
    assert eng._con_free is eng._con_pool.free and eng._con_slot is eng._con_pool.held
    assert eng._pen_pool is not eng._con_pool and sorted(eng._pen_free) == sorted(eng._con_free) == [0, 1, 2, 3]
    eng._pen_pool.take(5)
    eng._con_pool.take(5)
    eng._con_pool.take(6)
    assert eng._pen_slot == {5: 0} and eng._con_slot == {5: 0, 6: 1}
    eng._release_slots(5)
    eng._release_slots(7)  # holds nothing
    assert eng._pen_slot == {} and eng._con_slot == {6: 1}
    assert sorted(eng._pen_free) == [0, 1, 2, 3] and sorted(eng._con_free) == [0, 2, 3]
