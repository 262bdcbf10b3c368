"""Scheduler with a sliding window (csrc/runtime.cpp): prompt chunks of at most the window, blocks below the window
given back before a step is emitted, admission against the live bound, no double free."""
import math

import pytest

from llmss_amd import _native

native = _native()
BS, W = 4, 8


def drive(s, seqs, steps=10_000, on_step=None):
    """Run until every sequence has its max_new tokens; returns the longest chunk seen."""
    left = dict(seqs)  # id -> tokens still to sample
    qmax = 0
    for _ in range(steps):
        if not s.has_work():
            break
        b = s.schedule()
        assert b.kind != 0
        qmax = max(qmax, int(b.query_lens.max()))
        if on_step:
            on_step(b)
        for i, smp in zip(b.ids.tolist(), b.sample.tolist()):
            if smp:
                left[i] -= 1
                s.on_token(i, False)
    assert not s.has_work() and all(v == 0 for v in left.values())
    return qmax


def live(s, i):
    return [x for x in s.blocks(i) if x >= 0]


@pytest.mark.parametrize("chunk", [0, 3, 5])
def test_live_blocks_stay_within_the_window(chunk):
    s = native.Scheduler(num_blocks=64, block_size=BS, max_num_seqs=4, max_batched_tokens=64, max_model_len=128,
                         prefill_chunk=chunk, window=W)
    s.add(1, 30, 40)
    s.add(2, 3, 20)
    s.add(3, 9, 9)
    peak = {}
    q_seen = [0]

    def on_step(b):
        q_seen[0] = max(q_seen[0], int(b.query_lens.max()))
        assert int(b.query_lens.max()) <= W
        tab = b.block_table
        for row, (i, q, c) in enumerate(zip(b.ids.tolist(), b.query_lens.tolist(), b.ctx_lens.tolist())):
            blocks = s.blocks(i)
            peak[i] = max(peak.get(i, 0), len(live(s, i)))
            p0 = c - q
            first = max(0, p0 - W + 1) // BS  # the page of the lowest key the step reads
            assert all(x == -1 for x in blocks[:first]) and all(x >= 0 for x in blocks[first:])
            assert len(blocks) == math.ceil(c / BS)  # the logical length stays
            assert tab[row, :first].tolist() == [0] * first  # released entries read 0 in the step's table
            assert tab[row, first:len(blocks)].tolist() == blocks[first:]
        for x in b.slots.tolist():
            assert x >= 0

    drive(s, {1: 40, 2: 20, 3: 9}, on_step=on_step)
    bound = math.ceil((W + q_seen[0]) / BS) + 2
    assert max(peak.values()) <= bound, (peak, bound)
    assert peak[1] < math.ceil(70 / BS)  # fewer than the whole sequence would hold
    assert s.num_free_blocks() == 64


def test_slots_point_into_live_blocks():
    s = native.Scheduler(16, BS, 2, 64, 128, 0, W)
    s.add(7, 20, 30)

    def on_step(b):
        blocks = s.blocks(7)
        for p, slot in zip(b.positions.tolist(), b.slots.tolist()):
            assert blocks[p // BS] >= 0 and slot == blocks[p // BS] * BS + p % BS

    drive(s, {7: 30}, on_step=on_step)


def test_small_pool_admits_a_long_windowed_sequence():
    need_all = math.ceil((30 + 60) / BS)
    pool = 8
    assert pool < need_all
    plain = native.Scheduler(pool, BS, 2, 64, 128, 0)
    with pytest.raises(ValueError, match="more KV blocks"):
        plain.add(1, 30, 60)
    s = native.Scheduler(pool, BS, 2, 64, 128, 0, W)
    s.add(1, 30, 60)
    drive(s, {1: 60})
    assert s.num_free_blocks() == pool
    tiny = native.Scheduler(3, BS, 2, 64, 128, 0, W)  # not even the window fits
    with pytest.raises(ValueError, match="more KV blocks"):
        tiny.add(1, 30, 60)


def test_pool_is_whole_after_finish_abort_preempt_and_reserve():
    pool = 12
    s = native.Scheduler(pool, BS, 4, 64, 128, 0, W)
    for i, (p, n) in enumerate([(30, 40), (17, 40), (9, 40), (26, 40)]):
        s.add(i, p, n)
    preempted = 0
    for step in range(60):
        b = s.schedule()
        preempted += len(b.preempted)
        for i, smp in zip(b.ids.tolist(), b.sample.tolist()):
            if smp and s.contains(i):
                s.on_token(i, False)
        if step == 20:
            s.abort(1)
        if step == 30:
            s.finish(2)
        if step % 3 == 0:  # the pipelined decode's block ahead of schedule(): releases before it grows
            for i in (0, 3):
                if s.contains(i) and s.num_computed(i) == s.num_tokens(i) - 1 and s.num_computed(i) > 0:
                    n = s.num_tokens(i)
                    blk = s.reserve(i, n)
                    if blk >= 0:
                        blocks = s.blocks(i)
                        assert blocks[(n - 1) // BS] == blk
                        assert all(x == -1 for x in blocks[:max(0, n - 1 - W + 1) // BS])
        used = sum(len(live(s, i)) for i in range(4) if s.contains(i))
        assert used + s.num_free_blocks() == pool  # nothing lost, nothing freed twice
    assert preempted > 0, "the pool was meant to force a preemption"
    for i in range(4):
        s.abort(i)
    assert s.num_free_blocks() == pool


def test_whole_prompt_mode_rejects_a_prompt_longer_than_the_window():
    s = native.Scheduler(64, BS, 4, 64, 128, -1, W)
    s.add(1, W, 4)
    with pytest.raises(ValueError, match="window"):
        s.add(2, W + 1, 4)
    # a preempted sequence recomputing more than a window is chunked after all
    drive(s, {1: 4})
    assert s.num_free_blocks() == 64


def test_window_zero_is_the_plain_scheduler():
    a = native.Scheduler(32, BS, 4, 16, 64, 0)
    b = native.Scheduler(32, BS, 4, 16, 64, 0, 0)
    for s in (a, b):
        s.add(1, 21, 10)
        s.add(2, 5, 10)
    for _ in range(40):
        if not a.has_work():
            break
        x, y = a.schedule(), b.schedule()
        assert x.kind == y.kind and x.slots.tolist() == y.slots.tolist()
        assert x.block_table.tolist() == y.block_table.tolist()
        for s, st in ((a, x), (b, y)):
            for i, smp in zip(st.ids.tolist(), st.sample.tolist()):
                if smp:
                    s.on_token(i, False)
    assert not a.has_work() and not b.has_work()
