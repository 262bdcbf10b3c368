"""What the engine stages per decode step and per sequence: the static buffers behind the captured decode graphs
(:class:`_DecodeBuffers`, one blob laid out from the ``LANES`` table) and the pool of per-sequence state rows the
penalties and the token constraints each keep (:class:`SlotPool`)."""
from __future__ import annotations

import heapq
from typing import Dict, List, NamedTuple

import torch


class Lane(NamedTuple):
    name: str
    dtype: torch.dtype
    pad: float  # what rows [n, b_pad) of a step hold, and every row after reset()
    when: str = ""  # the _DecodeBuffers option the lane exists with ("": always)
    cols: str = ""  # the _DecodeBuffers attribute that counts a row's columns ("": one)
    slot: bool = False  # holds a row of per-sequence state (-1: none), which a dead row must let go of


# The staging blob, in byte order: int64, int32, then fp32 lanes of max_b rows each (``bt``: max_b x max_blocks). An
# option that is off leaves its lanes out and every other offset as it is without it. Padded rows are harmless:
# ctx 0 -> zero attention, slot -1 -> no cache write, top_k 1 -> greedy; pslot / cslot -1 -> the penalty and the
# constraint launch copy the row (its rep / pres / freq / cnout are read and unused); lnmp -inf -> no floor.
I64, I32, F32 = torch.int64, torch.int32, torch.float32
LANES = (
    Lane("ids", I64, 0), Lane("pos", I64, 0), Lane("slots", I64, -1), Lane("seeds", I64, 0),
    Lane("ctx", I32, 0), Lane("topk", I32, 1), Lane("bt", I32, 0, cols="max_blocks"),
    Lane("pslot", I32, -1, "penalties", slot=True),
    Lane("cslot", I32, -1, "constraints", slot=True), Lane("cnout", I32, 0, "constraints"),
    Lane("temp", F32, 0), Lane("topp", F32, 1),
    Lane("rep", F32, 1, "penalties"), Lane("pres", F32, 0, "penalties"), Lane("freq", F32, 0, "penalties"),
    Lane("lnmp", F32, float("-inf"), "min_p"),
)
SLOT_LANES = tuple(l.name for l in LANES if l.slot)
_ALWAYS = tuple(l.name for l in LANES if not l.when)  # fill's positional arrays, in this order


class SlotPool:
    """Rows 0..n-1 of a per-sequence device state, handed to request ids. Holders are always running sequences. A
    released row may still be written or read by a decode step in flight: its next holder rebuilds it whole, later on
    the same stream."""

    def __init__(self, n: int):
        self.free: List[int] = list(range(n))  # a heap: take() returns the lowest
        self.held: Dict[int, int] = {}  # request id -> row

    def get(self, rid: int, default: int = -1) -> int:
        return self.held.get(rid, default)

    def take(self, rid: int) -> int:
        s = self.held[rid] = heapq.heappop(self.free)
        return s

    def release(self, rid: int):
        s = self.held.pop(rid, None)
        if s is not None:
            heapq.heappush(self.free, s)


class _DecodeBuffers:
    """Static device buffers feeding the captured decode graphs, filled by ONE host-to-device copy
    per step from one of two pinned staging sets: with decode steps pipelined (LLMEngine.step),
    the host fills step t+1's set while step t's copy may still be queued, so a set is rewritten
    only after the step that used it has been collected. Token ids come back through two pinned
    output buffers for the same reason. ``max_logprobs`` N > 0 adds the log-probability outputs: ``lp_f`` [max_b, 1 + N]
    fp32 (the sampled token's, then the top N) and ``lp_i`` [max_b, N] int32 (their ids) with two pinned host sets.
    Every lane of ``LANES`` that is present is an attribute, a [max_b] view of the device blob (``bt``: [max_b,
    max_blocks]); ``lnmp`` is None without ``min_p``, the lanes of ``penalties`` and ``constraints`` are absent without
    them. ``penalties`` and ``constraints`` also keep the penalised and the constrained logits, one static buffer per
    logits width (``logits_out``)."""

    def __init__(self, max_b: int, max_blocks: int, device, max_logprobs: int = 0, penalties: bool = False,
                 constraints: bool = False, min_p: bool = False):
        B = self.max_b = max_b
        self.max_blocks = max_blocks
        self.penalties = bool(penalties)
        self.constraints = bool(constraints)
        self.min_p = bool(min_p)
        pin = torch.cuda.is_available() and device.type == "cuda"
        self.lanes = tuple(l for l in LANES if not l.when or getattr(self, l.when))
        self._optional = frozenset(l.name for l in self.lanes if l.when)
        span, start, nbytes = {}, {}, 0
        for l in self.lanes:
            start.setdefault(l.dtype, nbytes)
            span[l.name] = nbytes, nbytes + B * (getattr(self, l.cols) if l.cols else 1) * l.dtype.itemsize
            nbytes = span[l.name][1]
        self.o32, self.of32 = start[I32], start[F32]  # where the int32 and the fp32 lanes begin
        self.h = [torch.zeros(nbytes, dtype=torch.uint8, pin_memory=pin) for _ in range(2)]
        self.d = torch.zeros(nbytes, dtype=torch.uint8, device=device)

        def view(blob, l):
            v = blob[slice(*span[l.name])].view(l.dtype)
            return v.view(B, -1) if l.cols else v

        self._host = [{l.name: view(h, l).numpy() for l in self.lanes} for h in self.h]
        self.lnmp = None
        for l in self.lanes:
            setattr(self, l.name, view(self.d, l))
        if self.penalties or self.constraints:
            self._logits_out = {}
        self.out = torch.zeros(max_b, dtype=torch.int64, device=device)
        self.h_out = [torch.zeros(max_b, dtype=torch.int64, pin_memory=pin) for _ in range(2)]
        N = self.max_logprobs = max_logprobs
        if N > 0:
            self.lp_f = torch.zeros(max_b, 1 + N, dtype=torch.float32, device=device)
            self.lp_i = torch.zeros(max_b, N, dtype=torch.int32, device=device)
            self.h_lp_f = [torch.zeros(max_b, 1 + N, dtype=torch.float32, pin_memory=pin) for _ in range(2)]
            self.h_lp_i = [torch.zeros(max_b, N, dtype=torch.int32, pin_memory=pin) for _ in range(2)]

    def lp_out(self, b: int):
        """The kernels' (lp, top_lp, top_ids) outputs for the first b rows, or None without log-probabilities."""
        if self.max_logprobs <= 0:
            return None
        return self.lp_f[:b, 0], self.lp_f[:b, 1:], self.lp_i[:b]

    def logits_out(self, stage: str, b: int, like: torch.Tensor) -> torch.Tensor:
        """The static buffer that stage "pen" writes the penalised copy of the [b, width] logits ``like`` to, or
        stage "con" the constrained copy - apart from each other: the penalised logits are the constraint launch's
        input. Made at the first (warm-up) call for a width and kept for the buffers' lifetime: captured graphs write
        and read it."""
        key = (stage, like.shape[1], like.dtype)
        if key not in self._logits_out:
            self._logits_out[key] = torch.zeros(self.max_b, like.shape[1], dtype=like.dtype, device=like.device)
        return self._logits_out[key][:b]

    def reset(self):
        """Every row of the device blob padded, as ahead of the graph capture's warm-up."""
        for l in self.lanes:
            getattr(self, l.name).fill_(l.pad)

    def fill(self, k, b_pad, ids, pos, slots, seeds, ctx, topk, bt, temp, topp, **lanes):
        """Stage one step's inputs in set k and copy them to the device: rows [0, n) from the arrays, rows [n, b_pad)
        padded. ``ids=None``: the input ids are the previous step's sampled tokens, copied on the device (same rows).
        ``lanes``: the optional lanes' arrays by name (``pslot``, ``rep``, ``pres``, ``freq``; ``cslot``, ``cnout``;
        ``lnmp``); one that is present and not passed is padded in all b_pad rows."""
        if not lanes.keys() <= self._optional:
            raise TypeError(f"fill() got lanes these buffers do not have: {sorted(lanes.keys() - self._optional)}")
        n = len(pos)
        host = self._host[k]
        lanes.update(zip(_ALWAYS, (ids, pos, slots, seeds, ctx, topk, bt, temp, topp)))
        for l in self.lanes:
            v, arr = host[l.name], lanes.get(l.name)
            lo = n
            if arr is None:
                lo = n if l.name == "ids" else 0
            elif v.ndim == 2:
                v[:n, :arr.shape[1]] = arr
            else:
                v[:n] = arr
            v[lo:b_pad] = l.pad
        self.d.copy_(self.h[k], non_blocking=True)
        if ids is None:
            self.ids[:n].copy_(self.out[:n])
