"""Validated launchers for the gfx950 kernels in ``llmss_amd/csrc`` (module ``llmss_amd._C``).

Every wrapper checks dtype, device, contiguity/strides and the shape relations the kernel grid
assumes *before* launching, so a malformed call raises here instead of faulting the GPU.
Kernels run on the caller's current HIP stream (``torch.cuda.current_stream()``), which makes
them capturable into HIP graphs together with RCCL collectives.
"""
from __future__ import annotations

import math
import os
import threading
import weakref
from typing import Optional

import torch

from . import plans
from . import reference as _ref

_C = None
_ERR = None


def lib():
    """The native module; raises loudly if it is missing (no silent eager fallback on GPU)."""
    global _C, _ERR
    if _C is None:
        try:
            from .. import _native
            _C = _native()
        except Exception as e:  # pragma: no cover - exercised only on broken installs
            _ERR = e
            raise RuntimeError(
                "llmss_amd._C is not available: run `python -m llmss_amd._build` (hipcc --offload-arch=gfx950)"
            ) from e
    return _C


def _stream() -> int:
    return torch.cuda.current_stream().cuda_stream


def _ptr(t: Optional[torch.Tensor]) -> int:
    return 0 if t is None else t.data_ptr()


def _check(cond: bool, msg: str):
    if not cond:
        raise ValueError(msg)


def _bf16_rows(t: torch.Tensor, name: str, cols: Optional[int] = None):
    _check(t.is_cuda, f"{name} must be on the GPU")
    # kernels launch on the CURRENT device's stream: a tensor of another device would be addressed
    # through the wrong GPU's page tables
    _check(t.device.index == torch.cuda.current_device(),
           f"{name} is on {t.device} but the current device is cuda:{torch.cuda.current_device()}")
    _check(t.dtype == torch.bfloat16, f"{name} must be bfloat16, got {t.dtype}")
    _check(t.dim() == 2, f"{name} must be 2-D")
    _check(t.stride(1) == 1, f"{name} rows must be contiguous")
    _check(t.data_ptr() % 16 == 0 and (t.stride(0) * 2) % 16 == 0, f"{name} must be 16-byte aligned")
    if cols is not None:
        _check(t.shape[1] == cols, f"{name} has {t.shape[1]} columns, expected {cols}")


# ------------------------------------------------------------------------------------- norm
def _fp8_twin(y):
    """Scratch for the per-token fp8 twin of add_norm's output ``y`` [T, H], registered for its W8A8 consumer."""
    T, H = y.shape
    q, s = _PRESCRATCH.get(T, H, y.device)
    _PREQ.clear()  # one live twin at a time: the previous one's consumer has run (same stream, program order)
    _PREQ[id(y)] = (weakref.ref(y), q, s)
    return q, s


def add_norm(x, weight, bias, eps, rms, residual=None, out=None, residual_out=None, fp8_out=False):
    """``fp8_out``: also write the per-token fp8-e4m3 twin of the output (== quant_fp8_rows of it) for the W8A8
    GEMM that consumes it next, which then skips its own quantisation launch."""
    if isinstance(x, PartialSum):
        return add_norm_partial(x, weight, bias, eps, rms, residual, out, fp8_out=fp8_out)
    xcw = 0
    if x.dim() == 3:  # column-chunked [C, T, CW] (DecoderLM._reduce_cols): row t is x[:, t, :] concatenated
        _check(x.is_contiguous() and x.dtype == torch.bfloat16 and x.shape[2] % 8 == 0, "chunked x [C, T, CW]")
        C, T, xcw = x.shape
        H = C * xcw
    else:
        T, H = x.shape
        _bf16_rows(x, "x")
    _check(H % 8 == 0, "hidden must be a multiple of 8")
    _check(weight.is_contiguous() and weight.numel() == H and weight.dtype == torch.bfloat16, "norm weight")
    if bias is not None:
        _check(bias.is_contiguous() and bias.numel() == H and bias.dtype == torch.bfloat16, "norm bias")
    y = out if out is not None else torch.empty(T, H, dtype=x.dtype, device=x.device)
    _bf16_rows(y, "out", H)
    if residual is not None:
        _check(residual.is_contiguous() and residual.shape == (T, H) and residual.dtype == torch.bfloat16, "residual")
        ro = residual_out if residual_out is not None else residual
        _check(ro.is_contiguous() and ro.shape == (T, H), "residual_out")
    else:
        ro = None
    if residual is None and xcw:  # checked before the launch: an invalid call queues no GPU work
        raise ValueError("a column-chunked add_norm input needs a residual (its residual output is row-major)")
    q8, s8 = _fp8_twin(y) if fp8_out else (None, None)
    lib().add_norm(x.data_ptr(), x.stride(0) if not xcw else xcw, _ptr(residual), _ptr(ro), weight.data_ptr(),
                   _ptr(bias), y.data_ptr(), y.stride(0), T, H, float(eps), bool(rms), _stream(), _ptr(q8), _ptr(s8),
                   xcw)
    return y, (ro if residual is not None else x)


# ------------------------------------------------------------------------------------ embed
def embed(ids, wte, positions=None, wpe=None, out=None):
    T = ids.numel()
    V, H = wte.shape
    _check(ids.dtype == torch.int64 and ids.is_contiguous() and ids.is_cuda, "ids must be contiguous int64 cuda")
    _bf16_rows(wte, "wte")
    _check(wte.is_contiguous(), "wte contiguous")
    if wpe is not None:
        _check(positions is not None and positions.dtype == torch.int64 and positions.numel() == T, "positions")
        _check(wpe.is_contiguous() and wpe.shape[1] == H and wpe.dtype == torch.bfloat16, "wpe")
    y = out if out is not None else torch.empty(T, H, dtype=wte.dtype, device=wte.device)
    lib().embed(ids.data_ptr(), _ptr(positions), wte.data_ptr(), _ptr(wpe), y.data_ptr(), T, H, V, _stream())
    return y


# ------------------------------------------------------------------------------ rope + cache
def rope_cache(qkv, positions, cos, sin, k_cache, v_cache, slots, nh, nkv, D, rot, style, do_rope=True):
    """Rotate q/k in place and write k/v to the paged cache; returns the bf16 qkv tensor.

    ``qkv`` may be a :class:`PartialSum` (split-K slabs of the QKV GEMM): the kernel then sums the
    slabs (+ bias) itself and writes the finished rows into a fresh bf16 qkv tensor.
    """
    part = qkv if isinstance(qkv, PartialSum) else None
    if part is not None:
        _check(part.N == (nh + 2 * nkv) * D, "partial qkv width")
        qkv = torch.empty(part.M, part.N, dtype=torch.bfloat16, device=part.device)
    T = qkv.shape[0]
    _bf16_rows(qkv, "qkv")
    _check(qkv.shape[1] >= (nh + 2 * nkv) * D, "qkv too narrow")
    _check(D % 8 == 0 and rot <= D and (not do_rope or rot % 8 == 0), "head_dim / rotary_dim (multiple of 8)")
    _check(positions.dtype == torch.int64 and positions.numel() == T and positions.is_contiguous(), "positions")
    if do_rope and rot > 0:
        _check(cos.dtype == torch.float32 and cos.is_contiguous() and cos.shape[1] == rot // 2, "cos table")
        _check(sin.shape == cos.shape and sin.is_contiguous(), "sin table")
    kv8 = k_cache is not None and k_cache.dtype == torch.uint8
    if k_cache is not None:
        _kv_cache_check(k_cache, v_cache, nkv, D)
        _check(slots is not None and slots.dtype == torch.int64 and slots.numel() == T, "slots")
        bs = k_cache.shape[2]
    else:
        bs = 1
    lib().rope_cache(qkv.data_ptr(), qkv.stride(0), positions.data_ptr(), _ptr(cos) if do_rope else 0,
                     _ptr(sin) if do_rope else 0, _ptr(k_cache), _ptr(v_cache),
                     _ptr(slots) if k_cache is not None else 0, T, nh, nkv, D, rot,
                     bs, nh * D, (nh + nkv) * D, 1 if style == "gptj" else 0, bool(do_rope and rot > 0),
                     part.buf.data_ptr() if part else 0, part.S if part else 0, part.M * part.N if part else 0,
                     _ptr(part.bias) if part else 0, _stream(), kv8)
    return qkv


def _kv_cache_check(k_cache, v_cache, nkv, D):
    """bf16 [nb, nkv, bs, D] caches, or fp8 rows [nb, nkv, bs, D + 16] uint8 (ops/reference.py kv_rows_quant)."""
    kv8 = k_cache.dtype == torch.uint8
    _check(k_cache.is_cuda and k_cache.dtype in (torch.bfloat16, torch.uint8) and k_cache.is_contiguous()
           and k_cache.dim() == 4, "k_cache bf16 / uint8 (fp8 rows) [nb, nkv, bs, row]")
    _check(k_cache.shape[1] == nkv and k_cache.shape[3] == (D + _ref.KV8_TAIL if kv8 else D),
           f"k_cache shape [nb, nkv, bs, {'D + 16' if kv8 else 'D'}]")
    _check(v_cache.shape == k_cache.shape and v_cache.dtype == k_cache.dtype and v_cache.is_contiguous(), "v_cache")
    if kv8:
        _check(D % 16 == 0 and 256 % (D // 8) == 0, "fp8 KV cache needs head_dim 64/128/256")
    return kv8


# -------------------------------------------------------------------------------- attention
def attn_prefill(qkv, cu_seqlens, max_seqlen, nh, nkv, D, scale, out=None):
    T = qkv.shape[0]
    _bf16_rows(qkv, "qkv")
    _check(qkv.shape[1] >= (nh + 2 * nkv) * D, "qkv too narrow")
    _check(D in (64, 128, 256), "prefill attention supports head_dim 64/128/256")
    _check(cu_seqlens.dtype == torch.int32 and cu_seqlens.is_contiguous() and cu_seqlens.is_cuda, "cu_seqlens int32")
    B = cu_seqlens.numel() - 1
    y = out if out is not None else torch.empty(T, nh * D, dtype=qkv.dtype, device=qkv.device)
    _bf16_rows(y, "out")
    _check(qkv.stride(0) % 8 == 0 and qkv.data_ptr() % 16 == 0, "qkv rows 16-B aligned")
    lib().attn_prefill(qkv.data_ptr(), qkv.stride(0), T, cu_seqlens.data_ptr(), y.data_ptr(), y.stride(0), B,
                       int(max_seqlen), nh, nkv, D, nh * D, (nh + nkv) * D, float(scale), _stream())
    return y


def extend_fp8_twin_ok(nh: int, nkv: int) -> bool:
    """Can attn_extend write the per-token fp8 twin of its output in the same launch (every head of a row in
    one workgroup: one kv head, a power-of-two query group <= 16)?"""
    G = nh // nkv
    return nkv == 1 and G <= 16 and G & (G - 1) == 0


def _kv_starts_check(kv_starts, B: int, window: int) -> int:
    """``kv_starts`` [>= B] int32 (the first key a sequence may attend) is validated like ``ctx_lens``."""
    _check(int(window) >= 0, "window must be >= 0")
    if kv_starts is None:
        return 0
    _check(kv_starts.dtype == torch.int32 and kv_starts.is_contiguous() and kv_starts.is_cuda
           and kv_starts.numel() >= B, "kv_starts must be contiguous int32 cuda with >= B entries")
    _check(kv_starts.device.index == torch.cuda.current_device(), "kv_starts on the current device")
    return kv_starts.data_ptr()


def attn_extend(q, k_cache, v_cache, block_tables, cu_q, ctx_lens, max_qlen, nh, nkv, D, scale, out=None,
                fp8_out=False, window=0, kv_starts=None):
    """Chunked-prefill attention: q rows [T, >= nh*D] (query heads first, as in the QKV output) of B
    sequences (``cu_q`` [B+1] int32), each attending its whole paged context ``ctx_lens`` [B] int32 (the
    chunk's own K/V already written to the cache) causally. ``fp8_out`` (only where extend_fp8_twin_ok):
    also write the output's per-token fp8 twin for the W8A8 o-projection, which then skips its quantisation
    launch. ``window`` (0 = unlimited) / ``kv_starts`` [B] int32: the row at position p attends keys
    ``[max(kv_starts[b], p - window + 1), p]``; nothing below that range's first page is read from the table."""
    T = q.shape[0]
    _bf16_rows(q, "q")
    _check(q.shape[1] >= nh * D, "q too narrow")
    _check(D in (64, 128, 256), "extend attention supports head_dim 64/128/256")
    kv8 = _kv_cache_check(k_cache, v_cache, nkv, D)
    _check(nh % nkv == 0, "nh % nkv")
    B = cu_q.numel() - 1
    for t, nm in ((cu_q, "cu_q"), (ctx_lens, "ctx_lens"), (block_tables, "block_tables")):
        _check(t.dtype == torch.int32 and t.is_contiguous() and t.is_cuda, f"{nm} must be contiguous int32 cuda")
    _check(ctx_lens.numel() == B and block_tables.dim() == 2 and block_tables.shape[0] >= B, "batch sizes")
    bs = k_cache.shape[2]
    _check(block_tables.shape[1] * bs >= 1, "block table width")
    y = out if out is not None else torch.empty(T, nh * D, dtype=q.dtype, device=q.device)
    _bf16_rows(y, "out")
    _check(y.shape[0] >= T and y.shape[1] >= nh * D, "out shape")
    kvs = _kv_starts_check(kv_starts, B, window)
    q8 = s8 = None
    if fp8_out:
        _check(extend_fp8_twin_ok(nh, nkv) and y.shape == (T, nh * D), "fp8 twin: one kv head, group <= 16, dense out")
        q8, s8 = _fp8_twin(y)
    lib().attn_extend(q.data_ptr(), q.stride(0), k_cache.data_ptr(), v_cache.data_ptr(), block_tables.data_ptr(),
                      block_tables.shape[1], cu_q.data_ptr(), ctx_lens.data_ptr(), y.data_ptr(), y.stride(0), B,
                      int(max_qlen), nh, nkv, D, bs, float(scale), _stream(), kv8, _ptr(q8), _ptr(s8),
                      int(window), kvs)
    return y


def ce_loss_rows(logits, labels, vocab=None):
    """Per-row cross-entropy ``logsumexp(logits[t, :V]) - logits[t, label[t]]`` (0 where label < 0);
    ``logits`` [T, >= V] bf16 or fp32 rows, ``labels`` [T] int64."""
    T = logits.shape[0]
    V = int(vocab or logits.shape[1])
    _check(logits.is_cuda and logits.dim() == 2 and logits.stride(1) == 1, "logits [T, V] rows on the GPU")
    _check(logits.device.index == torch.cuda.current_device(), "logits on the current device")
    _check(logits.dtype in (torch.bfloat16, torch.float32), "logits must be bf16 or fp32")
    _check(logits.stride(0) % 8 == 0 and logits.data_ptr() % 16 == 0, "logits rows 16-B aligned")
    _check(V <= logits.shape[1], "vocab exceeds the row width")
    _check(labels.dtype == torch.int64 and labels.is_cuda and labels.numel() == T and labels.is_contiguous(),
           "labels [T] int64")
    loss = torch.empty(T, dtype=torch.float32, device=logits.device)
    lib().ce_loss(logits.data_ptr(), logits.stride(0), logits.dtype == torch.float32, labels.data_ptr(), T, V,
                  loss.data_ptr(), _stream())
    return loss


class DecodeWorkspace:
    """Split-K partial buffers for decode attention (allocated once; graph-capture safe)."""

    def __init__(self):
        self.po = None
        self.pml = None

    def get(self, B, nh, nsplit, D, device):
        need = B * nh * nsplit
        if (self.po is None or self.po.numel() < need * D or self.pml.numel() < need * 2
                or self.po.device != _dev(device)):
            if torch.cuda.is_current_stream_capturing():
                raise RuntimeError("decode workspace must be allocated before graph capture")
            n_o = max(need * D, 0 if self.po is None else 2 * self.po.numel())  # geometric: few retired buffers
            n_ml = max(need * 2, 0 if self.pml is None else 2 * self.pml.numel())
            _retire(self.po, self.pml)
            self.po = torch.empty(n_o, dtype=torch.float32, device=device)
            self.pml = torch.empty(n_ml, dtype=torch.float32, device=device)
        return self.po, self.pml


class _Slotted:
    """One instance of a scratch / workspace class per workspace slot (``workspace_slot``): kernels of chains
    that may run concurrently on different streams never share a buffer."""

    def __init__(self, cls):
        self._items = [cls() for _ in range(4)]

    def __getattr__(self, name):
        return getattr(self._items[getattr(_SLOT, "k", 0)], name)


_SLOT = threading.local()  # per host thread, like the native slot (csrc/gemm.hip gemm_set_slot)

# Scratch buffers outgrown by a later (eager) call are kept, never freed: a decode graph captured earlier still
# writes to the old addresses on every replay, and a freed block would go back to the caching allocator and be
# handed to live tensors (the native counters do the same, csrc/gemm.hip sk_counters).
_RETIRED: list = []


def _retire(*ts):
    _RETIRED.extend(t for t in ts if t is not None)


def _dev(device) -> torch.device:
    """``device`` as tensors report it ("cuda" -> "cuda:<current>"): a scratch buffer is reused only on its own device,
    and an unindexed name must not look like another device (every call would grow the buffer again)."""
    d = torch.device(device)
    if d.type == "cuda" and d.index is None:
        d = torch.device("cuda", torch.cuda.current_device())
    return d


class workspace_slot:
    """``with workspace_slot(k):`` ops issued inside use workspace slot k (GEMM workspace / combine counters,
    decode-attention partials, fp8 scratch) - for a chain that runs concurrently with slot 0's on another
    stream. Host-side state at launch (and capture) time."""

    def __init__(self, k: int):
        self.k = int(k) & 3

    def __enter__(self):
        self.prev = getattr(_SLOT, "k", 0)
        _SLOT.k = self.k
        lib().gemm_set_slot(self.k)
        return self

    def __exit__(self, *exc):
        _SLOT.k = self.prev
        lib().gemm_set_slot(self.prev)
        return False


_DECODE_WS = _Slotted(DecodeWorkspace)


def decode_span(max_ctx: int, block_size: int, window: int = 0) -> int:
    """Keys the decode partitions have to cover: a windowed row reads ``[lo, ctx)`` and its partitions start at
    lo's page, so at most ``window + block_size`` keys however long the context is."""
    return min(max_ctx, window + block_size) if window > 0 else max_ctx


def decode_splits(B: int, nkv: int, max_ctx: int, block_size: int) -> tuple:
    """(num_splits, partition_size): ~8 workgroups per CU (2048), partitions >= 256 tokens. ``max_ctx`` is the
    span to cover (:func:`decode_span` for a windowed call).

    Measured (bench/attn_bench.py): with few (sequence, kv-head) pairs - GQA / TP-sharded kv heads -
    each workgroup otherwise walks the whole context serially and the KV stream drops to 2-3 TB/s."""
    wgs = max(1, B * nkv)
    want = max(1, math.ceil(2048 / wgs))
    nsplit = max(1, min(want, math.ceil(max_ctx / 256)))
    psize = math.ceil(max_ctx / nsplit)
    psize = math.ceil(psize / block_size) * block_size
    nsplit = math.ceil(max_ctx / psize)
    return nsplit, psize


def attn_decode(q, k_cache, v_cache, block_tables, ctx_lens, nh, nkv, D, scale, max_ctx, out=None, splits=None,
                window=0, kv_starts=None):
    """``window`` (0 = unlimited) / ``kv_starts`` [B] int32: row b attends keys ``[lo, ctx_b)`` with
    ``lo = max(kv_starts[b], ctx_b - window)``; the splits are laid from lo's page and cover :func:`decode_span`."""
    B = q.shape[0]
    _check(q.is_cuda and q.dtype == torch.bfloat16 and q.stride(-1) == 1 and q.dim() == 2, "q [B, >=nh*D]")
    _check(q.shape[1] >= nh * D, "q too narrow")
    _check(D in (64, 128, 256), "decode attention supports head_dim 64/128/256")
    kv8 = _kv_cache_check(k_cache, v_cache, nkv, D)
    _check(block_tables.dtype == torch.int32 and block_tables.dim() == 2 and block_tables.shape[0] >= B
           and block_tables.stride(1) == 1, "block_tables int32 [B, maxb]")
    _check(ctx_lens.dtype == torch.int32 and ctx_lens.numel() >= B and ctx_lens.is_contiguous(), "ctx_lens int32")
    bs = k_cache.shape[2]
    _check(block_tables.shape[1] * bs >= max_ctx, "block table too short for max_ctx")
    kvs = _kv_starts_check(kv_starts, B, window)
    span = decode_span(max_ctx, bs, int(window))
    nsplit, psize = splits if splits is not None else decode_splits(B, nkv, span, bs)
    _check(nsplit >= 1 and psize >= 1 and nsplit * psize >= span, "splits do not cover max_ctx")
    y = out if out is not None else torch.empty(B, nh * D, dtype=q.dtype, device=q.device)
    _bf16_rows(y, "out")
    _check(y.shape[0] >= B and y.shape[1] >= nh * D, "out shape")
    po, pml = _DECODE_WS.get(B, nh, nsplit, D, q.device) if nsplit > 1 else (None, None)
    lib().attn_decode(q.data_ptr(), q.stride(0), k_cache.data_ptr(), v_cache.data_ptr(), block_tables.data_ptr(),
                      block_tables.stride(0), ctx_lens.data_ptr(), y.data_ptr(), y.stride(0), _ptr(po), _ptr(pml),
                      B, nh, nkv, D, bs, nsplit, psize, float(scale), _stream(), kv8, int(window), kvs)
    return y


# ------------------------------------------------------------------------------------- GEMM
class GemmWorkspace:
    def __init__(self):
        self.buf = None

    def get(self, nbytes, device):
        if self.buf is None or self.buf.numel() * 4 < nbytes or self.buf.device != _dev(device):
            if torch.cuda.is_current_stream_capturing():
                raise RuntimeError("gemm workspace must be allocated before graph capture")
            _retire(self.buf)
            self.buf = torch.empty((max(nbytes, 1 << 20) + 3) // 4, dtype=torch.float32, device=device)
        return self.buf


_GEMM_WS = _Slotted(GemmWorkspace)


def reserve_workspace(device, gemm_bytes: int = 64 << 20, decode_rows: int = 0, nh: int = 0, D: int = 128,
                      nsplit: int = 1):
    _GEMM_WS.get(gemm_bytes, device)
    lib().gemm_reserve_streamk(1 << 16)  # per-tile counters of the in-launch split-K combines
    if decode_rows and nsplit > 1:
        _DECODE_WS.get(decode_rows, nh, nsplit, D, device)


_ACT = {"none": 0, None: 0, "gelu_tanh": 1, "gelu": 2, "relu": 3}


class PartialSum:
    """fp32 split-K partial slabs [S, M, N] of a GEMM left in the GEMM workspace; consumed (summed +
    bias) by the next add_norm. Valid only until the next GEMM on the stream."""

    __slots__ = ("buf", "S", "M", "N", "bias", "dtype", "device")

    def __init__(self, buf, S, M, N, bias, device):
        self.buf, self.S, self.M, self.N, self.bias, self.device = buf, S, M, N, bias, device
        self.dtype = torch.bfloat16

    @property
    def shape(self):
        return (self.M, self.N)

    @property
    def is_cuda(self):
        return True


_FP8_PREFILL_M = 128  # untuned fp8 calls above this M run W8A8 (compute-bound); below, W8A16 weight streaming

# the hint fields are named in ops/plans.py; these are its names as tests and callers import them from here
W8A8_FLAG, W8A8_ILV, PACKED_HINT, MID_TILE_BN = plans.W8A8, plans.ILV, plans.PACKED, plans.MID_TILE_BN


class _QuantScratch:
    """Per-token fp8 activations + scales for W8A8 calls: one buffer reused by every call on the stream (each
    GEMM consumes it before the next quantisation), grown only outside graph capture, so a captured decode
    step quantises into the same addresses on every replay."""

    def __init__(self):
        self.q = None
        self.s = None

    def get(self, M, K, device):
        if self.q is None or self.q.numel() < M * K or self.s.numel() < M or self.q.device != _dev(device):
            if torch.cuda.is_current_stream_capturing():
                raise RuntimeError(f"fp8 activation scratch for [{M}, {K}] must be allocated before graph capture")
            nq = max(M * K, 0 if self.q is None else 2 * self.q.numel())  # geometric: few retired buffers
            ns = max(M, 0 if self.s is None else 2 * self.s.numel())
            _retire(self.q, self.s)
            self.q = torch.empty(nq, dtype=torch.uint8, device=device)
            self.s = torch.empty(ns, dtype=torch.float32, device=device)
        return self.q[:M * K].view(M, K), self.s[:M]


_QSCRATCH = _Slotted(_QuantScratch)


class MxAct:
    """MX-fp8 activations (OCP MX): e4m3 bytes ``q`` [M, K] and one e8m0 scale per row and 32 columns ``s``
    [M, K / 32]. What a W8A8 gate/up GEMM writes for its down projection (``linear(..., mx_out=True)``), consumed by
    ``linear`` like a bf16 input."""

    __slots__ = ("q", "s")

    def __init__(self, q, s):
        self.q, self.s = q, s

    @property
    def shape(self):
        return self.q.shape

    @property
    def is_cuda(self):
        return self.q.is_cuda


class _MxScratch:
    """The MX-fp8 SwiGLU output (one per stream slot, reused by every layer: the down projection consumes it before
    the next gate/up writes it), grown only outside graph capture."""

    def __init__(self):
        self.q = self.s = None

    def get(self, M, K, device):
        if self.q is None or self.q.numel() < M * K or self.q.device != _dev(device):
            if torch.cuda.is_current_stream_capturing():
                raise RuntimeError(f"MX-fp8 activation scratch for [{M}, {K}] must be allocated before graph capture")
            n = max(M * K, 0 if self.q is None else 2 * self.q.numel())  # geometric: few retired buffers
            _retire(self.q, self.s)
            self.q = torch.empty(n, dtype=torch.uint8, device=device)
            self.s = torch.empty(n // 32, dtype=torch.uint8, device=device)
        return self.q[:M * K].view(M, K), self.s[:M * K // 32].view(M, K // 32)


_MXSCRATCH = _Slotted(_MxScratch)


def _w8a8_mid(nt) -> bool:
    """``nt`` is a W8A8 plan on a gemm_mid tile (the MX-capable kernels)."""
    h = plans.decode(nt)
    return h.w8a8 and h.tile in MID_TILE_BN


def _w8a8_mid_plan(M, N, K, glu):
    """The tuned W8A8 plan of this shape when it runs a gemm_mid tile (the MX-capable kernels), else None."""
    tuned = lib().gemm_tuned_get(M, N, K, bool(glu), 1)
    return tuned if tuned is not None and _w8a8_mid(tuned[0]) else None


def mx_mlp_ok(M: int, up, down) -> bool:
    """The gate/up SwiGLU GEMM can write its output as MX-fp8 for the down projection (VERDICT r5 missing #4: no bf16
    intermediate, no per-token quantisation launch): both run tuned W8A8 gemm_mid plans at M rows, the gate/up plan is
    unsplit with whole 32-output blocks per tile (BN % 64 == 0)."""
    if up.w_scale is None or down.w_scale is None or not up.glu or up.N % 128 or down.K % 128 or up.N // 2 != down.K:
        return False
    pu, pd = _w8a8_mid_plan(M, up.N, up.K, True), _w8a8_mid_plan(M, down.N, down.K, False)
    return bool(pu and pd and pu[1] == 1 and MID_TILE_BN[plans.decode(pu[0]).tile] % 64 == 0)


def linear_w8a8(x, wq, w_scale, bias=None, act="none", glu=False, out=None, tile=0, depth=0, split=0,
                partial_ok=False, ilv=False, mx_out=False):
    """Y = (fp8(x) . wq^T) * x_scale[m] * w_scale[n] on the MX-fp8 MFMA (2x the bf16 matrix rate). The
    activations are quantised per token into a reusable scratch (graph-capturable). ``partial_ok``: a split
    plan may return its fp32 slabs as a :class:`PartialSum` for the consumer (rope_cache / add_norm).
    ``x`` may be an :class:`MxAct` (per-32 block scales, gemm_mid tiles); ``mx_out`` (SwiGLU, gemm_mid tile with
    BN % 64 == 0, no split) returns the output as an :class:`MxAct` instead of bf16."""
    mx_in = isinstance(x, MxAct)
    M, K = x.shape
    N = wq.shape[0]
    if mx_in:
        _check(x.q.dtype == torch.uint8 and x.q.is_contiguous() and x.s.is_contiguous() and x.s.numel() == M * K // 32,
               "MX activations: q [M, K] uint8, s [M, K / 32] uint8")
    else:
        _bf16_rows(x, "x")
    _check(wq.dtype == torch.uint8 and wq.is_contiguous() and K % 16 == 0 and wq.shape[1] == K, "fp8 weight")
    _check(w_scale.dtype == torch.float32 and w_scale.numel() == N, "w_scale [N] fp32")
    if glu:
        _check(N % 32 == 0, "glu needs N % 32 == 0")
    if bias is not None:
        _check(bias.dtype == torch.bfloat16 and bias.is_contiguous() and bias.numel() == N, "bias [N] bf16")
    dev = x.q.device if mx_in else x.device
    xs = None
    if mx_in:
        xq = x.q
    else:
        pre = _prequant_of(x)
        if pre is not None:  # add_norm already wrote this tensor's per-token fp8 twin
            xq, xs = pre
        else:
            xq, xs = _QSCRATCH.get(M, K, dev)
            lib().quant_fp8_rows_ld(x.data_ptr(), x.stride(0), xq.data_ptr(), xs.data_ptr(), M, K, _stream())
    nout = N // 2 if glu else N
    ws = _GEMM_WS.get(64 << 20, dev)
    if mx_out:
        _check(glu and out is None and not partial_ok, "MX-fp8 output: SwiGLU, no out buffer, no partial output")
        mq, ms = _MXSCRATCH.get(M, nout, dev)
        lib().gemm_f8f8(xq.data_ptr(), K, _ptr(xs), wq.data_ptr(), K, w_scale.data_ptr(), _ptr(bias), 0, nout, M, N,
                        K, _ACT[act], True, int(tile), int(depth), int(split), ws.data_ptr(), ws.numel() * 4,
                        _stream(), False, bool(ilv), mq.data_ptr(), ms.data_ptr(), 0)
        return MxAct(mq, ms)
    slabs = 0
    if partial_ok and out is None and not glu and act in ("none", None):
        slabs = lib().gemm_f8f8_partial_slabs(M, N, K, bool(glu), 0, int(tile), int(split), ws.numel() * 4)
    y = None if slabs else (out if out is not None else torch.empty(M, nout, dtype=torch.bfloat16, device=dev))
    if y is not None:
        _bf16_rows(y, "out", nout)
    S = lib().gemm_f8f8(xq.data_ptr(), K, _ptr(xs), wq.data_ptr(), K, w_scale.data_ptr(), _ptr(bias), _ptr(y),
                        y.stride(0) if y is not None else nout, M, N, K, _ACT[act], bool(glu), int(tile), int(depth),
                        int(split), ws.data_ptr(), ws.numel() * 4, _stream(), y is None, bool(ilv), 0, 0,
                        x.s.data_ptr() if mx_in else 0)
    if y is None:
        if S <= 1:
            raise RuntimeError("internal: partial W8A8 GEMM did not produce partial slabs")
        return PartialSum(ws, S, M, N, bias, dev)
    return y


# per-token fp8 twins written by add_norm(..., fp8_out=True) for the W8A8 GEMM that consumes the same tensor
# next (its own quantisation launch is then skipped): id(tensor) -> (weakref, q, s). The weakref makes a
# freed (and possibly address-reused) tensor miss; entries die with their tensor.
_PREQ = {}


class _PreQScratch:
    """Separate from _QSCRATCH: between add_norm and its consumer another W8A8 call may quantise into that."""

    def __init__(self):
        self.q = self.s = None

    def get(self, M, K, device):
        if self.q is None or self.q.numel() < M * K or self.s.numel() < M or self.q.device != _dev(device):
            if torch.cuda.is_current_stream_capturing():
                raise RuntimeError(f"fp8 norm-output scratch for [{M}, {K}] must be allocated before graph capture")
            _retire(self.q, self.s)
            nq = max(M * K, 0 if self.q is None else 2 * self.q.numel())  # geometric: few retired buffers
            ns = max(M, 0 if self.s is None else 2 * self.s.numel())
            self.q = torch.empty(nq, dtype=torch.uint8, device=device)
            self.s = torch.empty(ns, dtype=torch.float32, device=device)
        return self.q[:M * K].view(M, K), self.s[:M]


_PRESCRATCH = _Slotted(_PreQScratch)


def _prequant_of(x):
    e = _PREQ.get(id(x))
    if e is None or e[0]() is not x:
        return None
    return e[1], e[2]


def dequant_fp8_rows(q, scale, out=None):
    N, K = q.shape
    _check(q.dtype == torch.uint8 and q.is_contiguous() and K % 8 == 0, "fp8 weight [N, K] uint8, K % 8 == 0")
    _check(scale.dtype == torch.float32 and scale.numel() == N and scale.is_contiguous(), "scale [N] fp32")
    w = out if out is not None else torch.empty(N, K, dtype=torch.bfloat16, device=q.device)
    lib().dequant_fp8_rows(q.data_ptr(), scale.data_ptr(), w.data_ptr(), N, K, _stream())
    return w


def pack_panels(w, out=None):
    """Panel-packed copy ``[ceil(N/16)][ceil(K/64)][16][64]`` of a row-major bf16 ``[N, K]`` weight of any row stride,
    zeros past N and K (csrc/pack.hip; bit-equal to ``reference.pack_panels``): what a plan with :data:`PACKED_HINT`
    reads. Made once per weight; the decode GEMMs at M <= 64 stream it at the full HBM rate."""
    _check(w.is_cuda and w.device.index == torch.cuda.current_device(), "w must be on the current GPU")
    _check(w.dtype == torch.bfloat16 and w.dim() == 2 and w.stride(1) == 1 and w.stride(0) >= w.shape[1],
           "w must be bf16 [N, K] with contiguous rows")
    N, K = w.shape
    shape = (-(-N // 16), -(-K // 64), 16, 64)
    if out is None:
        out = torch.empty(shape, dtype=torch.bfloat16, device=w.device)
    _check(tuple(out.shape) == shape and out.dtype == torch.bfloat16 and out.is_contiguous() and out.device == w.device,
           f"out must be a contiguous bf16 {shape}")
    lib().pack_panels(w.data_ptr(), w.stride(0), out.data_ptr(), N, K, _stream())
    return out


def _packed_ptr(w_packed, N, K, device) -> int:
    if w_packed is None:
        return 0
    _check(w_packed.dtype == torch.bfloat16 and w_packed.is_contiguous() and w_packed.device == device
           and tuple(w_packed.shape) == (-(-N // 16), -(-K // 64), 16, 64),
           "w_packed must be pack_panels(w): contiguous bf16 [ceil(N/16), ceil(K/64), 16, 64] on x's device")
    return w_packed.data_ptr()


def linear(x, w, bias=None, act="none", glu=False, w_scale=None, out=None, nt_hint=0, split_hint=0,
           partial_ok=False, mx_out=False, w_packed=None):
    """``x`` bf16 [M, K], or an :class:`MxAct` for an fp8 weight with a W8A8 gemm_mid plan; ``mx_out``: return an
    fp8 SwiGLU output as :class:`MxAct` (its plan must allow it: :func:`mx_mlp_ok`). ``w_packed``: the
    :func:`pack_panels` twin of ``w``; a plan (hint or tuned) with :data:`PACKED_HINT` reads it instead of ``w``."""
    M, K = x.shape
    if isinstance(x, MxAct) or mx_out:
        _check(w_scale is not None, "MX-fp8 activations need fp8 weights")
        plan = (nt_hint, split_hint) if nt_hint else _w8a8_mid_plan(M, w.shape[0], K, glu)
        _check(plan is not None and _w8a8_mid(plan[0]), "MX-fp8 activations need a W8A8 gemm_mid plan")
        h = plans.decode(plan[0])
        return linear_w8a8(x, w, w_scale, bias, act, glu, out, h.tile, h.depth, plan[1], partial_ok=partial_ok,
                           ilv=h.ilv, mx_out=mx_out)
    _bf16_rows(x, "x")
    fp8 = w_scale is not None
    if fp8:
        _check(w.dtype == torch.uint8 and w.is_contiguous() and w.is_cuda, "fp8 weight stored as uint8 [N, K]")
        _check(w_scale.dtype == torch.float32 and w_scale.numel() == w.shape[0], "w_scale [N] fp32")
        tuned = lib().gemm_tuned_get(M, w.shape[0], K, bool(glu), 1) if not nt_hint else None
        if tuned is not None and tuned[0] & W8A8_FLAG:  # the autotuner picked W8A8 for this M
            nt_hint, split_hint = tuned
        if nt_hint & W8A8_FLAG:
            h = plans.decode(nt_hint)
            return linear_w8a8(x, w, w_scale, bias, act, glu, out, h.tile, h.depth, split_hint, partial_ok=partial_ok,
                               ilv=h.ilv)
        if M > _FP8_PREFILL_M and not nt_hint and tuned is None:  # compute-bound: per-token fp8 activations
            return linear_w8a8(x, w, w_scale, bias, act, glu, out, partial_ok=partial_ok)  # on the MX-fp8 MFMA
    else:
        _bf16_rows(w, "w")
        _check(w.is_contiguous(), "w contiguous")
    N = w.shape[0]
    _check(w.shape[1] == K, f"weight K={w.shape[1]} != x K={K}")
    # gemm_dec / gemm_mid hints take K % 8 == 0 (16-byte K-tail chunks); the library checks the plan it really runs
    _check(K % 16 == 0 or (K % 8 == 0 and nt_hint), "K must be a multiple of 16")
    if glu:
        _check(N % 32 == 0, "glu needs N % 32 == 0")
    if bias is not None:
        _check(bias.dtype == torch.bfloat16 and bias.is_contiguous() and bias.numel() == N, "bias [N] bf16")
    nout = N // 2 if glu else N
    ws = _GEMM_WS.get(64 << 20, x.device)
    partial_ok = partial_ok and not glu and act in ("none", None) and out is None
    y = out if out is not None else (None if partial_ok else torch.empty(M, nout, dtype=x.dtype, device=x.device))
    if partial_ok and lib().gemm_partial_slabs(M, N, K, fp8, False, 0, int(nt_hint), int(split_hint),
                                               ws.numel() * 4) == 0:
        y = torch.empty(M, nout, dtype=x.dtype, device=x.device)  # this call finishes its output itself
    if y is not None:
        _bf16_rows(y, "out", nout)
    S = lib().gemm(x.data_ptr(), x.stride(0), w.data_ptr(), K, fp8, _ptr(w_scale), _ptr(bias), _ptr(y),
                   y.stride(0) if y is not None else nout, M, N, K, _ACT[act], bool(glu), ws.data_ptr(),
                   ws.numel() * 4, int(nt_hint), int(split_hint), bool(y is None), _stream(),
                   _packed_ptr(w_packed, N, K, x.device) if M <= 64 or nt_hint else 0)
    if y is None:
        if S <= 1:
            raise RuntimeError("internal: partial GEMM did not produce partial slabs")
        return PartialSum(ws, S, M, N, bias, x.device)
    return y


def linear_qkv(x, w, bias, positions, cos, sin, k_cache, v_cache, slots, nh, nkv, D, rot, style, do_rope=True,
               nt_hint=0, split_hint=0, w_packed=None):
    """QKV projection whose GEMM epilogue applies RoPE and writes k / v into the paged cache (one launch
    instead of GEMM + rope_cache; same values). Returns the bf16 [T, N] qkv tensor, or None when this
    weight / cache / plan cannot take the fused epilogue (packed or fp8 weights, fp8 KV rows, streaming or
    big-tile plans, neox RoPE on tiles that are not head-aligned): the caller then runs linear + rope_cache."""
    if w.dim() != 2 or w.dtype != torch.bfloat16 or (k_cache is not None and k_cache.dtype != torch.bfloat16):
        return None
    M, K = x.shape
    _bf16_rows(x, "x")
    _bf16_rows(w, "w")
    _check(w.is_contiguous() and w.shape[1] == K, "w [N, K] contiguous")
    N = w.shape[0]
    _check(N == (nh + 2 * nkv) * D and D % 8 == 0, "qkv width")
    if bias is not None:
        _check(bias.dtype == torch.bfloat16 and bias.is_contiguous() and bias.numel() == N, "bias [N] bf16")
    _check(positions.dtype == torch.int64 and positions.numel() == M and positions.is_contiguous(), "positions")
    do_rope = bool(do_rope and rot > 0)
    if do_rope:
        _check(cos.dtype == torch.float32 and cos.is_contiguous() and cos.shape[1] == rot // 2, "cos table")
        _check(sin.shape == cos.shape and sin.is_contiguous(), "sin table")
    bs = 1
    if k_cache is not None:
        _kv_cache_check(k_cache, v_cache, nkv, D)
        _check(slots is not None and slots.dtype == torch.int64 and slots.numel() == M and slots.is_contiguous(),
               "slots")
        bs = k_cache.shape[2]
    ws = _GEMM_WS.get(64 << 20, x.device)
    y = torch.empty(M, N, dtype=x.dtype, device=x.device)
    rc = lib().gemm_qkv(x.data_ptr(), x.stride(0), w.data_ptr(), K, _ptr(bias), y.data_ptr(), y.stride(0), M, N, K,
                        ws.data_ptr(), ws.numel() * 4, int(nt_hint), int(split_hint), positions.data_ptr(),
                        _ptr(cos) if do_rope else 0, _ptr(sin) if do_rope else 0, _ptr(k_cache), _ptr(v_cache),
                        _ptr(slots) if k_cache is not None else 0, nh, nkv, D, rot, bs, 1 if style == "gptj" else 0,
                        do_rope, _stream(), _packed_ptr(w_packed, N, K, x.device) if M <= 64 or nt_hint else 0)
    return y if rc == 0 else None


def add_norm_partial(p: PartialSum, weight, bias, eps, rms, residual, out=None, fp8_out=False):
    T, H = p.M, p.N
    _check(residual is not None and residual.is_contiguous() and residual.shape == (T, H), "residual [T, H]")
    _check(weight.numel() == H and weight.dtype == torch.bfloat16 and weight.is_contiguous(), "norm weight")
    y = out if out is not None else torch.empty(T, H, dtype=torch.bfloat16, device=residual.device)
    q8, s8 = _fp8_twin(y) if fp8_out else (None, None)
    lib().add_norm_partial(p.buf.data_ptr(), p.S, T * H, _ptr(p.bias), residual.data_ptr(), residual.data_ptr(),
                           weight.data_ptr(), _ptr(bias), y.data_ptr(), y.stride(0), T, H, float(eps), bool(rms),
                           _stream(), _ptr(q8), _ptr(s8))
    return y, residual


def w8a8_planned(M: int, N: int, K: int, glu: bool) -> bool:
    """Whether an fp8-weight linear of this shape runs W8A8 (per-token fp8 activations) at M rows: the tuned
    table's plan, else the static rule (W8A8 above _FP8_PREFILL_M rows)."""
    tuned = lib().gemm_tuned_get(M, N, K, bool(glu), 1)
    if tuned is not None:
        return bool(tuned[0] & W8A8_FLAG)
    return M > _FP8_PREFILL_M


def quant_fp8_rows(w):
    _bf16_rows(w, "w")
    _check(w.is_contiguous(), "w contiguous")
    N, K = w.shape
    q = torch.empty(N, K, dtype=torch.uint8, device=w.device)
    s = torch.empty(N, dtype=torch.float32, device=w.device)
    lib().quant_fp8_rows(w.data_ptr(), q.data_ptr(), s.data_ptr(), N, K, _stream())
    return q, s


# ---------------------------------------------------------------------------------- sampler
CAND_K = 64  # rows with 1 <= top_k <= CAND_K (or greedy) can be sampled from gathered candidates
CAND_KC = 128  # candidate slots per rank and row (>= CAND_K: ties at the K-th value ride along)
CAND_MAX_SHARD = 16384  # widest vocab shard the candidate kernel takes


def cand_topk(local, lo, V, temperature, top_k, K=CAND_K, KC=CAND_KC, out=None, shards=1):
    """Per-rank candidates of a vocab-parallel logit shard: [B, 2*KC] fp32 (KC scaled values, then KC
    global token ids as int32 bits). ``shards`` > 1: the row is cut into that many column shards sampled by
    one launch (grid.y), packed shard-major [B, shards * 2*KC] - the layout of gathered per-rank packs, so a
    single GPU samples its full vocabulary through the same two short kernels instead of one long
    row-per-workgroup pass."""
    _bf16_rows(local, "local logits")
    B, width = local.shape
    vl = -(-width // shards)
    _check(shards >= 1 and vl <= CAND_MAX_SHARD, "vocab shard too wide for the candidate sampler")
    for t, dt, nm in ((temperature, torch.float32, "temperature"), (top_k, torch.int32, "top_k")):
        _check(t.dtype == dt and t.numel() >= B and t.is_contiguous() and t.is_cuda, f"{nm} must be {dt}")
    pack = out if out is not None else torch.empty(B, shards * 2 * KC, dtype=torch.float32, device=local.device)
    _check(pack.shape == (B, shards * 2 * KC) and pack.is_contiguous() and pack.dtype == torch.float32,
           "candidate pack")
    # columns past `width` in the last shard are masked by the kernel's lo + j < V bound only if V <= width
    _check(V <= width or shards == 1, "sharded candidates need the vocabulary inside the logits row")
    lib().cand_topk(local.data_ptr(), local.stride(0), B, vl, int(lo), int(V), temperature.data_ptr(),
                    top_k.data_ptr(), int(K), int(KC), pack.data_ptr(), pack.stride(0), _stream(), int(shards))
    return pack


def _ln_min_p_arg(ln_min_p, B, device):
    """Checked ``ln_min_p`` [B] fp32 (ln of each row's min_p, -inf = off) -> pointer extras of the launch; none
    without it, which runs the kernels without the min-p floor."""
    if ln_min_p is None:
        return ()
    _check(ln_min_p.dtype == torch.float32 and ln_min_p.dim() == 1 and ln_min_p.numel() >= B
           and ln_min_p.is_contiguous() and ln_min_p.is_cuda and ln_min_p.device == device,
           "ln_min_p must be torch.float32 [B] on the logits' device")
    return (ln_min_p.data_ptr(),)


def sample_cand(pack, KC, temperature, top_k, top_p, seeds, out=None, out2=None, ln_min_p=None):
    """Sample from gathered candidates ``pack`` [B, groups * 2*KC] (rank-major). ``ln_min_p``: see sample."""
    _check(pack.is_cuda and pack.dtype == torch.float32 and pack.dim() == 2 and pack.stride(1) == 1, "pack")
    B = pack.shape[0]
    _check(pack.shape[1] % (2 * KC) == 0, "pack width must be a multiple of 2*KC")
    groups = pack.shape[1] // (2 * KC)
    for t, dt, nm in ((temperature, torch.float32, "temperature"), (top_k, torch.int32, "top_k"),
                      (top_p, torch.float32, "top_p"), (seeds, torch.int64, "seeds")):
        _check(t.dtype == dt and t.numel() >= B and t.is_contiguous() and t.is_cuda, f"{nm} must be {dt}")
    extra = _ln_min_p_arg(ln_min_p, B, pack.device)
    y = out if out is not None else torch.empty(B, dtype=torch.int64, device=pack.device)
    lib().sample_cand(pack.data_ptr(), pack.stride(0), B, groups, int(KC), temperature.data_ptr(), top_k.data_ptr(),
                      top_p.data_ptr(), seeds.data_ptr(), y.data_ptr(), _ptr(out2), _stream(), *extra)
    return y


def sample(logits, temperature, top_k, top_p, seeds, vocab: Optional[int] = None, out=None, out2=None,
           ln_min_p=None):
    """``ln_min_p`` [B] fp32 (None: off): the min-p floor as fp32 ln(min_p) per row, -inf where a row has none.
    A non-greedy row keeps, after top-k and top-p, only tokens with scaled logit >= max + ln_min_p (the MINP
    kernel variants of csrc/sampling.hip; ops/reference.py _select is the definition)."""
    _check(logits.is_cuda and logits.dim() == 2 and logits.stride(1) == 1, "logits [B, V]")
    _check(logits.dtype in (torch.bfloat16, torch.float32), "logits bf16/fp32")
    B = logits.shape[0]
    V = vocab or logits.shape[1]
    _check(V <= logits.shape[1], "vocab > logits width")
    for t, dt, nm in ((temperature, torch.float32, "temperature"), (top_k, torch.int32, "top_k"),
                      (top_p, torch.float32, "top_p"), (seeds, torch.int64, "seeds")):
        if t is not None:
            _check(t.dtype == dt and t.numel() >= B and t.is_contiguous() and t.is_cuda, f"{nm} must be {dt}")
    extra = _ln_min_p_arg(ln_min_p, B, logits.device)
    y = out if out is not None else torch.empty(B, dtype=torch.int64, device=logits.device)
    lib().sample(logits.data_ptr(), logits.stride(0), logits.dtype == torch.float32, B, V, _ptr(temperature),
                 _ptr(top_k), _ptr(top_p), _ptr(seeds), y.data_ptr(), _ptr(out2), _stream(), *extra)
    return y


# -------------------------------------------------------------------------------- log-probabilities
MAX_TOP_LOGPROBS = _ref.MAX_TOP_LOGPROBS
LOGPROB_MAX_CAND = 2048  # groups * N the combine kernel ranks in LDS


def _lp_logits(logits, tokens, N, name="logits"):
    _check(isinstance(N, int) and 0 <= N <= MAX_TOP_LOGPROBS, f"N must be an int in 0..{MAX_TOP_LOGPROBS}, got {N!r}")
    _check(logits.is_cuda and logits.dim() == 2 and logits.stride(1) == 1, f"{name} must be [B, V] GPU rows")
    _check(logits.device.index == torch.cuda.current_device(),
           f"{name} is on {logits.device} but the current device is cuda:{torch.cuda.current_device()}")
    _check(logits.dtype in (torch.bfloat16, torch.float32), f"{name} must be bfloat16 or float32, got {logits.dtype}")
    _check(logits.shape[0] == 0 or logits.stride(0) >= logits.shape[1], f"{name} rows overlap")
    B = logits.shape[0]
    _check(torch.is_tensor(tokens) and tokens.dtype == torch.int64 and tokens.device == logits.device
           and tokens.dim() == 1 and tokens.shape[0] == B and tokens.is_contiguous(),
           f"tokens must be a contiguous int64 [B={B}] tensor on {logits.device}")
    return B


def _lp_outputs(B, N, device, out):
    """(lp [B], top_lp [B, N], top_ids [B, N]): fresh, or the caller's (row-strided views are fine)."""
    if out is None:
        return (torch.empty(B, dtype=torch.float32, device=device),
                torch.empty(B, N, dtype=torch.float32, device=device),
                torch.empty(B, N, dtype=torch.int32, device=device))
    lp, top, ids = out
    for t, dt, shape, nm in ((lp, torch.float32, (B,), "lp"), (top, torch.float32, (B, N), "top_lp"),
                             (ids, torch.int32, (B, N), "top_ids")):
        _check(t.dtype == dt and tuple(t.shape) == shape and t.device == device, f"out {nm} must be {dt} {shape}")
        _check(t.dim() == 1 or N == 0 or t.stride(1) == 1, f"out {nm} rows must be contiguous")
        _check(B <= 1 or t.stride(0) >= (1 if t.dim() == 1 else N), f"out {nm} rows overlap")
    return lp, top, ids


def token_logprobs(logits, V, tokens, N, out=None):
    """``log_softmax(logits[:, :V])`` of ``tokens`` [B] and of the N most likely tokens per row (logit descending,
    ties by ascending id): (lp [B] fp32, top_lp [B, N] fp32, top_ids [B, N] int32); entries past V are -inf / -1."""
    B = _lp_logits(logits, tokens, N)
    V = int(V)
    _check(1 <= V <= logits.shape[1], f"V = {V} outside the logits row of {logits.shape[1]} columns")
    lp, top, ids = _lp_outputs(B, N, logits.device, out)
    lib().token_logprobs(logits.data_ptr(), logits.stride(0), logits.dtype == torch.float32, B, V, 0, V,
                         tokens.data_ptr(), N, 1, lp.data_ptr(), lp.stride(0) if B else 1, top.data_ptr(),
                         top.stride(0), ids.data_ptr(), ids.stride(0), 0, 0, _stream())
    return lp, top, ids


def token_logprobs_partial(local, lo, V, tokens, N, shards=1, out=None):
    """Packs of a vocab-parallel shard ``local`` [B, width] whose column 0 is global token ``lo``:
    [B, shards * (3 + 2N)] fp32 (ops/reference.py token_logprobs_partial). ``shards`` > 1 cuts the row into that
    many column shards in one launch, packed shard-major like gathered per-rank packs."""
    B = _lp_logits(local, tokens, N, "local logits")
    _check(isinstance(shards, int) and shards >= 1, "shards must be a positive int")
    _check(int(lo) >= 0 and int(V) >= 1, "lo / V")
    width = local.shape[1]
    _check(width >= 1, "empty shard")
    P = 3 + 2 * N
    pack = out if out is not None else torch.empty(B, shards * P, dtype=torch.float32, device=local.device)
    _check(pack.dtype == torch.float32 and tuple(pack.shape) == (B, shards * P) and pack.device == local.device
           and pack.stride(1) == 1 and (B <= 1 or pack.stride(0) >= shards * P), "log-probability pack")
    lib().token_logprobs(local.data_ptr(), local.stride(0), local.dtype == torch.float32, B, width, int(lo), int(V),
                         tokens.data_ptr(), N, shards, 0, 0, 0, 0, 0, 0, pack.data_ptr(), pack.stride(0), _stream())
    return pack


def token_logprobs_combine(pack, N, out=None):
    """Merge gathered packs [B, groups * (3 + 2N)] (rank-major) into (lp, top_lp, top_ids)."""
    _check(isinstance(N, int) and 0 <= N <= MAX_TOP_LOGPROBS, f"N must be an int in 0..{MAX_TOP_LOGPROBS}")
    _check(pack.is_cuda and pack.dtype == torch.float32 and pack.dim() == 2 and pack.stride(1) == 1, "pack")
    _check(pack.device.index == torch.cuda.current_device(), "pack is not on the current device")
    B = pack.shape[0]
    P = 3 + 2 * N
    _check(pack.shape[1] >= P and pack.shape[1] % P == 0, f"pack width must be a multiple of 3 + 2N = {P}")
    _check(B <= 1 or pack.stride(0) >= pack.shape[1], "pack rows overlap")
    groups = pack.shape[1] // P
    _check(groups * N <= LOGPROB_MAX_CAND, "too many gathered candidates per row")
    lp, top, ids = _lp_outputs(B, N, pack.device, out)
    lib().logprobs_combine(pack.data_ptr(), pack.stride(0), B, groups, N, lp.data_ptr(), lp.stride(0) if B else 1,
                           top.data_ptr(), top.stride(0), ids.data_ptr(), ids.stride(0), _stream())
    return lp, top, ids


# ---------------------------------------------------------------------------------------- penalties
def _pen_vec(t, dt, n, device, name):
    _check(torch.is_tensor(t) and t.dtype == dt and t.device == device and t.dim() == 1 and t.shape[0] == n
           and t.is_contiguous(), f"{name} must be a contiguous {dt} [{n}] tensor on {device}")


def _pen_state(state, name="state"):
    _check(torch.is_tensor(state) and state.is_cuda and state.dtype == torch.int32 and state.dim() == 2
           and state.stride(1) == 1, f"{name} must be [S, vocab] int32 GPU rows")
    _check(state.device.index == torch.cuda.current_device(),
           f"{name} is on {state.device} but the current device is cuda:{torch.cuda.current_device()}")
    _check(state.shape[0] <= 1 or state.stride(0) >= state.shape[1], f"{name} rows overlap")


def _overlap(a, b) -> bool:
    """Do the address ranges of two row-strided 2-D tensors intersect?"""
    def span(t):
        n = (t.shape[0] - 1) * t.stride(0) + t.shape[1] if t.numel() else 0
        return t.data_ptr(), t.data_ptr() + n * t.element_size()
    a0, a1 = span(a)
    b0, b1 = span(b)
    return a0 < b1 and b0 < a1


def apply_penalties(logits, state, slots, new_tokens, rep, pres, freq, lo=0, vocab=None, out=None):
    """Repetition / presence / frequency penalties over ``logits`` [B, W] (bf16 / fp32, any row stride) whose column
    j is global token ``lo + j``, written out of place into ``out`` (csrc/penalties.hip; ops/reference.py
    apply_penalties is the definition). Row b with ``slots[b]`` >= 0 first registers ``new_tokens[b]`` (>= 0) as one
    more output occurrence in its ``state`` row. The rows of one call must hold different slots."""
    _check(torch.is_tensor(logits) and logits.is_cuda and logits.dim() == 2 and (logits.shape[1] <= 1 or
                                                                                logits.stride(1) == 1),
           "logits must be [B, W] GPU rows")
    _check(logits.device.index == torch.cuda.current_device(),
           f"logits is on {logits.device} but the current device is cuda:{torch.cuda.current_device()}")
    _check(logits.dtype in (torch.bfloat16, torch.float32), f"logits must be bfloat16 or float32, got {logits.dtype}")
    B, W = logits.shape
    _check(B <= 1 or logits.stride(0) >= W, "logits rows overlap")
    _pen_state(state)
    _check(state.device == logits.device, "state and logits are on different devices")
    vocab = state.shape[1] if vocab is None else int(vocab)
    lo = int(lo)
    _check(lo >= 0 and 0 <= vocab <= state.shape[1], f"need lo >= 0 and 0 <= vocab <= state.shape[1] = "
                                                      f"{state.shape[1]}, got lo = {lo}, vocab = {vocab}")
    _check(B <= 65535 and lo + W < 2 ** 31, "too many rows or columns")
    _pen_vec(slots, torch.int32, B, logits.device, "slots")
    _pen_vec(new_tokens, torch.int64, B, logits.device, "new_tokens")
    for t, nm in ((rep, "rep"), (pres, "pres"), (freq, "freq")):
        _pen_vec(t, torch.float32, B, logits.device, nm)
    if out is None:
        out = torch.empty(B, W, dtype=logits.dtype, device=logits.device)
    _check(torch.is_tensor(out) and out.dtype == logits.dtype and out.device == logits.device
           and tuple(out.shape) == (B, W) and (W <= 1 or out.stride(1) == 1),
           f"out must be a {logits.dtype} [{B}, {W}] tensor with contiguous rows on {logits.device}")
    _check(B <= 1 or out.stride(0) >= W, "out rows overlap")
    _check(not _overlap(out, logits), "out must not alias logits: the raw logits are kept")
    lib().apply_penalties(logits.data_ptr(), logits.stride(0), out.data_ptr(), out.stride(0),
                          logits.dtype == torch.float32, B, W, lo, vocab, state.data_ptr(), state.stride(0),
                          state.shape[0], slots.data_ptr(), new_tokens.data_ptr(), rep.data_ptr(), pres.data_ptr(),
                          freq.data_ptr(), _stream())
    return out


def penalty_reset(state, slots, cu, tokens, words):
    """(Re)build the state rows ``slots`` [R] int32 (-1: skip) in one launch: row i becomes zero except its distinct
    ``tokens[cu[i]:cu[i + 1]]`` (int64), which get ``words[cu[i]:cu[i + 1]]`` (int32). ``cu`` [R + 1] int32."""
    _pen_state(state)
    dev = state.device
    _check(torch.is_tensor(slots) and slots.dim() == 1, "slots must be 1-D")
    R = slots.shape[0]
    _check(R <= 65535, "too many rows")
    _pen_vec(slots, torch.int32, R, dev, "slots")
    _pen_vec(cu, torch.int32, R + 1, dev, "cu")
    _check(torch.is_tensor(tokens) and tokens.dim() == 1, "tokens must be 1-D")
    n = tokens.shape[0]
    _pen_vec(tokens, torch.int64, n, dev, "tokens")
    _pen_vec(words, torch.int32, n, dev, "words")
    lib().penalty_reset(state.data_ptr(), state.stride(0), state.shape[0], state.shape[1], slots.data_ptr(), R,
                        cu.data_ptr(), n, tokens.data_ptr(), words.data_ptr(), _stream())
    return state


# ---------------------------------------------------------------------------------------- token constraints
def apply_token_edits(logits, edit_ids, edit_vals, edit_meta, slots, nout, lo=0, vocab=None, out=None):
    """Token constraints over ``logits`` [B, W] (bf16 / fp32, any row stride) whose column j is global token
    ``lo + j``, written out of place into ``out`` (csrc/constraints.hip; ops/reference.py apply_token_edits is the
    definition). ``edit_ids`` [S, 2, E] int32, ``edit_vals`` [S, 2, E] fp32 and ``edit_meta`` [S, 4] int32 are the
    constraint slots' state, which the launch only reads; ``slots`` [B] int32 (-1: copy the row), ``nout`` [B] int32
    the tokens each row's sequence has generated so far."""
    _check(torch.is_tensor(logits) and logits.is_cuda and logits.dim() == 2 and (logits.shape[1] <= 1 or
                                                                                logits.stride(1) == 1),
           "logits must be [B, W] GPU rows")
    dev = logits.device
    _check(dev.index == torch.cuda.current_device(),
           f"logits is on {dev} but the current device is cuda:{torch.cuda.current_device()}")
    _check(logits.dtype in (torch.bfloat16, torch.float32), f"logits must be bfloat16 or float32, got {logits.dtype}")
    B, W = logits.shape
    _check(B <= 1 or logits.stride(0) >= W, "logits rows overlap")
    def slot_rows(t):  # each slot's row contiguous, the slots themselves apart by any stride that keeps them disjoint
        n = t[0].numel() if t.shape[0] else 0
        return t.shape[0] == 0 or (t[0].is_contiguous() and (t.shape[0] == 1 or t.stride(0) >= n))
    _check(torch.is_tensor(edit_ids) and edit_ids.dtype == torch.int32 and edit_ids.dim() == 3
           and edit_ids.shape[1] == 2 and edit_ids.device == dev and slot_rows(edit_ids),
           f"edit_ids must be an int32 [S, 2, E] tensor on {dev} with contiguous slots")
    S, _, E = edit_ids.shape
    _check(torch.is_tensor(edit_vals) and edit_vals.dtype == torch.float32 and tuple(edit_vals.shape) == (S, 2, E)
           and edit_vals.device == dev and slot_rows(edit_vals),
           f"edit_vals must be a float32 [{S}, 2, {E}] tensor on {dev} with contiguous slots")
    _check(torch.is_tensor(edit_meta) and edit_meta.dtype == torch.int32 and tuple(edit_meta.shape) == (S, 4)
           and edit_meta.device == dev and slot_rows(edit_meta),
           f"edit_meta must be an int32 [{S}, 4] tensor on {dev} with contiguous slots")
    lo = int(lo)
    vocab = lo + W if vocab is None else int(vocab)
    _check(lo >= 0 and vocab >= 0, f"need lo >= 0 and vocab >= 0, got lo = {lo}, vocab = {vocab}")
    _check(B <= 65535 and lo + W < 2 ** 31 and vocab < 2 ** 31, "too many rows or columns")
    _pen_vec(slots, torch.int32, B, dev, "slots")
    _pen_vec(nout, torch.int32, B, dev, "nout")
    if out is None:
        out = torch.empty(B, W, dtype=logits.dtype, device=dev)
    _check(torch.is_tensor(out) and out.dtype == logits.dtype and out.device == dev
           and tuple(out.shape) == (B, W) and (W <= 1 or out.stride(1) == 1),
           f"out must be a {logits.dtype} [{B}, {W}] tensor with contiguous rows on {dev}")
    _check(B <= 1 or out.stride(0) >= W, "out rows overlap")
    _check(not _overlap(out, logits), "out must not alias logits: the raw logits are kept")
    lib().apply_token_edits(logits.data_ptr(), logits.stride(0), out.data_ptr(), out.stride(0),
                            logits.dtype == torch.float32, B, W, lo, vocab, edit_ids.data_ptr(),
                            max(edit_ids.stride(0), 2 * E), edit_vals.data_ptr(), max(edit_vals.stride(0), 2 * E),
                            edit_meta.data_ptr(), max(edit_meta.stride(0), 4), S, E, slots.data_ptr(),
                            nout.data_ptr(), _stream())
    return out
