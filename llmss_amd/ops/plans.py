"""The GEMM plan encoding, named: the fields of ``nt_hint`` / ``split_hint``, the tile table, and the helpers that
build, decode and describe hints. The Python twin of ``csrc/gemm_plan.h`` (which documents the encoding and resolves
a hint to a launch); ``tests/test_plan_resolve_cpu.py`` holds the two tables to each other.

The integers are the stored and wire format (tuned table, ``nt_hint=`` keywords, logged hex): nothing here changes
them, it only gives the bits names."""
from __future__ import annotations

from collections import namedtuple
from typing import Optional

STREAM_MASK = 0xff  # streaming kernels: nt + 16 * variant
TILE_SHIFT = 8  # tile code 1-15 (with DEC: the BN code 1-5)
DEPTH_SHIFT = 12  # bf16 plans: 2-bit depth code; W8A8 plans: 4-bit literal depth
DEFAULT_W = 64 << TILE_SHIFT  # default-policy weight loads
STREAM_K = 128 << TILE_SHIFT  # stream-K; split_hint = workgroups per CU
COMBINE = 256 << TILE_SHIFT  # split-K combined inside the launch
ILV = 512 << TILE_SHIFT  # gemm_mid's interleaved ring
DEC = 1024 << TILE_SHIFT  # gemm_dec (K split over the waves)
PACKED = 2048 << TILE_SHIFT  # the plan reads the panel-packed copy of the weight (ops.hip.pack_panels)
W8A8 = 1 << 20  # per-token fp8 activations (launch_gemm_f8f8); decoded here only
D2, D3, D4, D6 = 0, 16, 32, 48  # depth field of a bf16 tile hint: 2 / 3 / 4 / 6 stages (gemm_dec: 2 / 3 / 4 / 4)
_TILED_DEPTH, _DEC_DEPTH = (2, 3, 4, 6), (2, 3, 4, 4)


# family: tiled / wide8 / ping_pong / mid / dec; packed: has a packed-weight variant; k8: takes K % 8 == 0 (the others
# K % 16 == 0); qkv: can carry the QKV RoPE / KV-write epilogue
Tile = namedtuple("Tile", "code family bm bn threads packed k8 qkv", defaults=(False, False, True))
TILES = (
    Tile(1, "tiled", 128, 128, 256), Tile(2, "tiled", 64, 128, 256), Tile(3, "tiled", 64, 64, 256),
    Tile(4, "ping_pong", 256, 256, 512, qkv=False), Tile(5, "wide8", 256, 128, 512), Tile(6, "wide8", 256, 64, 512),
    Tile(7, "mid", 64, 48, 128, True, True), Tile(8, "mid", 128, 128, 256, False, True),
    Tile(9, "mid", 256, 128, 512, False, True), Tile(10, "mid", 64, 256, 256, True, True),
    Tile(11, "mid", 64, 128, 256, True, True), Tile(12, "mid", 128, 256, 512, False, True),
    Tile(13, "mid", 64, 192, 256, True, True), Tile(14, "mid", 64, 32, 256, True, True),
    Tile(15, "mid", 64, 96, 256, True, True),
    Tile(1, "dec", 64, 16, 256, True, True), Tile(2, "dec", 64, 32, 256, True, True),
    Tile(3, "dec", 64, 48, 256, True, True), Tile(4, "dec", 64, 64, 256, True, True),
    Tile(5, "dec", 64, 96, 256, True, True),
)
MID_TILE_BN = {t.code: t.bn for t in TILES if t.family == "mid"}  # gemm_mid tile -> BN


def tile(code: int, dec: bool = False) -> Optional[Tile]:
    return next((t for t in TILES if t.code == code and (t.family == "dec") == dec), None)


def stream_hint(nt: int, variant: int = 0) -> int:
    return nt + 16 * variant


def tile_hint(code: int, depth: int = D2, flags: int = 0) -> int:
    """bf16 plan on tile ``code`` with depth field D2 / D3 / D4 / D6 and any of the flag bits above."""
    return ((code | depth) << TILE_SHIFT) | flags


def w8a8_hint(code: int, depth: int = 0, flags: int = 0) -> int:
    """W8A8 plan: tile code, LITERAL ring depth (0 = the kernel's default), ILV."""
    return W8A8 | (code << TILE_SHIFT) | (depth << DEPTH_SHIFT) | flags


# nt: the streaming kernels' 64-column blocks per workgroup (0: not a streaming hint); depth: ring stages asked for
# (W8A8: 0 = the kernel's default)
Hint = namedtuple("Hint", "nt variant tile depth default_w streamk combine ilv dec packed w8a8")


def decode(nt: int) -> Hint:
    w8 = bool(nt & W8A8)
    dec = bool(nt & DEC) and not w8
    code = (nt >> DEPTH_SHIFT) & (15 if w8 else 3)
    depth = code if w8 else (_DEC_DEPTH if dec else _TILED_DEPTH)[code]
    flag = lambda f: bool(nt & f) and not w8
    return Hint(nt & 15, (nt & STREAM_MASK) >> 4, (nt >> TILE_SHIFT) & 15, depth, flag(DEFAULT_W), flag(STREAM_K),
                flag(COMBINE), bool(nt & ILV), dec, flag(PACKED), w8)


def describe(nt: int, split: int = 0) -> str:
    """One readable line for a plan, printed next to its hex in log lines and bench/plan_dump.py."""
    h = decode(nt)
    if not nt:
        return "static plan" + (f" split {split}" if split else "")
    if nt & STREAM_MASK:
        return f"stream nt={h.nt} v{h.variant or 2} split {split}"
    t = tile(h.tile, h.dec)
    name = f"{t.family} {t.bm}x{t.bn}" if t else ("auto tile" if not h.tile else f"bad tile {h.tile}")
    flags = [n for n, on in (("w8a8", h.w8a8), ("stream-k", h.streamk), ("combine", h.combine), ("ilv", h.ilv),
                             ("default-w", h.default_w), ("packed", h.packed)) if on]
    what = f"{split} wg/cu" if h.streamk else f"split {split}"
    return " ".join([name, f"{h.depth} stages" if h.depth else "default depth", what] + flags)


def packed_twin(M: int, nt: int, fp8: bool = False) -> Optional[int]:
    """The hint of the same plan reading panel-packed weights, or None where the kernel has no such variant:
    gemm_dec and the 64-row gemm_mid tiles (plain, in-launch combine), bf16 weights, M <= 64."""
    h = decode(nt)
    if fp8 or M > 64 or nt & STREAM_MASK or nt >= W8A8 or h.streamk or h.ilv or h.default_w:
        return None
    t = tile(h.tile, h.dec)
    if h.dec or (t is not None and t.family == "mid" and t.packed):
        return nt | PACKED
    return None
