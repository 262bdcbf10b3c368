// The GEMM plan: what the two integers that steer every GEMM call mean, and the one function that turns a problem
// and its hints into the launch that runs. Host-only (no HIP, no pybind), so tests/native/gemm_plan_host_test.cpp
// builds it alone under AddressSanitizer + UndefinedBehaviorSanitizer; csrc/gemm.hip launches what it resolves and
// llmss_amd/ops/plans.py names the same fields for Python.
//
// nt_hint (the stored and wire format: the tuned table, gemm_tuned_set / get, every nt_hint= keyword, logged hex):
//   bits 0-7    streaming kernels: nt + 16 * variant. nt = 64-column blocks per workgroup (1, 2, 4), variant 1 =
//               LDS-DMA X staging, 2 (default) = register-staged X + 3-deep W ring. Nonzero selects them.
//   bits 8-11   tile code 1-15 (kGemmTiles below); with kTileDec the BN code 1-5 of gemm_dec.
//   bits 12-13  ring-depth code: 2 / 3 / 4 / 6 stages (kTiledDepth), gemm_dec 2 / 3 / 4 / 4 (kDecDepth). The kernels
//               clamp the request to what their LDS image holds (dec_depth, mid_depth, mx_ns in the kernel files).
//   bit 14      kTileDefaultW: default-policy weight loads (else non-temporal when one workgroup row reads a tile).
//   bit 15      kTileStreamK: stream-K (4-wave tiled tiles, bf16 weights); split_hint = workgroups per CU. The
//               output is finished in the launch. Dropped silently on the 8-wave and gemm_mid tiles.
//   bit 16      kTileCombine: split-K slices combine in the launch (last arriver per tile, common.h
//               splitk_combine): slabs [tile][split][bm * bn] in the workspace, finished output, no reduce launch.
//   bit 17      kTileIlv: gemm_mid's interleaved (software-pipelined) ring, >= 3 stages.
//   bit 18      kTileDec: gemm_dec (K split over the waves, M <= 64, bf16 weights); split_hint = K split over
//               the grid.
//   bit 19      kTilePacked: the weight pointer is the panel-packed copy [ceil(N/16)][ceil(K/64)][16][64] (pack.hip):
//               gemm_dec and the 64-row gemm_mid tiles, bf16 weights, M <= 64, bit-identical output. An explicit
//               hint with the bit and no packed copy throws; a TUNED plan without one runs its row-major sibling.
//   bit 20      kHintW8A8: a W8A8 plan (fp8 activations, launch_gemm_f8f8). Decoded in Python only (ops/plans.py):
//               bits 8-11 the tile code, bits 12-15 the LITERAL ring depth, kTileIlv as above.
// split_hint: K split over grid.y (0 = the planner's choice), or workgroups per CU under kTileStreamK.
// A call with both hints 0 takes the tuned table's entry for (M, N, K, glu, kind), else the static plan.
// A split plan finishes its output by (GemmFinish) a splitk_reduce launch, the in-launch combine, or - partial_out
// without activation / GLU - leaves fp32 slabs [split, M, N] in the workspace for the consumer (rope_cache /
// add_norm sum them and add the bias).
#pragma once

#include <algorithm>
#include <cstdint>
#include <mutex>
#include <stdexcept>
#include <unordered_map>
#include <utility>

constexpr int kHintStream = 0xff, kHintTileShift = 8, kHintW8A8 = 1 << 20;
// fields of nt_hint >> kHintTileShift
constexpr int kTileCode = 15, kTileDepthShift = 4, kTileDepth3 = 1 << kTileDepthShift, kTileDefaultW = 64,
              kTileStreamK = 128, kTileCombine = 256, kTileIlv = 512, kTileDec = 1024, kTilePacked = 2048;
constexpr int kTiledDepth[4] = {2, 3, 4, 6}, kDecDepth[4] = {2, 3, 4, 4};
constexpr int kPingPongTile = 4, kGemmBK = 64, kGemmBK8 = 128;  // K elements (bytes for fp8 x fp8) per stage

struct GemmHint {
  int nt, variant;  // streaming kernels (0: not a streaming hint)
  int tile, depth_code;
  bool default_w, streamk, combine, ilv, dec, packed, w8a8;
  int w8a8_depth;  // literal, W8A8 only
};
inline GemmHint gemm_hint_decode(int nt_hint) {
  const unsigned h = (unsigned)nt_hint, t = h >> kHintTileShift;
  return {(int)(h & 15), (int)((h >> 4) & 15), (int)(t & kTileCode), (int)((t >> kTileDepthShift) & 3),
          (t & kTileDefaultW) != 0, (t & kTileStreamK) != 0, (t & kTileCombine) != 0, (t & kTileIlv) != 0,
          (t & kTileDec) != 0, (t & kTilePacked) != 0, (h & kHintW8A8) != 0, (int)((h >> 12) & 15)};
}

// The one tile table. kTiled: gemm_tiled_kernel, 4 waves; kWide8: the same kernel on 8 waves (one workgroup per
// CU); kPingPong: gemm_pp_kernel; kMid: gemm_mid.hip (buffer-descriptor staging, wm x wn waves); kDec: gemm_dec.hip
// (code = BN code; 64 rows, K split over 4 waves).
// gemm_mid: 13 = 64x192 (a 12288-column QKV is 64 tiles), 14 = 64x32 (narrow projections without a K split), 15 =
// 64x96 (Llama-2-7B's 22016-column gate/up is 230 workgroups), 7 = 64x48 (2x1 waves: a 12288-column QKV is exactly
// 256 workgroups).
// (the other families are not tiles of this table: the streaming kernels, stream-K on the kTiled tiles, W8A8's own)
enum class GemmFamily { kNone, kStream, kStreamPanels, kTiled, kWide8, kPingPong, kStreamK, kMid, kDec, kF8Big, kF8Tiled };
struct GemmTile {
  int code;
  GemmFamily family;
  int bm, bn, wm, wn;
  // packed: has a packed-weight variant; k8: takes K % 8 == 0 (stages and zeroes its K tail in 16-byte chunks; the
  // others need K % 16 == 0); qkv: can carry the QKV RoPE / KV-write epilogue
  bool packed, k8, qkv;
  int threads() const { return 64 * wm * wn; }
};
constexpr GemmTile kGemmTiles[] = {
    {1, GemmFamily::kTiled, 128, 128, 2, 2, false, false, true},
    {2, GemmFamily::kTiled, 64, 128, 2, 2, false, false, true},
    {3, GemmFamily::kTiled, 64, 64, 2, 2, false, false, true},
    {4, GemmFamily::kPingPong, 256, 256, 4, 2, false, false, false},
    {5, GemmFamily::kWide8, 256, 128, 4, 2, false, false, true},
    {6, GemmFamily::kWide8, 256, 64, 4, 2, false, false, true},
    {7, GemmFamily::kMid, 64, 48, 2, 1, true, true, true},
    {8, GemmFamily::kMid, 128, 128, 2, 2, false, true, true},
    {9, GemmFamily::kMid, 256, 128, 4, 2, false, true, true},
    {10, GemmFamily::kMid, 64, 256, 1, 4, true, true, true},
    {11, GemmFamily::kMid, 64, 128, 1, 4, true, true, true},
    {12, GemmFamily::kMid, 128, 256, 2, 4, false, true, true},
    {13, GemmFamily::kMid, 64, 192, 2, 2, true, true, true},
    {14, GemmFamily::kMid, 64, 32, 4, 1, true, true, true},
    {15, GemmFamily::kMid, 64, 96, 4, 1, true, true, true},
    {1, GemmFamily::kDec, 64, 16, 4, 1, true, true, true},
    {2, GemmFamily::kDec, 64, 32, 4, 1, true, true, true},
    {3, GemmFamily::kDec, 64, 48, 4, 1, true, true, true},
    {4, GemmFamily::kDec, 64, 64, 4, 1, true, true, true},
    {5, GemmFamily::kDec, 64, 96, 4, 1, true, true, true},
};
inline const GemmTile* gemm_tile(int code, bool dec = false) {
  for (const GemmTile& t : kGemmTiles)
    if (t.code == code && (t.family == GemmFamily::kDec) == dec) return &t;
  return nullptr;
}
// A tile field with flag bits and code 0 is not "auto" (only a field of 0 is): it has always been planned with the
// 64x128 dims and launched on the 64x64 instantiation, which leaves output tiles unwritten when N > 64. Kept as it
// is; no caller builds such a hint.
inline const GemmTile* gemm_planned_tile(int code) { return gemm_tile(code ? code : 2); }
inline int tiles_of(int M, int N, int bm, int bn) { return ((M + bm - 1) / bm) * ((N + bn - 1) / bn); }

// Tile/split choice for the streaming kernel: columns per workgroup and K splits such that the
// grid reaches ~2 workgroups per CU (256 CUs) without splitting K below 4 chunks per slice.
inline void gemm_stream_plan(int M, int N, int K, int* nt_out, int* splitk_out) {
  int nt = (N >= 16384) ? 2 : 1;
  const int nblk = (N + 64 * nt - 1) / (64 * nt);
  const int kc = M > 64 ? 128 : 256;
  const int nck = (K + kc - 1) / kc;
  // measured (bench/gemm_bench.py --sweep, Llama-2-7B shapes): M <= 16 likes ~3 workgroups per
  // CU, larger M ~1 per CU (its X tile already costs LDS); N alone filling the chip -> no split
  const int target = nblk >= 256 ? nblk : (M <= 16 ? 768 : 256);
  int s = 1;
  while (nblk * s < target && s < 16 && nck / (2 * s) >= 4) s *= 2;
  *nt_out = nt;
  *splitk_out = s;
}

// Tiled-path plan on the tile field (tile code | depth code | flag bits). Tile: 64 rows for M <= 64 (64x64, or
// 64x128 when 64x64 gives > 256 tiles), else 128x128. K is split until the grid holds ~3 (64-row tiles) or ~1.5
// (128x128) workgroups per CU, keeping >= 512 k per slice. Measured on the Llama-2-7B shapes at M = 64..512
// (bench/gemm_bench.py --sweep): within ~5% of the best (tile, split) of the sweep everywhere.
inline void gemm_tiled_plan(int M, int N, int K, int* tsel_io, int* split_io, bool glu) {
  int tsel = *tsel_io;
  // SwiGLU output cannot be folded into the next kernel, so a split would cost its own reduce
  // launch: with >= 256 64x64 tiles, no split (measured equal or better at M <= 128)
  if (tsel == 0 && glu && M <= 128 && tiles_of(M, N, 64, 64) >= 256 && *split_io <= 0) {
    *tsel_io = 3 | kTileDepth3;
    *split_io = 1;
    return;
  }
  if (tsel == 0) {
    if (tiles_of(M, N, 256, 256) >= 192) tsel = kPingPongTile;
    else tsel = M <= 64 ? (tiles_of(M, N, 64, 64) > 256 ? 2 : 3) : 1;
  }
  int hint_bits = tsel & ~kTileCode;
  tsel &= kTileCode;
  if (tsel >= 5) hint_bits &= ~kTileStreamK;  // no stream-K variant of the 8-wave and gemm_mid tiles
  if (hint_bits & kTileStreamK) {  // stream-K: output is final (no slabs); split_io carries workgroups per CU
    *tsel_io = tsel | hint_bits;
    if (*split_io <= 0) *split_io = 2;
    return;
  }
  if (tsel == kPingPongTile) {  // no split-K, no stage option
    *tsel_io = tsel;
    *split_io = 1;
    return;
  }
  const GemmTile* t = gemm_planned_tile(tsel);
  const int nt = tiles_of(M, N, t->bm, t->bn);
  int s = *split_io;
  if (s <= 0) {
    const int bound = t->bm == 64 ? 800 : (t->bm == 128 ? 537 : 300);
    s = 1;
    while (nt * s * 2 <= bound && s < 8 && K / (2 * s) >= 512) s *= 2;
  }
  s = std::max(1, std::min(s, (K + kGemmBK - 1) / kGemmBK));
  // 3-stage LDS ring when the grid is too small for block-level latency hiding (measured: o/down
  // projections and the LM head at M <= 128 gain 10-20%; wide grids lose occupancy to its LDS)
  if (*tsel_io == 0 && nt * s <= (t->bm == 64 ? 600 : 256)) tsel |= kTileDepth3;
  *tsel_io = tsel | hint_bits;
  *split_io = s;
}

// how the output is finished: in the kernel, by the in-launch combine, as slabs left for the consumer, or by a
// splitk_reduce launch
enum class GemmFinish { kInKernel, kCombine, kSlabs, kReduce };

struct QkvFacts { int D; bool neox, rope; };
// qkv: the call carries the QKV epilogue (launch_gemm_qkv); aligned: the row strides of x and w are multiples of 8
// elements; tuned: the hints came from the tuned table
struct GemmProblem {
  int M, N, K;
  bool w_fp8, glu;
  int act;
  int64_t ws_bytes;
  bool has_out, partial_out, has_packed;
  const QkvFacts* qkv;
  bool aligned;
  int nt_hint, split_hint;
  bool tuned;
};
struct GemmExec {
  GemmFamily family = GemmFamily::kNone;  // kNone: nothing to launch (M == 0 or N == 0)
  int tile = 0, bm = 0, bn = 0, threads = 0;
  // depth: requested ring depth after the dispatch-level clamps; split: K split, workgroups per CU under kStreamK,
  // what a full 128-row panel takes under kStreamPanels
  int depth = 0, split = 1;
  GemmFinish finish = GemmFinish::kInKernel;
  bool wnt = false, ilv = false, packed = false;
  int nt = 0, variant = 0, sk_grid = 0, sk_maxseg = 0;  // kStream; kStreamK
  int counters = 0;                                     // arrival counters needed (combine, stream-K)
  int64_t ws_bytes = 0;                                 // workspace bytes needed
  bool qkv_cannot = false;         // the plan cannot take the QKV epilogue: run the plain GEMM + rope_cache
  // nt_hint: the hint in force (a tuned packed bit without a packed copy is cleared); nt_plan: the planner's
  // normalised hint, (tile | depth code | flags) << 8 or the streaming nt
  int nt_hint = 0, nt_plan = 0;
  const char* error = nullptr;     // gemm_resolve throws it
  bool split_out() const { return finish == GemmFinish::kSlabs || finish == GemmFinish::kReduce; }
};

inline void gemm_set_tile(GemmExec& e, GemmFamily f, const GemmTile& t, int code) {
  e.family = f, e.tile = code, e.bm = t.bm, e.bn = t.bn, e.threads = t.threads();
}
inline void gemm_set_split(GemmExec& e, int s, bool slabs_ok, int M, int N) {
  e.split = s;
  if (s <= 1) return;
  e.finish = slabs_ok ? GemmFinish::kSlabs : GemmFinish::kReduce;
  e.ws_bytes = (int64_t)s * M * N * 4;
}

// Resolves a problem and its hints to the launch. Never throws: an invalid combination comes back in `error`, with the
// fields the predictors (gemm_partial_slabs, gemm_plan) read still filled in.
inline GemmExec gemm_resolve_raw(const GemmProblem& p) {
  GemmExec e;
  const int M = p.M, N = p.N, K = p.K;
  if (M == 0 || N == 0) return e;
  const bool qkv = p.qkv != nullptr, f8 = p.w_fp8;
  const char *e_sel = nullptr, *e_k = nullptr, *e_glu = nullptr, *e_late = nullptr;
  int nt_hint = p.nt_hint;
  // packed weights: which weight pointer the launch reads
  if (gemm_hint_decode(nt_hint).packed) {
    if (!p.has_packed && p.tuned) nt_hint &= ~(kTilePacked << kHintTileShift);
    else if (!p.has_packed) e_sel = "gemm: the packed-weight hint (bit 2048) needs the packed copy of the weight";
    else if (f8) e_sel = "gemm: packed weights are bf16 only (no fp8 variant)";
    else if (M > 64) e_sel = "gemm: packed weights serve M <= 64 only";
    else if (nt_hint & kHintStream) e_sel = "gemm: the streaming kernels have no packed-weight variant";
  }
  const GemmHint h = gemm_hint_decode(nt_hint);
  const int raw = (int)((unsigned)nt_hint >> kHintTileShift);
  e.nt_hint = nt_hint;
  e.packed = h.packed;
  const GemmTile* ht = gemm_tile(h.tile, h.dec);
  if (K % 16 && !(K % 8 == 0 && !(nt_hint & kHintStream) && !h.streamk && (h.dec || (ht && ht->k8))))
    e_k = qkv ? "gemm_qkv: K must be a multiple of 16 (of 8 on gemm_dec / gemm_mid hints)"
              : "gemm: K must be a multiple of 16 (of 8 on gemm_dec / gemm_mid hints)";
  if (p.glu && (N % 32)) e_glu = "gemm: glu needs N % 32 == 0";
  const bool slabs_ok = p.partial_out && !p.glu && p.act == 0;
  auto done = [&](bool cannot = false) {
    e.qkv_cannot = cannot;
    const char* e_buf = !p.has_out && e.finish != GemmFinish::kSlabs
                            ? "gemm: this configuration writes the output, but no output buffer was given" : nullptr;
    if (qkv) e.error = e_k ? e_k : (e_sel ? e_sel : (cannot ? nullptr : e_late));
    else e.error = e_sel ? e_sel : (e_buf ? e_buf : (e_k ? e_k : (e_glu ? e_glu : e_late)));
    return e;
  };

  // weight-streaming kernel: M <= 16, explicit stream hints, and fp8 prefill panels; fp8 decode
  // (16 < M <= 128) runs the tiled kernel with fp8 weight tiles (W8A16); a QKV call streams on an explicit hint only
  if ((nt_hint & kHintStream) || (!qkv && !raw && (M <= 16 || (f8 && M > 128)))) {
    if (qkv) return done(true);  // streaming kernels have no LDS-staged epilogue
    int nt, s;
    gemm_stream_plan(std::min(M, 128), N, K, &nt, &s);
    if (h.nt > 0) nt = h.nt;
    if (p.split_hint > 0) s = p.split_hint;
    if (p.glu && nt < 2) nt = 2;  // the SwiGLU epilogue pairs (gate, up) 16-column tiles inside a wave
    e.nt = e.nt_plan = nt;
    e.variant = h.variant ? h.variant : 2;
    if (M > 128) {  // fp8 weights with many rows (prefill): 128-row panels, each resolved and finished on its own
      e.family = GemmFamily::kStreamPanels;
      e.split = s;
      return done();
    }
    e.family = GemmFamily::kStream;
    if ((int64_t)s * M * N * 4 > p.ws_bytes) s = 1;
    gemm_set_split(e, s, slabs_ok, M, N);
    return done();
  }

  if (h.dec) {  // K split over the waves (gemm_dec.hip), M <= 64, bf16 weights
    if (f8) e_late = "gemm_dec: bf16 weights only";
    else if (!ht) e_late = "gemm_dec: bad tile code";
    if (qkv && (M > 64 || !ht || (p.qkv->rope && p.qkv->neox && ht->bn % p.qkv->D))) return done(true);
    int s = std::max(1, std::min(p.split_hint, (K + 63) / 64));
    if ((int64_t)s * M * N * 4 > p.ws_bytes) s = 1;
    e.family = GemmFamily::kDec, e.tile = h.tile, e.bm = 64, e.bn = ht ? ht->bn : 0, e.threads = 256;
    e.depth = kDecDepth[h.depth_code];
    e.split = s;
    if (f8) return done();  // rejected: no slabs
    // in-launch combine: [tile][split][64 * bn] fp32 in the workspace; the QKV epilogue needs finished sums
    const int nt = ht ? (N + ht->bn - 1) / ht->bn : 0;
    if ((h.combine || qkv) && s > 1 && ht && (int64_t)nt * s * 64 * ht->bn * 4 <= p.ws_bytes) {
      e.finish = GemmFinish::kCombine, e.counters = nt, e.ws_bytes = (int64_t)nt * s * 64 * ht->bn * 4;
    } else if (qkv && s > 1) {
      return done(true);
    } else {
      gemm_set_split(e, s, slabs_ok, M, N);
    }
    return done();
  }

  int tsel = raw, s = p.split_hint;
  if (f8 && h.tile >= 5) tsel = (tsel & ~kTileCode) | 1;  // 8-wave and mid tiles are bf16-only
  gemm_tiled_plan(M, N, K, &tsel, &s, p.glu);
  e.nt_plan = (int)((unsigned)tsel << kHintTileShift);
  int ns = kTiledDepth[(tsel >> kTileDepthShift) & 3];
  const bool sk = (tsel & kTileStreamK) != 0;
  int tile = tsel & kTileCode;
  const GemmTile* t = gemm_planned_tile(tile);
  if (qkv) {
    if (!t->qkv || sk || (p.qkv->rope && p.qkv->neox && t->bn % p.qkv->D)) return done(true);
    if (s > 1 && (int64_t)tiles_of(M, N, t->bm, t->bn) * s * t->bm * t->bn * 4 > p.ws_bytes) return done(true);
  }
  if (h.packed && (tile < 7 || h.streamk))
    e_late = "gemm: this kernel has no packed-weight variant (gemm_dec and 64-row gemm_mid tiles only)";
  else if (h.packed && !t->packed)
    e_late = "gemm_mid: this tile has no packed-weight variant (64-row tiles only)";
  // the ping-pong kernel's zero-page K tail works on 8-element chunks and its LDS-DMA rows need 16-B aligned
  // strides, and it has no fp8-weight variant: anything else runs on the 128x128 tile
  if (tile == kPingPongTile && (K % 8 || !p.aligned || f8)) t = gemm_tile(tile = 1);
  if ((tile == 1 || tile == 5) && ns > 3) ns = 3;  // 128x128 / 256x128 x 4 stages exceed the 160 KiB LDS
  if ((tile == 2 || tile == 6) && ns > 4) ns = 4;
  e.depth = ns;
  e.wnt = !h.default_w && M <= t->bm;  // non-temporal weights when one workgroup row reads every weight tile
  if (tile == kPingPongTile) {
    gemm_set_tile(e, GemmFamily::kPingPong, *t, tile);
    return done();
  }
  if (sk && !f8) {  // tile < 5: the plan drops the bit on the others
    if (ns == 6) e.depth = 4;
    const int tiles = tiles_of(M, N, t->bm, t->bn), nk = (K + kGemmBK - 1) / kGemmBK;
    const int64_t U = (int64_t)tiles * nk;
    const int G = (int)std::min<int64_t>(U, 256LL * std::max(1, std::min(s, 8)));
    const int64_t per = U / std::max(G, 1);  // >= 1
    const int maxseg = (int)std::min<int64_t>(G, (nk + per - 1) / std::max<int64_t>(per, 1) + 1);
    if (U < (1LL << 31) && (int64_t)tiles * maxseg * t->bm * t->bn * 4 <= p.ws_bytes) {
      gemm_set_tile(e, GemmFamily::kStreamK, *t, tile);
      e.split = s, e.sk_grid = G, e.sk_maxseg = maxseg, e.counters = tiles;
      e.ws_bytes = (int64_t)tiles * maxseg * t->bm * t->bn * 4;
      return done();
    }
    e.depth = ns;
    s = 1;  // workspace too small for the partial tiles: plain tiled launch
  }
  gemm_set_tile(e, t->family, *t, tile);
  e.ilv = h.ilv && t->family == GemmFamily::kMid;
  const int nt = tiles_of(M, N, t->bm, t->bn);
  if ((h.combine || qkv) && s > 1 && (int64_t)nt * s * t->bm * t->bn * 4 <= p.ws_bytes) {
    e.split = s, e.finish = GemmFinish::kCombine, e.counters = nt, e.ws_bytes = (int64_t)nt * s * t->bm * t->bn * 4;
    return done();
  }
  if ((int64_t)s * M * N * 4 > p.ws_bytes) s = 1;
  // a stream-K bit that does not run stream-K (fp8 weights) splits by its workgroups-per-CU value and never
  // leaves slabs
  gemm_set_split(e, s, slabs_ok && !sk, M, N);
  return done();
}

inline GemmExec gemm_checked(const GemmExec& e) {
  if (e.error) throw std::runtime_error(e.error);
  return e;
}
inline GemmExec gemm_resolve(const GemmProblem& p) { return gemm_checked(gemm_resolve_raw(p)); }

// W8A8 (launch_gemm_f8f8): tile 0 = auto, 1-3 the fp8 x fp8 tiled kernel, 4 the 256x256 kernel, 7-15 the gemm_mid
// tiles; depth and split 0 = auto. Any other code sizes its grid as 64x128 and launches the 64x64 kernel.
// has_xs: per-token scales given; mx_in / mx_out: MX-fp8 activation scales (asc) / SwiGLU output (mxq);
// mx_out_dense: mxs given and ldy == N / 2
struct F8Problem {
  int M, N, K;
  bool glu;
  int act, tile, depth, split;
  int64_t ws_bytes;
  bool has_out, partial_out, has_xs, mx_in, mx_out, mx_out_dense;
};
inline GemmExec gemm_f8f8_resolve_raw(const F8Problem& p) {
  GemmExec e;
  const int M = p.M, N = p.N, K = p.K;
  if (M == 0 || N == 0) return e;
  auto err = [&](bool bad, const char* what) {
    if (bad && !e.error) e.error = what;
  };
  err(K % 16, "gemm_f8f8: K must be a multiple of 16");
  err(p.glu && (N % 32), "gemm_f8f8: glu needs N % 32 == 0");
  err(!p.has_out && !p.partial_out && !p.mx_out, "gemm_f8f8: output required");
  int tile = p.tile;
  const GemmTile* t = tile >= 1 && tile <= 15 ? gemm_tile(tile) : nullptr;
  const bool mid = t && t->family == GemmFamily::kMid;
  err(mid && K % 128, "gemm_f8f8: gemm_mid tiles need K % 128 == 0");
  err((p.mx_in || p.mx_out) && !mid, "gemm_f8f8: MX-fp8 activations need a gemm_mid tile (7-15)");
  err(p.mx_in && (p.has_xs || K % 128), "gemm_f8f8: MX scales replace xs; K % 128 == 0");
  err(p.mx_out && (!p.mx_out_dense || !p.glu || (t ? t->bn : 128) % 64 || N % 128 || p.partial_out),
      "gemm_f8f8: MX output needs SwiGLU, BN % 64 == 0, N % 128 == 0, dense rows, no slabs");
  if (tile == kPingPongTile || (tile == 0 && K % 128 == 0 && tiles_of(M, N, 256, 256) >= 192)) {
    err(K % 128, "gemm_f8f8: the 256x256 tile needs K % 128 == 0");
    gemm_set_tile(e, GemmFamily::kF8Big, *gemm_tile(kPingPongTile), kPingPongTile);
    return e;
  }
  if (tile == 0) {  // auto: 128x128 when it fills the chip, else 64x128 / 64x64, split to >= ~256 WGs
    tile = tiles_of(M, N, 128, 128) >= 240 ? 1 : (tiles_of(M, N, 64, 128) >= 240 ? 2 : 3);
    t = gemm_tile(tile);
  }
  const bool known = t && t->family != GemmFamily::kWide8;
  e.family = mid ? GemmFamily::kMid : GemmFamily::kF8Tiled, e.tile = tile;
  e.bm = known ? t->bm : 64, e.bn = known ? t->bn : 128, e.threads = mid ? t->threads() : 256;
  const int tiles = tiles_of(M, N, e.bm, e.bn), nk = (K + kGemmBK8 - 1) / kGemmBK8;
  int split = p.split;
  if (split <= 0) {
    split = 1;
    while (tiles * split * 2 <= 512 && nk / (2 * split) >= 4 && split < 8) split *= 2;
  }
  split = std::max(1, std::min(split, nk));
  if ((int64_t)split * M * N * 4 > p.ws_bytes) split = 1;
  err(p.mx_out && split > 1, "gemm_f8f8: an MX-fp8 SwiGLU output cannot be split over K");
  e.depth = p.depth <= 0 ? (tile == 1 ? 3 : 4) : p.depth;
  if (tile == 1 && e.depth > 3) e.depth = 3;
  e.wnt = M <= e.bm;
  gemm_set_split(e, split, p.partial_out && !p.glu && p.act == 0, M, N);
  err(e.finish == GemmFinish::kReduce && !p.has_out, "gemm_f8f8: output required");
  return e;
}
inline GemmExec gemm_f8f8_resolve(const F8Problem& p) { return gemm_checked(gemm_f8f8_resolve_raw(p)); }

// Autotuned plans: (M, N, K, glu, kind) -> (nt_hint, split) measured by llmss_amd/ops/autotune.py for the shapes an
// engine will actually run (decode batch buckets x layer GEMMs). Consulted by every call without explicit hints and
// by the predictors below, so split-K partial fusion stays consistent.
// kind: 0 = bf16 [N, K] weights, 1 = fp8 weights, 3 = QKV RoPE / KV-write epilogue (launch_gemm_qkv)
inline std::mutex g_tuned_mu;
inline std::unordered_map<uint64_t, std::pair<int, int>> g_tuned;
inline uint64_t gemm_tune_key(int M, int N, int K, bool glu, int kind) {
  return ((uint64_t)(kind & 7) << 61) | ((uint64_t)(M & 0x7FFFF) << 42) | ((uint64_t)N << 22) |
         ((uint64_t)K << 2) | (glu ? 2u : 0u) | (kind == 1 ? 1u : 0u);
}
inline void gemm_tuned_set(int M, int N, int K, bool glu, int kind, int nt_hint, int split) {
  std::lock_guard<std::mutex> lk(g_tuned_mu);
  g_tuned[gemm_tune_key(M, N, K, glu, kind)] = {nt_hint, split};
}
inline void gemm_tuned_clear() {
  std::lock_guard<std::mutex> lk(g_tuned_mu);
  g_tuned.clear();
}
inline bool gemm_tuned_get(int M, int N, int K, bool glu, int kind, int* nt_hint, int* split) {
  std::lock_guard<std::mutex> lk(g_tuned_mu);
  auto it = g_tuned.find(gemm_tune_key(M, N, K, glu, kind));
  if (it == g_tuned.end()) return false;
  *nt_hint = it->second.first;
  *split = it->second.second;
  return true;
}

// Number of fp32 partial slabs launch_gemm(..., partial_out=true) leaves for these hints, or 0 if that call writes
// the finished output. The Python wrapper allocates Y exactly when this returns 0.
inline int gemm_partial_slabs(int M, int N, int K, bool w_fp8, bool glu, int act, int nt_hint, int split_hint,
                              int64_t ws_bytes) {
  bool tuned = false;
  if (nt_hint == 0 && split_hint == 0) tuned = gemm_tuned_get(M, N, K, glu, w_fp8 ? 1 : 0, &nt_hint, &split_hint);
  const GemmExec e = gemm_resolve_raw({M, N, K, w_fp8, glu, act, ws_bytes, true, true, true, nullptr, true, nt_hint,
                                       split_hint, tuned});
  return e.finish == GemmFinish::kSlabs ? e.split : 0;
}
// the split a W8A8 call with these arguments leaves as slabs under partial_out (0 = finished output)
inline int gemm_f8f8_partial_slabs(int M, int N, int K, bool glu, int act, int tile, int split, int64_t ws_bytes) {
  const GemmExec e = gemm_f8f8_resolve_raw({M, N, K, glu, act, tile, 0, split, ws_bytes, true, true, true, false,
                                            false, false});
  return e.finish == GemmFinish::kSlabs ? e.split : 0;
}
// the plan a call without hints runs, as (nt_hint, K split: 1 where the launch combines its slices itself); a tuned
// streaming entry is reported as stored
inline void gemm_plan(int M, int N, int K, bool w_fp8, int* nt, int* splitk) {
  int th = 0, ts = 0;
  const bool tuned = gemm_tuned_get(M, N, K, false, w_fp8 ? 1 : 0, &th, &ts);
  const GemmExec e = gemm_resolve_raw({M, N, K, w_fp8, false, 0, INT64_MAX, true, true, true, nullptr, true, th, ts,
                                       tuned});
  *nt = tuned ? th : e.nt_plan;
  if (tuned && !((unsigned)th >> kHintTileShift)) *splitk = ts;
  else *splitk = e.finish == GemmFinish::kCombine || e.finish == GemmFinish::kReduce || e.family == GemmFamily::kStreamK
                     ? 1 : e.split;
}
