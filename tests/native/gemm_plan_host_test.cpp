// The GEMM plan resolver (csrc/gemm_plan.h) alone under AddressSanitizer + UndefinedBehaviorSanitizer: every hint of
// the decoder's field space and a few thousand fixed-seed random 32-bit hints over small problems. Each call either
// throws std::runtime_error or returns a plan a launcher can run: real tile dims, split >= 1, no more workspace than
// given, slabs only where the caller can consume them, packed weights only where a kernel reads them.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../llmss_amd/csrc/gemm_plan.h"

static long g_resolved = 0, g_thrown = 0;
#define CHECK(c)                                                                                   \
  do {                                                                                             \
    if (!(c)) {                                                                                    \
      std::printf("FAILED %s (line %d): M %d N %d K %d fp8 %d glu %d act %d ws %lld nt %#x split %d qkv %d\n", #c, \
                  __LINE__, p.M, p.N, p.K, p.w_fp8, p.glu, p.act, (long long)p.ws_bytes, (unsigned)p.nt_hint,      \
                  p.split_hint, p.qkv != nullptr);                                                 \
      std::exit(1);                                                                                \
    }                                                                                              \
  } while (0)

static void check(const GemmProblem& p) {
  GemmExec e;
  try {
    e = gemm_resolve(p);
  } catch (const std::runtime_error&) {
    ++g_thrown;
    return;
  }
  ++g_resolved;
  CHECK(!e.error);
  CHECK(!e.qkv_cannot || p.qkv);
  if (e.qkv_cannot) return;
  CHECK((e.family == GemmFamily::kNone) == (p.M == 0 || p.N == 0));
  if (e.family == GemmFamily::kNone) return;
  if (e.family == GemmFamily::kStream || e.family == GemmFamily::kStreamPanels) {
    CHECK(e.nt >= 1 && e.variant >= 1);
    CHECK((e.family == GemmFamily::kStream) == (p.M <= 128));
  } else {
    CHECK(e.bm > 0 && e.bn > 0 && e.threads > 0 && e.tile >= 0);
    CHECK(e.family == GemmFamily::kPingPong || e.depth >= 2);
  }
  CHECK(e.split >= 1);
  CHECK(e.ws_bytes >= 0 && e.ws_bytes <= p.ws_bytes);
  CHECK(e.finish != GemmFinish::kSlabs || (p.partial_out && !p.glu && p.act == 0));
  CHECK(p.has_out || e.finish == GemmFinish::kSlabs);
  CHECK((e.counters > 0) == (e.finish == GemmFinish::kCombine || e.family == GemmFamily::kStreamK));
  CHECK(e.split > 1 || e.finish == GemmFinish::kInKernel);
  if (e.packed) {
    const GemmTile* t = gemm_tile(e.tile, e.family == GemmFamily::kDec);
    CHECK(e.family == GemmFamily::kDec || e.family == GemmFamily::kMid);
    CHECK(t && t->packed && p.M <= 64 && !p.w_fp8 && p.has_packed);
  }
  if (p.qkv) CHECK(e.finish == GemmFinish::kInKernel || e.finish == GemmFinish::kCombine);
}

static void check_f8(const F8Problem& q) {
  GemmExec e;
  try {
    e = gemm_f8f8_resolve(q);
  } catch (const std::runtime_error&) {
    ++g_thrown;
    return;
  }
  ++g_resolved;
  const GemmProblem p{q.M, q.N, q.K, true, q.glu, q.act, q.ws_bytes, q.has_out, q.partial_out, false, nullptr, true,
                      q.tile, q.split, false};  // for the failure message
  CHECK((e.family == GemmFamily::kNone) == (q.M == 0 || q.N == 0));
  if (e.family == GemmFamily::kNone) return;
  CHECK(e.bm > 0 && e.bn > 0 && e.threads > 0 && e.split >= 1);
  CHECK(e.ws_bytes <= q.ws_bytes);
  CHECK(e.finish != GemmFinish::kSlabs || (q.partial_out && !q.glu && q.act == 0));
  CHECK(e.finish != GemmFinish::kReduce || q.has_out);
  CHECK(!q.mx_out || e.split == 1);
}

int main() {
  const int Ms[] = {0, 1, 16, 17, 33, 64, 65, 128, 129, 300}, Ns[] = {0, 1, 16, 32, 48, 96, 256, 1000};
  const int Ks[] = {0, 1, 8, 24, 64, 72, 128, 1024}, splits[] = {0, 1, 2, 3, 8, 1000, -5};
  const int64_t WSs[] = {0, 1 << 20, (int64_t)256 << 20};
  const QkvFacts qfs[] = {{16, true, true}, {64, true, true}, {64, false, true}, {128, true, false}};
  uint64_t rng = 0x9E3779B97F4A7C15ull;  // fixed seed (splitmix-style step)
  auto next = [&]() {
    rng += 0x9E3779B97F4A7C15ull;
    uint64_t z = rng;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
  };
  auto problems = [&](int nt_hint, int count) {
    for (int i = 0; i < count; ++i) {
      const uint64_t r = next();
      GemmProblem p{};
      p.M = Ms[r % 10];
      p.N = Ns[(r >> 4) % 8];
      p.K = Ks[(r >> 8) % 8];
      p.w_fp8 = (r >> 12) % 4 == 0;
      p.glu = (r >> 14) % 4 == 0;
      p.act = (r >> 16) % 4 == 0 ? 1 : 0;
      p.ws_bytes = WSs[(r >> 18) % 3];
      p.partial_out = (r >> 22) % 2;
      p.has_packed = (r >> 23) % 2;
      p.qkv = (r >> 24) % 4 == 0 ? &qfs[(r >> 26) % 4] : nullptr;
      p.has_out = p.qkv || (r >> 20) % 4 != 0;  // a QKV call always has its output buffer
      p.aligned = (r >> 28) % 4 != 0;
      p.nt_hint = nt_hint;
      p.split_hint = (r >> 30) % 8 == 7 ? (int)(uint32_t)(r >> 32) : splits[(r >> 30) % 7];
      p.tuned = (r >> 34) % 2;
      check(p);
    }
  };
  // the field space: every streaming byte; every tile field (code, depth, default-w, stream-K, combine, ilv, dec,
  // packed), alone, with a streaming byte, and under the W8A8 bit
  for (int lo = 0; lo < 256; ++lo) problems(lo, 16);
  for (int field = 0; field < 4096; ++field)
    for (int extra : {0, 17, kHintW8A8}) problems((field << kHintTileShift) | extra, 8);
  for (int i = 0; i < 4000; ++i) problems((int)(uint32_t)next(), 8);

  for (int tile = -2; tile <= 17; ++tile)
    for (int M : Ms)
      for (int N : Ns)
        for (int K : Ks)
          for (int split : splits)
            for (int64_t ws : WSs) {
              const uint64_t r = next();
              check_f8({M, N, K, r % 4 == 0, (r >> 2) % 4 == 0 ? 1 : 0, tile, (int)((r >> 4) % 8) - 1, split, ws,
                        (r >> 8) % 4 != 0, (r >> 10) % 2 == 0, (r >> 11) % 2 == 0, (r >> 12) % 8 == 0,
                        (r >> 15) % 8 == 0, (r >> 18) % 2 == 0});
            }
  std::printf("%ld plans resolved, %ld rejected\nALL OK\n", g_resolved, g_thrown);
  return g_resolved > 100000 && g_thrown > 10000 ? 0 : 1;
}
