// Token constraints on LM logits: logit_bias, banned / allowed tokens and min_tokens as one sparse per-request edit
// of the logits row between the LM head (and the penalties) and the sampler.
//
// State, owned by the engine and constant while a sequence runs (S constraint slots, E = MAX_TOKEN_EDITS):
//   edit_ids  [S, 2, E] int32   distinct global token ids; list 0 = early, list 1 = late
//   edit_vals [S, 2, E] fp32    -inf (the token is forbidden) or a finite bias
//   edit_meta [S, 4]    int32   (n_early, n_late, fill, min_tokens)
// (each with its own slot stride, so that a slot's three rows can lie in one block that one copy fills)
// Row b with slot s = slots[b] >= 0 uses the early list iff nout[b] < min_tokens (the stop set is forced out until
// the sequence has generated min_tokens tokens), else the late one. For column j (global token v = lo + j):
//
//   v >= vocab (head padding)      out = in, bit for bit
//   v listed with -inf             out = -inf
//   v listed with a finite a       out = round-to-nearest-even(float(in) + a) in the logits' dtype
//   v not listed                   out = fill ? -inf : in      (fill: the request has an allowed set)
//
// Rows with slot -1 are copied bit for bit. The output is a separate buffer: the raw logits stay for the
// log-probability launch.
//
// One launch, two phases per workgroup, no atomics and no ordering between workgroups. A row is cut over gridDim.x
// workgroups of CON_GROUPS 8-column groups (64 rows of a 32,000-token vocabulary: 1,024 workgroups for the 256 CUs);
// the columns before the first 16-B boundary of the input row and after the last full group belong to the row's first
// workgroup. Phase 1: the workgroup writes its own columns - the copy, or -inf below `vocab` for a filled row - a
// thread moving 8 columns per step with one 16-B load and store (two for fp32); where the output row does not share
// the input row's alignment the stores go column by column. Then __syncthreads(). Phase 2: the workgroup's threads
// stride over the row's active list (at most E entries) and store the entries whose column the same workgroup wrote
// in phase 1. Entries outside [lo, lo + W) or at or past `vocab` are skipped (another rank's shard). So every output
// column is written by one workgroup, and a listed column's second store comes after that workgroup's barrier.
#include "common.h"

#include <cmath>

constexpr int CON_T = 256;
constexpr int CON_GROUPS = 256;  // 8-column groups per workgroup

template <typename T>
__device__ __forceinline__ T con_ninf() {
  if constexpr (sizeof(T) == 2) return (T)0xFF80;
  else return -INFINITY;
}

template <typename T>
__device__ __forceinline__ T con_add(T x, float a) {
  if constexpr (sizeof(T) == 2) return f2bf(bf2f(x) + a);
  else return x + a;
}

template <typename T>
__global__ __launch_bounds__(CON_T) void apply_token_edits_kernel(
    const T* __restrict__ logits, int64_t ld, T* __restrict__ out, int64_t ldo, int W, int lo, int vocab,
    const int* __restrict__ edit_ids, int64_t ld_ids, const float* __restrict__ edit_vals, int64_t ld_vals,
    const int* __restrict__ edit_meta, int64_t ld_meta, int nslots, int E, const int* __restrict__ slots,
    const int* __restrict__ nout) {
  constexpr int UNIT = 16 / sizeof(T);  // elements per 16 B
  const int b = blockIdx.y;
  const T* in = logits + (int64_t)b * ld;
  T* o = out + (int64_t)b * ldo;
  const int slot = slots[b];
  const bool held = slot >= 0 && slot < nslots;
  int n = 0, list = 0;
  bool fill = false;
  if (held) {
    const int* meta = edit_meta + (int64_t)slot * ld_meta;
    list = nout[b] < meta[3] ? 0 : 1;
    n = min(max(meta[list], 0), E);
    fill = meta[2] != 0;
  }
  const T ninf = con_ninf<T>();
  // columns [0, head) up to the first 16-B boundary of the input row, then full groups of 8, then the tail
  const int ai = (int)(((uintptr_t)in / sizeof(T)) % UNIT), ao = (int)(((uintptr_t)o / sizeof(T)) % UNIT);
  const int head = min((UNIT - ai) % UNIT, W);
  const bool wide = ai == ao;  // the output row shares the input row's 16-B phase
  const int ngroups = (W - head) / 8;
  const int tail0 = head + ngroups * 8;

  // ---- phase 1: this workgroup's columns
  if (blockIdx.x == 0) {
    const int nloose = head + (W - tail0);
    for (int i = threadIdx.x; i < nloose; i += CON_T) {
      const int j = i < head ? i : tail0 + (i - head);
      o[j] = (fill && lo + j < vocab) ? ninf : in[j];
    }
  }
  const int g1 = min(ngroups, (int)(blockIdx.x + 1) * CON_GROUPS);
  for (int g = blockIdx.x * CON_GROUPS + threadIdx.x; g < g1; g += CON_T) {
    const int j = head + g * 8, v = lo + j;
    alignas(16) T x[8];
    if constexpr (sizeof(T) == 2) {
      *reinterpret_cast<u16x8*>(x) = *reinterpret_cast<const u16x8*>(in + j);
    } else {
      *reinterpret_cast<f32x4*>(x) = *reinterpret_cast<const f32x4*>(in + j);
      *reinterpret_cast<f32x4*>(x + 4) = *reinterpret_cast<const f32x4*>(in + j + 4);
    }
    if (fill) {
#pragma unroll
      for (int i = 0; i < 8; ++i)
        if (v + i < vocab) x[i] = ninf;
    }
    if (wide) {
      if constexpr (sizeof(T) == 2) {
        *reinterpret_cast<u16x8*>(o + j) = *reinterpret_cast<const u16x8*>(x);
      } else {
        *reinterpret_cast<f32x4*>(o + j) = *reinterpret_cast<const f32x4*>(x);
        *reinterpret_cast<f32x4*>(o + j + 4) = *reinterpret_cast<const f32x4*>(x + 4);
      }
    } else {
#pragma unroll
      for (int i = 0; i < 8; ++i) o[j + i] = x[i];
    }
  }
  if (n == 0) return;  // uniform over the workgroup
  __syncthreads();     // this workgroup's phase-1 stores are done before its edits: no other workgroup writes them

  // ---- phase 2: the listed tokens whose column this workgroup wrote
  const int* ids = edit_ids + (int64_t)slot * ld_ids + (int64_t)list * E;
  const float* vals = edit_vals + (int64_t)slot * ld_vals + (int64_t)list * E;
  for (int i = threadIdx.x; i < n; i += CON_T) {
    const int id = ids[i];
    if (id < lo || id >= vocab) continue;
    const int j = id - lo;
    if (j >= W) continue;
    const int owner = (j < head || j >= tail0) ? 0 : ((j - head) / 8) / CON_GROUPS;
    if (owner != (int)blockIdx.x) continue;
    const float a = vals[i];
    o[j] = (a == -INFINITY) ? ninf : con_add<T>(in[j], a);
  }
}

void launch_apply_token_edits(const void* logits, int64_t ld, void* out, int64_t ldo, bool fp32, int B, int W, int lo,
                              int vocab, const void* edit_ids, int64_t ld_ids, const void* edit_vals,
                              int64_t ld_vals, const void* edit_meta, int64_t ld_meta, int nslots, int E,
                              const void* slots, const void* nout, hipStream_t st) {
  if (B == 0 || W == 0) return;  // nothing to write: the state never changes in a launch
  if (B < 0 || B > 65535 || W < 0 || lo < 0 || vocab < 0 || nslots < 0 || E < 0 || (int64_t)lo + W > INT32_MAX ||
      ld_ids < 2 * (int64_t)E || ld_vals < 2 * (int64_t)E || ld_meta < 4)
    throw std::runtime_error("apply_token_edits: bad B / W / lo / vocab / state shape");
  const int chunks = std::max(1, (W / 8 + CON_GROUPS - 1) / CON_GROUPS);
#define CONK(T_)                                                                                                    \
  apply_token_edits_kernel<T_><<<dim3(chunks, B), CON_T, 0, st>>>(                                                   \
      (const T_*)logits, ld, (T_*)out, ldo, W, lo, vocab, (const int*)edit_ids, ld_ids, (const float*)edit_vals,     \
      ld_vals, (const int*)edit_meta, ld_meta, nslots, E, (const int*)slots, (const int*)nout)
  if (fp32) CONK(float);
  else CONK(bf16_t);
#undef CONK
  HIP_CHECK_LAUNCH();
}
