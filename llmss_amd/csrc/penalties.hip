// Repetition, presence and frequency penalties on LM logits, with the token history kept on the device.
//
// State: one int32 word per (penalty slot, token): bit 31 = "occurs in the prompt", bits 0..30 = how often the
// token occurs in the output so far. For row b with slot s = slots[b] >= 0 and column j (global token v = lo + j,
// v < vocab), in fp32 and in this order:
//
//   w = state[s][v], plus one output occurrence when v == new_tokens[b]
//   x = float(logits[b][j])
//   if (w != 0)       x = x > 0 ? x / rep[b] : x * rep[b]          (seen in prompt or output)
//   c = w & 0x7fffffff
//   if (c > 0)        x = x - (freq[b] * float(c) + pres[b])       (output occurrences only)
//   out[b][j] = round-to-nearest-even(x) in the logits' dtype
//
// Rows with slot -1, columns with v >= vocab (head padding) and every word that is 0 copy their logit bit for bit.
// The output is a separate buffer: the raw logits stay for the log-probability launch.
//
// Registering new_tokens[b] and applying happen in one launch, without atomics or ordering between workgroups:
// every state word is read and written by one thread. When lo <= token < lo + W that is the thread that owns the
// token's column - it applies count + 1 and stores the word back. Otherwise (the token lies in another rank's
// vocabulary shard) nobody reads the word in this launch and thread 0 of the row's first workgroup increments it.
// The caller gives every row of a launch a different slot.
//
// Memory-bound and elementwise: a thread moves 8 columns per step - one 16-B load and store of logits (two for
// fp32) and two 16-B loads of state words. The columns before the first 16-B boundary of the logits row and after
// the last full group are done one by one by the row's first workgroup; state words whose address is not 16-B
// aligned (lo, the row base) are loaded one by one inside the group. A row is cut over gridDim.x workgroups of
// PEN_GROUPS 8-column groups, so 64 rows of a 32,000-token vocabulary make 1,024 workgroups for the 256 CUs.
//
// penalty_reset_kernel (re)builds whole rows from the host's list of distinct tokens and finished words: each
// workgroup zeroes its column chunk of the row, barriers, then stores the listed words that fall in its chunk.
#include "common.h"

typedef int __attribute__((ext_vector_type(4))) i32x4;

constexpr int PEN_T = 256;
constexpr int PEN_GROUPS = 256;       // 8-column groups per workgroup
constexpr int PEN_RESET_COLS = 4096;  // state words per reset workgroup (a multiple of 4)

__device__ __forceinline__ float pen_apply(float x, int w, float r, float p, float f) {
  if (w != 0) x = x > 0.f ? x / r : x * r;
  const int c = w & 0x7fffffff;
  if (c > 0) x = x - (f * (float)c + p);
  return x;
}

template <typename T>
__device__ __forceinline__ float pen_ld(const T* p) {
  if constexpr (sizeof(T) == 2) return bf2f(*p);
  else return *p;
}

template <typename T>
__device__ __forceinline__ void pen_st(T* p, float x) {
  if constexpr (sizeof(T) == 2) *p = f2bf(x);
  else *p = x;
}

// One column: the word (registering `tok` when it is this column's token), the penalty, the store.
template <typename T>
__device__ __forceinline__ void pen_one(const T* in, T* out, int* srow, int j, int lo, int vocab, int tok, float r,
                                        float p, float f) {
  const int v = lo + j;
  if (srow == nullptr || v >= vocab) {
    out[j] = in[j];
    return;
  }
  int w = srow[v];
  if (v == tok) srow[v] = ++w;
  if (w == 0) out[j] = in[j];
  else pen_st<T>(out + j, pen_apply(pen_ld<T>(in + j), w, r, p, f));
}

template <typename T>
__global__ __launch_bounds__(PEN_T) void apply_penalties_kernel(
    const T* __restrict__ logits, int64_t ld, T* __restrict__ out, int64_t ldo, int W, int lo, int vocab,
    int* __restrict__ state, int64_t lds, int nslots, const int* __restrict__ slots,
    const int64_t* __restrict__ new_tokens, const float* __restrict__ rep, const float* __restrict__ pres,
    const float* __restrict__ freq) {
  constexpr int UNIT = 16 / sizeof(T);  // elements per 16 B
  const int b = blockIdx.y;
  const T* in = logits + (int64_t)b * ld;
  T* o = out + (int64_t)b * ldo;
  const int slot = slots[b];
  int* srow = slot >= 0 && slot < nslots ? state + (int64_t)slot * lds : nullptr;
  const float r = rep[b], p = pres[b], f = freq[b];
  int tok = -1;
  if (srow) {
    const int64_t t = new_tokens[b];
    tok = (t >= 0 && t < vocab) ? (int)t : -1;
  }
  // columns [0, head) up to the first 16-B boundary of the input row; the output row must share it, else the
  // whole row goes column by column
  const int ai = (int)(((uintptr_t)in / sizeof(T)) % UNIT), ao = (int)(((uintptr_t)o / sizeof(T)) % UNIT);
  int head = (UNIT - ai) % UNIT;
  if (ai != ao || head > W) head = W;
  const int ngroups = (W - head) / 8;
  const int tail0 = head + ngroups * 8;

  if (blockIdx.x == 0) {
    const int nloose = head + (W - tail0);
    for (int i = threadIdx.x; i < nloose; i += PEN_T)
      pen_one<T>(in, o, srow, i < head ? i : tail0 + (i - head), lo, vocab, tok, r, p, f);
    // a token of another shard: nobody reads its word in this launch
    if (threadIdx.x == 0 && tok >= 0 && (tok < lo || tok >= lo + W)) srow[tok] += 1;
  }

  const int g1 = min(ngroups, (int)(blockIdx.x + 1) * PEN_GROUPS);
  for (int g = blockIdx.x * PEN_GROUPS + threadIdx.x; g < g1; g += PEN_T) {
    const int j = head + g * 8, v = lo + j;
    alignas(16) T xin[8];
    if constexpr (sizeof(T) == 2) {
      *reinterpret_cast<u16x8*>(xin) = *reinterpret_cast<const u16x8*>(in + j);
    } else {
      *reinterpret_cast<f32x4*>(xin) = *reinterpret_cast<const f32x4*>(in + j);
      *reinterpret_cast<f32x4*>(xin + 4) = *reinterpret_cast<const f32x4*>(in + j + 4);
    }
    if (srow != nullptr && v < vocab) {
      alignas(16) int w[8];
      if (v + 8 <= vocab && (uintptr_t)(srow + v) % 16 == 0) {
        *reinterpret_cast<i32x4*>(w) = *reinterpret_cast<const i32x4*>(srow + v);
        *reinterpret_cast<i32x4*>(w + 4) = *reinterpret_cast<const i32x4*>(srow + v + 4);
      } else {
#pragma unroll
        for (int i = 0; i < 8; ++i) w[i] = v + i < vocab ? srow[v + i] : 0;
      }
      if (tok >= v && tok < v + 8) {  // this thread owns the new token's word
        const int i = tok - v;
        int nw = 0;
#pragma unroll
        for (int e = 0; e < 8; ++e)
          if (e == i) nw = ++w[e];
        srow[tok] = nw;
      }
#pragma unroll
      for (int i = 0; i < 8; ++i)
        if (w[i] != 0) pen_st<T>(xin + i, pen_apply(pen_ld<T>(xin + i), w[i], r, p, f));
    }
    if constexpr (sizeof(T) == 2) {
      *reinterpret_cast<u16x8*>(o + j) = *reinterpret_cast<const u16x8*>(xin);
    } else {
      *reinterpret_cast<f32x4*>(o + j) = *reinterpret_cast<const f32x4*>(xin);
      *reinterpret_cast<f32x4*>(o + j + 4) = *reinterpret_cast<const f32x4*>(xin + 4);
    }
  }
}

__global__ __launch_bounds__(PEN_T) void penalty_reset_kernel(int* __restrict__ state, int64_t lds, int nslots,
                                                              int width,
                                                              const int* __restrict__ slots,
                                                              const int* __restrict__ cu, int ntok,
                                                              const int64_t* __restrict__ tokens,
                                                              const int* __restrict__ words) {
  const int slot = slots[blockIdx.y];
  if (slot < 0 || slot >= nslots) return;
  int* srow = state + (int64_t)slot * lds;
  const int c0 = blockIdx.x * PEN_RESET_COLS, c1 = min(width, c0 + PEN_RESET_COLS);
  if ((uintptr_t)srow % 16 == 0) {  // c0 is a multiple of 4
    const int n4 = (c1 - c0) / 4;
    for (int i = threadIdx.x; i < n4; i += PEN_T) *reinterpret_cast<i32x4*>(srow + c0 + 4 * i) = i32x4{0, 0, 0, 0};
    for (int c = c0 + 4 * n4 + threadIdx.x; c < c1; c += PEN_T) srow[c] = 0;
  } else {
    for (int c = c0 + threadIdx.x; c < c1; c += PEN_T) srow[c] = 0;
  }
  __syncthreads();  // this workgroup's zeroes are done before its words: no other workgroup touches the chunk
  const int i1 = min(cu[blockIdx.y + 1], ntok);
  for (int i = max(cu[blockIdx.y], 0) + threadIdx.x; i < i1; i += PEN_T) {
    const int64_t t = tokens[i];
    if (t >= c0 && t < c1) srow[t] = words[i];
  }
}

void launch_apply_penalties(const void* logits, int64_t ld, void* out, int64_t ldo, bool fp32, int B, int W, int lo,
                            int vocab, void* state, int64_t lds, int nslots, const void* slots,
                            const void* new_tokens,
                            const void* rep, const void* pres, const void* freq, hipStream_t st) {
  if (B == 0) return;  // W == 0 still launches: a shard without columns registers its rows' tokens
  if (B < 0 || B > 65535 || W < 0 || lo < 0 || vocab < 0 || vocab > lds)
    throw std::runtime_error("apply_penalties: bad B / W / lo / vocab");
  const int chunks = std::max(1, (W / 8 + PEN_GROUPS - 1) / PEN_GROUPS);
#define PENK(T_)                                                                                                   \
  apply_penalties_kernel<T_><<<dim3(chunks, B), PEN_T, 0, st>>>(                                                    \
      (const T_*)logits, ld, (T_*)out, ldo, W, lo, vocab, (int*)state, lds, nslots, (const int*)slots,              \
      (const int64_t*)new_tokens, (const float*)rep, (const float*)pres, (const float*)freq)
  if (fp32) PENK(float);
  else PENK(bf16_t);
#undef PENK
  HIP_CHECK_LAUNCH();
}

void launch_penalty_reset(void* state, int64_t lds, int nslots, int width, const void* slots, int R, const void* cu,
                          int ntok, const void* tokens, const void* words, hipStream_t st) {
  if (R == 0 || width == 0) return;
  if (R < 0 || R > 65535 || width < 0 || width > lds) throw std::runtime_error("penalty_reset: bad R / width");
  const int chunks = (width + PEN_RESET_COLS - 1) / PEN_RESET_COLS;
  penalty_reset_kernel<<<dim3(chunks, R), PEN_T, 0, st>>>((int*)state, lds, nslots, width, (const int*)slots,
                                                          (const int*)cu, ntok,
                                                          (const int64_t*)tokens, (const int*)words);
  HIP_CHECK_LAUNCH();
}
