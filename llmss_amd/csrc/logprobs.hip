// Per-token log-probabilities of the raw model distribution: for each row of LM logits, the
// log-softmax value of one chosen token and the N most likely tokens with theirs (N <= 20).
//
//   lp[b]        = x[tok_b] - max - log(sum exp(x - max))        over columns [0, V)
//   top_ids[b,:] = the N columns with the largest logits, logit descending, ties by ascending id
//
// One 256-thread workgroup per row (and per column shard, below), a separate launch after the sampler.
//   pass 1 (memory): per-thread maxima -> row max. The N-th largest of the 256 thread maxima is a floor
//           under the row's N-th largest value (each maximum is a distinct element), so everything below it
//           can be ignored by the selection: a few dozen elements survive on a real row.
//   pass 2 (L2): sum exp(x - max); the elements at or above the floor are gathered into LDS.
//   select: the N-th largest key by radix select (11 + 11 + 10 bits of the order-preserving key that the
//           sampler uses; integer counts, so the result does not depend on the order of the atomics), over the
//           gathered elements - or over the row again when more than LP_CAP survive the floor (rows of ties).
//           Elements above that key plus the lowest-id ties at it are ranked in LDS by (value desc, id asc).
// Selection compares stored values only. Max and sum are reduced in a fixed order (8-element tree per 16-B
// chunk, per-thread serial over chunks, xor-shuffle tree, 4 wave partials as a tree; no float atomics): the same
// input gives the same bits on every run and every tensor-parallel rank. The longest chain of the sum is
// ceil(V / 2048) + 11 additions.
//
// Partial mode (vocab-parallel heads): the row is a [B, width] shard whose column 0 is global token `lo`,
// optionally cut into gridDim.y column shards by one launch. Each (row, shard) emits a pack of 3 + 2N floats:
// shard max, shard sum exp(x - max), the chosen token's raw logit (-inf when it lies elsewhere), N raw logits and
// N global ids as int bits (-inf / -1 past the shard's width). logprobs_combine_kernel merges gathered packs.
#include "common.h"

constexpr int LP_T = 256;
constexpr int LP_BINS = 2048;
constexpr int LP_CAP = 2048;     // gathered elements the LDS selection takes
constexpr int LP_MAXN = 20;      // MAX_TOP_LOGPROBS
constexpr int LP_MAXCAND = 2048; // combine: groups * N

// sampling.hip's fkey (order-preserving ascending uint key of a float), with -0 read as +0 so that keys order
// exactly as float comparison does
__device__ __forceinline__ unsigned lp_key(float f) {
  unsigned u = __float_as_uint(f);
  u = u == 0x80000000u ? 0u : u;
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

template <typename T>
__device__ __forceinline__ float lp_load(const T* p, int i) {
  if constexpr (sizeof(T) == 2) return bf2f(p[i]);
  else return p[i];
}

template <typename T>
__device__ __forceinline__ void lp_load8(const T* p, float (&v)[8]) {
  if constexpr (sizeof(T) == 2) {
    const u16x8 x = *reinterpret_cast<const u16x8*>(p);
#pragma unroll
    for (int i = 0; i < 8; ++i) v[i] = bf2f(x[i]);
  } else {
    const f32x4 a = *reinterpret_cast<const f32x4*>(p), b = *reinterpret_cast<const f32x4*>(p + 4);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      v[i] = a[i];
      v[4 + i] = b[i];
    }
  }
}

// Every element of row[0, n): f8(v[8], j0) per aligned 16-B chunk when `vec`, f1(x, j) for the tail and for
// unaligned rows. A thread's elements come in ascending j.
template <typename T, typename F8, typename F1>
__device__ __forceinline__ void lp_for_row(const T* row, int n, bool vec, F8&& f8, F1&& f1) {
  int done = 0;
  if (vec) {
    done = n & ~7;
    for (int c = threadIdx.x * 8; c < done; c += LP_T * 8) {
      float v[8];
      lp_load8<T>(row + c, v);
      f8(v, c);
    }
  }
  for (int c = done + threadIdx.x; c < n; c += LP_T) f1(lp_load<T>(row, c), c);
}

struct LpSmem {
  unsigned hist[LP_BINS];
  float cv[LP_CAP];
  int ci[LP_CAP];
  unsigned tkey[LP_T];
  float sv[32];
  int si[32];
  float red[16];
  unsigned wsum[4];
  int wtie[4];
  unsigned floor_key;
  int ncand;
  int nsurv;
  int digit;
  unsigned above;
};

// First digit from the top whose inclusive count reaches target (1 <= target <= total): sm.digit and the count
// strictly above it. Thread t owns the 8 bins LP_BINS - 1 - 8t .. LP_BINS - 8 - 8t.
__device__ __forceinline__ void lp_find_digit(LpSmem& sm, unsigned target) {
  const int t = threadIdx.x, lane = t & 63, wid = t >> 6;
  unsigned c[8], loc = 0;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    c[i] = sm.hist[LP_BINS - 1 - (8 * t + i)];
    loc += c[i];
  }
  unsigned inc = loc;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const unsigned u = __shfl_up(inc, o, 64);
    if (lane >= o) inc += u;
  }
  if (lane == 63) sm.wsum[wid] = inc;
  __syncthreads();
  unsigned off = 0;
  for (int w = 0; w < wid; ++w) off += sm.wsum[w];
  const unsigned excl = off + inc - loc;
  if (excl < target && excl + loc >= target) {
    unsigned run = excl;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      if (run < target && run + c[i] >= target) {
        sm.digit = LP_BINS - 1 - (8 * t + i);
        sm.above = run;
      }
      run += c[i];
    }
  }
  __syncthreads();
}

template <typename T>
__global__ __launch_bounds__(LP_T) void token_logprobs_kernel(const T* __restrict__ logits, int64_t ld, int width,
                                                              int vl, int lo, int V,
                                                              const int64_t* __restrict__ tokens, int N, int vec,
                                                              float* __restrict__ lp, int64_t ld_lp,
                                                              float* __restrict__ top_lp, int64_t ld_top,
                                                              int* __restrict__ top_ids, int64_t ld_ids,
                                                              float* __restrict__ pack, int64_t ldp) {
  // radix levels: bits [31, 21], [20, 10], [9, 0]. bf16 values differ in key bits >= 16 only: two levels order them
  constexpr int NLVL = sizeof(T) == 2 ? 2 : 3;
  constexpr int LOW = sizeof(T) == 2 ? 10 : 0;
  __shared__ LpSmem sm;
  const int b = blockIdx.x, t = threadIdx.x, lane = t & 63, wid = t >> 6;
  const int c0 = blockIdx.y * vl;  // this shard's first column in the row
  const int glo = lo + c0;         // and its global token id
  int n = min(vl, width - c0);
  n = max(min(n, V - glo), 0);     // columns [c0, c0 + n) hold vocabulary entries
  const T* row = logits + (int64_t)b * ld + c0;
  const int NE = min(N, n);

  // pass 1: max
  float tmax = -INFINITY;
  lp_for_row<T>(row, n, vec != 0,
      [&](const float (&v)[8], int) {
        const float a = fmaxf(fmaxf(v[0], v[1]), fmaxf(v[2], v[3])), c = fmaxf(fmaxf(v[4], v[5]), fmaxf(v[6], v[7]));
        tmax = fmaxf(tmax, fmaxf(a, c));
      },
      [&](float x, int) { tmax = fmaxf(tmax, x); });
  sm.tkey[t] = tmax > -INFINITY ? lp_key(tmax) : 0u;  // 0 = below every real key (a thread without elements)
  if (t == 0) {
    sm.floor_key = 0u;
    sm.ncand = 0;
    sm.nsurv = 0;
  }
  const float mx = block_max(tmax, sm.red);  // its barriers publish tkey
  if (NE > 0) {
    const unsigned k = sm.tkey[t];
    int rank = 0;
    for (int j = 0; j < LP_T; ++j) {
      const unsigned k2 = sm.tkey[j];
      rank += (k2 > k || (k2 == k && j < t)) ? 1 : 0;
    }
    if (rank == NE - 1) sm.floor_key = k;
  }
  __syncthreads();
  const unsigned floor_key = sm.floor_key;

  // pass 2: sum exp(x - max), gather the elements at or above the floor
  float s = 0.f;
  auto gather = [&](float x, int j) {
    if (NE > 0 && lp_key(x) >= floor_key) {
      const int slot = atomicAdd(&sm.ncand, 1);
      if (slot < LP_CAP) {
        sm.cv[slot] = x;
        sm.ci[slot] = j;
      }
    }
  };
  lp_for_row<T>(row, n, vec != 0,
      [&](const float (&v)[8], int j0) {
        float e[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) {
          e[i] = __expf(v[i] - mx);
          gather(v[i], j0 + i);
        }
        s += ((e[0] + e[1]) + (e[2] + e[3])) + ((e[4] + e[5]) + (e[6] + e[7]));
      },
      [&](float x, int j) {
        s += __expf(x - mx);
        gather(x, j);
      });
  s = warp_sum(s);
  __syncthreads();
  if (lane == 0) sm.red[wid] = s;
  __syncthreads();
  const float S = (sm.red[0] + sm.red[1]) + (sm.red[2] + sm.red[3]);
  const float lse = mx + logf(S);

  if (NE > 0) {
    const int nc = sm.ncand;
    const bool inl = nc <= LP_CAP;  // the selection runs on the gathered elements
    auto for_sel = [&](auto&& f) {  // f(x, j) over every element at or above the floor
      if (inl) {
        for (int c = t; c < nc; c += LP_T) f(sm.cv[c], sm.ci[c]);
      } else {
        lp_for_row<T>(row, n, vec != 0,
            [&](const float (&v)[8], int j0) {
#pragma unroll
              for (int i = 0; i < 8; ++i)
                if (lp_key(v[i]) >= floor_key) f(v[i], j0 + i);
            },
            [&](float x, int j) {
              if (lp_key(x) >= floor_key) f(x, j);
            });
      }
    };
    unsigned prefix = 0u, target = (unsigned)NE;
#pragma unroll
    for (int lvl = 0; lvl < NLVL; ++lvl) {
      const int shift = lvl == 0 ? 21 : (lvl == 1 ? 10 : 0), bits = lvl == 2 ? 10 : 11;
      for (int i = t; i < LP_BINS; i += LP_T) sm.hist[i] = 0u;
      if (t == 0) {
        sm.digit = 0;
        sm.above = 0u;
      }
      __syncthreads();
      for_sel([&](float x, int) {
        const unsigned k = lp_key(x);
        if (lvl == 0 || (k >> ((shift + bits) & 31)) == prefix)
          atomicAdd(&sm.hist[(k >> shift) & ((1u << bits) - 1u)], 1u);
      });
      __syncthreads();
      lp_find_digit(sm, target);
      const unsigned d = (unsigned)sm.digit, a = sm.above;
      __syncthreads();  // both are read before thread 0 resets them
      target -= a;
      prefix = (prefix << bits) | d;
    }
    // prefix = (key >> LOW) of the NE-th largest element; `target` of the elements equal to it are kept
    const int need = (int)target;
    auto keep = [&](float x, int j) {
      const int slot = atomicAdd(&sm.nsurv, 1);
      if (slot < 32) {
        sm.sv[slot] = x;
        sm.si[slot] = j;
      }
    };
    if (inl) {
      for (int c = t; c < nc; c += LP_T) {
        const float x = sm.cv[c];
        const int j = sm.ci[c];
        const unsigned kq = lp_key(x) >> LOW;
        if (kq > prefix) {
          keep(x, j);
        } else if (kq == prefix) {  // ties: the `need` lowest ids
          int rank = 0;
          for (int c2 = 0; c2 < nc && rank < need; ++c2)
            rank += ((lp_key(sm.cv[c2]) >> LOW) == prefix && sm.ci[c2] < j) ? 1 : 0;
          if (rank < need) keep(x, j);
        }
      }
    } else {
      for_sel([&](float x, int j) {
        if ((lp_key(x) >> LOW) > prefix) keep(x, j);
      });
      // ties in ascending id: 256 consecutive columns per step, ballot ranks, until `need` are found
      int tie_base = 0;
      for (int base = 0; base < n && tie_base < need; base += LP_T) {
        const int j = base + t;
        const float x = j < n ? lp_load<T>(row, j) : 0.f;
        const bool tie = j < n && (lp_key(x) >> LOW) == prefix;
        const unsigned long long bal = __ballot(tie);
        if (lane == 0) sm.wtie[wid] = __popcll(bal);
        __syncthreads();
        int off = tie_base, tot = 0;
        for (int w = 0; w < LP_T / 64; ++w) {
          off += w < wid ? sm.wtie[w] : 0;
          tot += sm.wtie[w];
        }
        const int rank = off + __popcll(bal & ((1ull << lane) - 1ull));
        if (tie && rank < need) keep(x, j);
        __syncthreads();
        tie_base += tot;
      }
    }
    __syncthreads();
  }

  // rank the NE survivors and write
  float* ov;
  int* oi;
  if (pack) {
    float* p = pack + (int64_t)b * ldp + (int64_t)blockIdx.y * (3 + 2 * N);
    ov = p + 3;
    oi = reinterpret_cast<int*>(p + 3 + N);
    if (t == 0) {
      const int64_t j = tokens[b] - glo;
      p[0] = mx;
      p[1] = S;
      p[2] = (j >= 0 && j < n) ? lp_load<T>(row, (int)j) : -INFINITY;
    }
  } else {
    ov = top_lp + (int64_t)b * ld_top;
    oi = top_ids + (int64_t)b * ld_ids;
    if (t == 0) {
      const int64_t j = tokens[b];
      lp[(int64_t)b * ld_lp] = (j >= 0 && j < n) ? lp_load<T>(row, (int)j) - lse : __uint_as_float(0x7fc00000u);
    }
  }
  if (t < NE) {
    const float x = sm.sv[t];
    const int j = sm.si[t];
    int rank = 0;
    for (int i = 0; i < NE; ++i) rank += (sm.sv[i] > x || (sm.sv[i] == x && sm.si[i] < j)) ? 1 : 0;
    ov[rank] = pack ? x : x - lse;
    oi[rank] = glo + j;
  } else if (t < N) {
    ov[t] = -INFINITY;
    oi[t] = -1;
  }
}

// Merge the gathered packs of `groups` shards (rank-major, 3 + 2N floats each) per row. One candidate per thread
// at tp * N <= 256; each ranks itself against all candidates in LDS (no early exit: the loop pipelines).
constexpr int LPC_T = 256;

__global__ __launch_bounds__(LPC_T) void logprobs_combine_kernel(const float* __restrict__ pack, int64_t ldp,
                                                              int groups, int N, float* __restrict__ lp, int64_t ld_lp,
                                                              float* __restrict__ top_lp, int64_t ld_top,
                                                              int* __restrict__ top_ids, int64_t ld_ids) {
  __shared__ float v[LP_MAXCAND];
  __shared__ int id[LP_MAXCAND];
  __shared__ int nvalid;
  const int b = blockIdx.x, t = threadIdx.x, P = 3 + 2 * N, n = groups * N;
  if (t == 0) nvalid = 0;
  __syncthreads();
  const float* row = pack + (int64_t)b * ldp;
  float M = -INFINITY, xt = -INFINITY;
  for (int g = 0; g < groups; ++g) {
    M = fmaxf(M, row[g * P]);
    xt = fmaxf(xt, row[g * P + 2]);
  }
  float S = 0.f;
  for (int g = 0; g < groups; ++g) S += row[g * P + 1] * expf(row[g * P] - M);  // rank order
  const float lse = M + logf(S);
  if (t == 0) lp[(int64_t)b * ld_lp] = xt > -INFINITY ? xt - lse : __uint_as_float(0x7fc00000u);
  int myvalid = 0;
  for (int i = t; i < n; i += LPC_T) {
    const int g = i / N, k = i - g * N;
    v[i] = row[g * P + 3 + k];
    id[i] = reinterpret_cast<const int*>(row)[g * P + 3 + N + k];
    myvalid += id[i] >= 0 ? 1 : 0;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) myvalid += __shfl_xor(myvalid, o, 64);
  if ((t & 63) == 0 && myvalid) atomicAdd(&nvalid, myvalid);
  __syncthreads();
  myvalid = nvalid;
  float* ov = top_lp + (int64_t)b * ld_top;
  int* oi = top_ids + (int64_t)b * ld_ids;
  for (int i = t; i < n; i += LPC_T) {
    const float x = v[i];
    const int xi = id[i];
    if (xi < 0) continue;
    int rank = 0;
#pragma unroll 8
    for (int j = 0; j < n; ++j) rank += (id[j] >= 0 && (v[j] > x || (v[j] == x && id[j] < xi))) ? 1 : 0;
    if (rank < N) {
      ov[rank] = x - lse;
      oi[rank] = xi;
    }
  }
  if (t < N && t >= myvalid) {
    ov[t] = -INFINITY;
    oi[t] = -1;
  }
}

void launch_token_logprobs(const void* logits, int64_t ld, bool fp32, int B, int width, int lo, int V,
                           const void* tokens, int N, int shards, void* lp, int64_t ld_lp, void* top_lp,
                           int64_t ld_top, void* top_ids, int64_t ld_ids, void* pack, int64_t ldp, hipStream_t st) {
  if (B == 0) return;
  if (N < 0 || N > LP_MAXN) throw std::runtime_error("token_logprobs: N must be in 0..20");
  if (shards < 1 || width < 1) throw std::runtime_error("token_logprobs: need shards >= 1 and a non-empty row");
  if (pack) {
    if ((int64_t)shards * (3 + 2 * N) > ldp) throw std::runtime_error("token_logprobs: pack row too narrow");
  } else if (shards != 1 || !lp || (N > 0 && (!top_lp || !top_ids))) {
    throw std::runtime_error("token_logprobs: full rows take one shard and all three outputs");
  }
  const int vl = (width + shards - 1) / shards;
  const int vec = (uintptr_t)logits % 16 == 0 && ld % 8 == 0 && (shards == 1 || vl % 8 == 0);
#define LPK(T_)                                                                                                     \
  token_logprobs_kernel<T_><<<dim3(B, shards), LP_T, 0, st>>>((const T_*)logits, ld, width, vl, lo, V,               \
                                                              (const int64_t*)tokens, N, vec, (float*)lp, ld_lp,      \
                                                              (float*)top_lp, ld_top, (int*)top_ids, ld_ids,          \
                                                              (float*)pack, ldp)
  if (fp32) LPK(float);
  else LPK(bf16_t);
#undef LPK
  HIP_CHECK_LAUNCH();
}

void launch_logprobs_combine(const void* pack, int64_t ldp, int B, int groups, int N, void* lp, int64_t ld_lp,
                             void* top_lp, int64_t ld_top, void* top_ids, int64_t ld_ids, hipStream_t st) {
  if (B == 0) return;
  if (N < 0 || N > LP_MAXN) throw std::runtime_error("logprobs_combine: N must be in 0..20");
  if (groups < 1 || groups * N > LP_MAXCAND || (int64_t)groups * (3 + 2 * N) > ldp)
    throw std::runtime_error("logprobs_combine: bad group count for the pack row");
  logprobs_combine_kernel<<<B, LPC_T, 0, st>>>((const float*)pack, ldp, groups, N, (float*)lp, ld_lp, (float*)top_lp,
                                            ld_top, (int*)top_ids, ld_ids);
  HIP_CHECK_LAUNCH();
}
