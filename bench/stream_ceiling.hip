// Streaming-read ceilings on MI355X for the decode GEMM design (no compute, one pass over a buffer
// far larger than the Infinity Cache): what per-CU / chip read rate each load path reaches.
//   dma<NS, L>   : buffer_load ... lds ring (NS slots, L KiB per wave per slot), counted vmcnt + s_barrier
//                  per slot - the gemm_tiled / gemm_mid staging pattern without the MFMA work
//   vgpr<U>      : global 16-B loads straight into registers, U per lane in flight, folded into a checksum
// build: hipcc -O3 --offload-arch=gfx950 -std=c++17 bench/stream_ceiling.hip -o bench/stream_ceiling
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#define CK(x)                                                                       \
  do {                                                                              \
    hipError_t e = (x);                                                             \
    if (e != hipSuccess) {                                                          \
      fprintf(stderr, "%s:%d %s\n", __FILE__, __LINE__, hipGetErrorString(e));      \
      exit(1);                                                                      \
    }                                                                               \
  } while (0)

typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
#define LDS_AS __attribute__((address_space(3)))

template <int NS, int L, int NW, int AUX>
__global__ __launch_bounds__(64 * NW) void dma_kernel(const char* __restrict__ src, size_t chunk, unsigned* out) {
  __shared__ __attribute__((aligned(16))) char ring[NS * NW * L * 1024];
  const int lane = threadIdx.x & 63;
  const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const char* base = src + (size_t)blockIdx.x * chunk;
  const auto rs = __builtin_amdgcn_make_buffer_rsrc(const_cast<char*>(base), (short)0, (int)chunk, 0x00020000);
  constexpr int SLOT = NW * L * 1024;
  const int steps = (int)(chunk / SLOT);
  const uint32_t voff = (uint32_t)(w * L * 1024 + lane * 16);
#define ISSUE(T_)                                                                                            \
  do {                                                                                                       \
    char* d_ = ring + ((T_) % NS) * SLOT + w * L * 1024;                                                     \
    const int so_ = (T_) * SLOT;                                                                             \
    _Pragma("unroll") for (int i_ = 0; i_ < L; ++i_)                                                         \
      __builtin_amdgcn_raw_ptr_buffer_load_lds(rs, (LDS_AS void*)(d_ + i_ * 1024), 16, (uint32_t)(voff + i_ * 1024), \
                                               (uint32_t)so_, 0, AUX);                                       \
  } while (0)
  for (int j = 0; j < NS - 1 && j < steps; ++j) ISSUE(j);
  unsigned acc = 0;
  for (int t = 0; t < steps; ++t) {
    const int younger = min(steps - 1 - t, NS - 2);
    if (NS >= 5 && younger >= 3) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(3 * L) : "memory");
    else if (NS >= 4 && younger == 2) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(2 * L) : "memory");
    else if (NS >= 3 && younger == 1) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(L) : "memory");
    else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
    if (t + NS - 1 < steps) ISSUE(t + NS - 1);
    acc += *reinterpret_cast<const unsigned*>(ring + (t % NS) * SLOT + threadIdx.x * 4);
  }
#undef ISSUE
  if (acc == 0x12345678u) out[blockIdx.x] = acc;
}


// the GEMM weight-tile pattern: workgroup w streams rows [w*BN, (w+1)*BN) x K of a [rows][K] bf16 matrix,
// one 128-B k-slice of every row per ring slot (8 rows x 128 B per wave-instruction), as gemm_mid does.
// PACKED: the same bytes laid out [rows/16][K/64][16][64] (a slot = BN/16 contiguous 2-KiB panels);
// WITHA: each slot also stages a 64-row x 128-B activation tile from a 512 KiB (L2-resident) matrix
template <int NS, int BN, int NW, bool PACKED, bool WITHA>
__global__ __launch_bounds__(64 * NW) void tile_kernel(const char* __restrict__ src, const char* __restrict__ act,
                                                       int K, int ksplit, unsigned* out) {
  constexpr int BBYTES = BN * 128, ABYTES = WITHA ? 64 * 128 : 0, SLOT = BBYTES + ABYTES;
  constexpr int L = BN / (8 * NW), LA = WITHA ? 64 / (8 * NW) : 0;
  __shared__ __attribute__((aligned(16))) char ring[NS * SLOT];
  const int lane = threadIdx.x & 63;
  const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int rt = blockIdx.x / ksplit, kz = blockIdx.x % ksplit;
  const size_t rowb = (size_t)K * 2;
  const int steps = K / 64 / ksplit;
  const int k64 = K / 64;
  const char* base = PACKED ? src + (size_t)rt * BN * rowb + (size_t)kz * steps * 2048
                            : src + (size_t)rt * BN * rowb + (size_t)kz * steps * 128;
  const auto rs = __builtin_amdgcn_make_buffer_rsrc(const_cast<char*>(base), (short)0, (int)(BN * rowb), 0x00020000);
  const auto ra = __builtin_amdgcn_make_buffer_rsrc(const_cast<char*>(act + (size_t)kz * steps * 128), (short)0,
                                                    (int)(64 * rowb), 0x00020000);
  uint32_t voff[L], aoff[LA > 0 ? LA : 1];
#pragma unroll
  for (int i = 0; i < L; ++i) {
    const int r = (i * NW + w) * 8 + (lane >> 3);
    voff[i] = PACKED ? (uint32_t)((r / 16) * k64 * 2048 + (r % 16) * 128 + (lane & 7) * 16)
                     : (uint32_t)(r * rowb + (lane & 7) * 16);
  }
#pragma unroll
  for (int i = 0; i < LA; ++i) aoff[i] = (uint32_t)(((i * NW + w) * 8 + (lane >> 3)) * rowb + (lane & 7) * 16);
#define TISSUE(T_)                                                                                           \
  do {                                                                                                       \
    char* d_ = ring + ((T_) % NS) * SLOT;                                                                    \
    _Pragma("unroll") for (int i_ = 0; i_ < LA; ++i_)                                                        \
      __builtin_amdgcn_raw_ptr_buffer_load_lds(ra, (LDS_AS void*)(d_ + BBYTES + (i_ * NW + w) * 1024), 16,   \
                                               (uint32_t)aoff[i_], (uint32_t)((T_) * 128), 0, 0);           \
    _Pragma("unroll") for (int i_ = 0; i_ < L; ++i_)                                                         \
      __builtin_amdgcn_raw_ptr_buffer_load_lds(rs, (LDS_AS void*)(d_ + (i_ * NW + w) * 1024), 16, (uint32_t)voff[i_], \
                                               (uint32_t)((T_) * (PACKED ? 2048 : 128)), 0, 2);              \
  } while (0)
  constexpr int LT = L + LA;
  for (int j = 0; j < NS - 1 && j < steps; ++j) TISSUE(j);
  unsigned acc = 0;
  for (int t = 0; t < steps; ++t) {
    const int younger = min(steps - 1 - t, NS - 2);
    if (NS >= 5 && younger >= 3) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(3 * LT) : "memory");
    else if (NS >= 4 && younger == 2) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(2 * LT) : "memory");
    else if (NS >= 3 && younger == 1) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(LT) : "memory");
    else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
    if (t + NS - 1 < steps) TISSUE(t + NS - 1);
    acc += *reinterpret_cast<const unsigned*>(ring + (t % NS) * SLOT + threadIdx.x * 4);
  }
#undef TISSUE
  if (acc == 0x12345678u) out[blockIdx.x] = acc;
}

// row-major weight tile with RB bytes of every row per ring slot (RB = 128: gemm_mid's k-step; RB = 256: a 128-element
// bf16 k-step, each wave-instruction 64 * 16 / RB rows x RB contiguous bytes), plus the 64-row activation tile
template <int NS, int BN, int NW, int RB>
__global__ __launch_bounds__(64 * NW) void tile_rb_kernel(const char* __restrict__ src, const char* __restrict__ act,
                                                          int K, int ksplit, unsigned* out) {
  constexpr int BBYTES = BN * RB, ABYTES = 64 * RB, SLOT = BBYTES + ABYTES;
  constexpr int RPI = 1024 / RB;  // rows per wave-instruction
  constexpr int L = BN / (RPI * NW), LA = 64 / (RPI * NW);
  static_assert(L >= 1 && LA >= 1, "tile rows must cover the waves");
  __shared__ __attribute__((aligned(16))) char ring[NS * SLOT];
  const int lane = threadIdx.x & 63;
  const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int rt = blockIdx.x / ksplit, kz = blockIdx.x % ksplit;
  const size_t rowb = (size_t)K * 2;
  const int steps = (int)(rowb / RB) / ksplit;
  const char* base = src + (size_t)rt * BN * rowb + (size_t)kz * steps * RB;
  const auto rs = __builtin_amdgcn_make_buffer_rsrc(const_cast<char*>(base), (short)0, (int)(BN * rowb), 0x00020000);
  const auto ra = __builtin_amdgcn_make_buffer_rsrc(const_cast<char*>(act + (size_t)kz * steps * RB), (short)0,
                                                    (int)(64 * rowb), 0x00020000);
  uint32_t voff[L], aoff[LA];
#pragma unroll
  for (int i = 0; i < L; ++i)
    voff[i] = (uint32_t)(((i * NW + w) * RPI + lane / (RB / 16)) * rowb + (lane % (RB / 16)) * 16);
#pragma unroll
  for (int i = 0; i < LA; ++i)
    aoff[i] = (uint32_t)(((i * NW + w) * RPI + lane / (RB / 16)) * rowb + (lane % (RB / 16)) * 16);
#define RISSUE(T_)                                                                                           \
  do {                                                                                                       \
    char* d_ = ring + ((T_) % NS) * SLOT;                                                                    \
    _Pragma("unroll") for (int i_ = 0; i_ < LA; ++i_)                                                        \
      __builtin_amdgcn_raw_ptr_buffer_load_lds(ra, (LDS_AS void*)(d_ + BBYTES + (i_ * NW + w) * 1024), 16,   \
                                               (uint32_t)aoff[i_], (uint32_t)((T_) * RB), 0, 0);            \
    _Pragma("unroll") for (int i_ = 0; i_ < L; ++i_)                                                         \
      __builtin_amdgcn_raw_ptr_buffer_load_lds(rs, (LDS_AS void*)(d_ + (i_ * NW + w) * 1024), 16, (uint32_t)voff[i_], \
                                               (uint32_t)((T_) * RB), 0, 2);                                 \
  } while (0)
  constexpr int LT = L + LA;
  for (int j = 0; j < NS - 1 && j < steps; ++j) RISSUE(j);
  unsigned acc = 0;
  for (int t = 0; t < steps; ++t) {
    const int younger = min(steps - 1 - t, NS - 2);
    if (NS >= 4 && younger >= 2) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(2 * LT) : "memory");
    else if (NS >= 3 && younger >= 1) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(LT) : "memory");
    else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
    if (t + NS - 1 < steps) RISSUE(t + NS - 1);
    acc += *reinterpret_cast<const unsigned*>(ring + (t % NS) * SLOT + threadIdx.x * 4);
  }
#undef RISSUE
  if (acc == 0x12345678u) out[blockIdx.x] = acc;
}

template <int U, int NW>
__global__ __launch_bounds__(64 * NW) void vgpr_kernel(const char* __restrict__ src, size_t chunk, unsigned* out) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const char* base = src + (size_t)blockIdx.x * chunk;
  const size_t per_iter = (size_t)NW * U * 1024;
  unsigned acc = 0;
  for (size_t o = 0; o + per_iter <= chunk; o += per_iter) {
    u32x4 v[U];
#pragma unroll
    for (int u = 0; u < U; ++u)
      v[u] = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(base + o + (size_t)(u * NW + w) * 1024 + lane * 16));
#pragma unroll
    for (int u = 0; u < U; ++u) acc ^= v[u][0] + v[u][1] + v[u][2] + v[u][3];
  }
  if (acc == 0x12345678u) out[blockIdx.x] = acc;
}

// Today's two decode-GEMM load patterns on the real decode shapes (row-major vs panel-packed weights).
// dec_pattern: gemm_dec - wave w of 4 takes k-steps t0 + w, t0 + w + 4, ... of the workgroup's K slice and stages
//   the whole (64 + BN)-row x 128-B k-step into its private ring (depth as dec_depth picks), waiting on its own
//   counted vmcnt; no workgroup barrier in the loop.
// mid_pattern: gemm_mid - 4 waves share one ring; each stages every 4th 8-row piece of the 64 + BN rows of a k-step.
// Rows past N fall outside the descriptor range and read as zero, as in the kernels.
template <int BN>
constexpr int dec_nsw() {
  int ns = 4;
  while (ns > 2 && 4 * ns * (64 + BN) * 128 > 160 * 1024) --ns;
  return ns;
}
template <int N_>
__device__ __forceinline__ void probe_wait(int younger) {
  if (younger >= 3) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(3 * N_ <= 63 ? 3 * N_ : 0) : "memory");
  else if (younger == 2) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(2 * N_ <= 63 ? 2 * N_ : 0) : "memory");
  else if (younger == 1) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N_) : "memory");
  else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
}

template <int BN, bool PACKED>
__global__ __launch_bounds__(256) void dec_pattern_kernel(const char* __restrict__ src, const char* __restrict__ act,
                                                          int N, int K, unsigned* out) {
  constexpr int NW = 4, AR = 64, AL = AR / 8, BL = BN / 8, LOADS = AL + BL, SLOT = (AR + BN) * 128;
  constexpr int NSW = dec_nsw<BN>();
  static_assert((NSW - 1) * LOADS <= 63, "vmcnt immediate");
  __shared__ __attribute__((aligned(16))) char smem[NW * NSW * SLOT];
  const int lane = threadIdx.x & 63;
  const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int n0 = blockIdx.x * BN, zk = blockIdx.y;
  const int nk_all = K / 64;
  const int per = (nk_all + gridDim.y - 1) / gridDim.y;
  const int t0 = zk * per, t1 = min(nk_all, t0 + per);
  const int mine = t1 - t0 - w;
  const int nloc = mine > 0 ? (mine + NW - 1) / NW : 0;
  const uint32_t rowb = (uint32_t)K * 2u;
  const uint32_t bbytes = PACKED ? (uint32_t)((N + 15) / 16 - n0 / 16) * (uint32_t)nk_all * 2048u
                                 : (uint32_t)(N - n0) * rowb;
  const char* bbase = PACKED ? src + (size_t)(n0 / 16) * nk_all * 2048 : src + (size_t)n0 * rowb;
  const auto ra = __builtin_amdgcn_make_buffer_rsrc(const_cast<char*>(act), (short)0, (int)(64u * rowb), 0x00020000);
  const auto rb = __builtin_amdgcn_make_buffer_rsrc(const_cast<char*>(bbase), (short)0, (int)bbytes, 0x00020000);
  uint32_t va[AL], vb[BL];
#pragma unroll
  for (int i = 0; i < AL; ++i) {
    const int row = i * 8 + (lane >> 3);
    va[i] = (uint32_t)(row * rowb + (((lane & 7) ^ (row & 7)) << 4));
  }
#pragma unroll
  for (int i = 0; i < BL; ++i) {
    const int row = i * 8 + (lane >> 3);
    const uint32_t ch = (uint32_t)(((lane & 7) ^ (row & 7)) << 4);
    vb[i] = PACKED ? (uint32_t)((row / 16) * nk_all * 2048 + (row % 16) * 128) + ch : (uint32_t)(row * rowb) + ch;
  }
  char* ring = smem + w * (NSW * SLOT);
#define PISSUE(J_)                                                                                               \
  do {                                                                                                           \
    const int t_ = t0 + w + NW * (J_);                                                                           \
    char* sl_ = ring + ((J_) % NSW) * SLOT;                                                                      \
    _Pragma("unroll") for (int i_ = 0; i_ < AL; ++i_)                                                            \
      __builtin_amdgcn_raw_ptr_buffer_load_lds(ra, (LDS_AS void*)(sl_ + i_ * 1024), 16, (uint32_t)va[i_],        \
                                               (uint32_t)t_ * 128u, 0, 0);                                       \
    _Pragma("unroll") for (int i_ = 0; i_ < BL; ++i_)                                                            \
      __builtin_amdgcn_raw_ptr_buffer_load_lds(rb, (LDS_AS void*)(sl_ + AR * 128 + i_ * 1024), 16,               \
                                               (uint32_t)vb[i_], (uint32_t)t_ * (PACKED ? 2048u : 128u), 0, 2);  \
  } while (0)
  const int pre = nloc < NSW ? nloc : NSW;
  for (int j = 0; j < pre; ++j) PISSUE(j);
  unsigned acc = 0;
  for (int j = 0; j < nloc; ++j) {
    probe_wait<LOADS>(min(NSW - 1, nloc - 1 - j));
    acc += *reinterpret_cast<const unsigned*>(ring + (j % NSW) * SLOT + AR * 128 + lane * 4);
    if (j + NSW < nloc) {
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      PISSUE(j + NSW);
    }
  }
#undef PISSUE
  if (acc == 0x12345678u) out[blockIdx.x] = acc;
}

template <int NS, int BN, bool PACKED>
__global__ __launch_bounds__(256) void mid_pattern_kernel(const char* __restrict__ src, const char* __restrict__ act,
                                                          int N, int K, unsigned* out) {
  constexpr int NW = 4, BM = 64, AL = BM / (8 * NW), BL = BN / (8 * NW), LOADS = AL + BL;
  constexpr int A_BYTES = BM * 128, STAGE = (BM + BN) * 128;
  static_assert(BN % (8 * NW) == 0 && (NS - 2) * LOADS <= 63 && NS * STAGE <= 160 * 1024, "tile");
  __shared__ __attribute__((aligned(16))) char smem[NS * STAGE];
  const int lane = threadIdx.x & 63;
  const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int n0 = blockIdx.x * BN, zk = blockIdx.y;
  const int nk_all = K / 64;
  const int per = (nk_all + gridDim.y - 1) / gridDim.y;
  const int t0 = zk * per, t1 = min(nk_all, t0 + per);
  const uint32_t rowb = (uint32_t)K * 2u;
  const uint32_t bbytes = PACKED ? (uint32_t)((N + 15) / 16 - n0 / 16) * (uint32_t)nk_all * 2048u
                                 : (uint32_t)(N - n0) * rowb;
  const char* bbase = PACKED ? src + (size_t)(n0 / 16) * nk_all * 2048 : src + (size_t)n0 * rowb;
  const auto ra = __builtin_amdgcn_make_buffer_rsrc(const_cast<char*>(act), (short)0, (int)(64u * rowb), 0x00020000);
  const auto rb = __builtin_amdgcn_make_buffer_rsrc(const_cast<char*>(bbase), (short)0, (int)bbytes, 0x00020000);
  uint32_t va[AL], vb[BL];
#pragma unroll
  for (int i = 0; i < AL; ++i) {
    const int row = (i * NW + w) * 8 + (lane >> 3);
    va[i] = (uint32_t)(row * rowb + (((lane & 7) ^ (row & 7)) << 4));
  }
#pragma unroll
  for (int i = 0; i < BL; ++i) {
    const int row = (i * NW + w) * 8 + (lane >> 3);
    const uint32_t ch = (uint32_t)(((lane & 7) ^ (row & 7)) << 4);
    vb[i] = PACKED ? (uint32_t)((row / 16) * nk_all * 2048 + (row % 16) * 128) + ch : (uint32_t)(row * rowb) + ch;
  }
#define MISSUE(T_, SA_)                                                                                          \
  do {                                                                                                           \
    char* sA_ = (SA_);                                                                                           \
    _Pragma("unroll") for (int i_ = 0; i_ < AL; ++i_)                                                            \
      __builtin_amdgcn_raw_ptr_buffer_load_lds(ra, (LDS_AS void*)(sA_ + (i_ * NW + w) * 1024), 16,               \
                                               (uint32_t)va[i_], (uint32_t)(T_) * 128u, 0, 0);                   \
    _Pragma("unroll") for (int i_ = 0; i_ < BL; ++i_)                                                            \
      __builtin_amdgcn_raw_ptr_buffer_load_lds(rb, (LDS_AS void*)(sA_ + A_BYTES + (i_ * NW + w) * 1024), 16,     \
                                               (uint32_t)vb[i_], (uint32_t)(T_) * (PACKED ? 2048u : 128u), 0, 2); \
  } while (0)
  for (int j = 0; j < NS - 1; ++j)
    if (t0 + j < t1) MISSUE(t0 + j, smem + j * STAGE);
  unsigned acc = 0;
  int cur = 0;
  for (int t = t0; t < t1; ++t) {
    probe_wait<LOADS>(min(t1 - 1 - t, NS - 2));
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
    const int nxt = cur == 0 ? NS - 1 : cur - 1;
    if (t + NS - 1 < t1) MISSUE(t + NS - 1, smem + nxt * STAGE);
    acc += *reinterpret_cast<const unsigned*>(smem + cur * STAGE + A_BYTES + threadIdx.x * 4);
    cur = cur == NS - 1 ? 0 : cur + 1;
  }
#undef MISSUE
  if (acc == 0x12345678u) out[blockIdx.x] = acc;
}

template <typename F>
static double time_us(F f, int reps) {
  hipEvent_t a, b;
  CK(hipEventCreate(&a));
  CK(hipEventCreate(&b));
  f(0);
  CK(hipDeviceSynchronize());
  CK(hipEventRecord(a));
  for (int i = 0; i < reps; ++i) f(i + 1);
  CK(hipEventRecord(b));
  CK(hipEventSynchronize(b));
  float ms;
  CK(hipEventElapsedTime(&ms, a, b));
  return ms * 1e3 / reps;
}

// Llama-2-7B's four decode GEMMs (M = 64) through the gemm_dec and gemm_mid load patterns, row-major vs packed.
// Each launch reads another copy of the weight: `rot` copies spread over the three buffers, > 1.5 GB in all, so no
// copy is still in the 256 MiB Infinity Cache when its turn comes again.
static void decode_table(std::vector<char*>& bufs, size_t total, const char* actbuf, unsigned* out) {
  struct Shape { const char* name; int N, K; };
  const Shape shapes[4] = {{"qkv", 12288, 4096}, {"o", 4096, 4096}, {"gate/up", 22016, 4096}, {"down", 4096, 11008}};
  printf("%-8s %-18s %5s %9s %9s %7s %7s %6s\n", "shape", "pattern", "grid", "rows us", "packed us", "TB/s", "TB/s",
         "gain");
  for (const Shape& sh : shapes) {
    const size_t bytes = (size_t)sh.N * sh.K * 2;
    const size_t stride = (bytes + 4095) & ~(size_t)4095;
    const int per_buf = (int)(total / stride);
    const int rot = 3 * (per_buf < 8 ? per_buf : 8);
    auto wptr = [&](int i) { return bufs[(i % rot) % 3] + (size_t)((i % rot) / 3) * stride; };
    auto row = [&](const char* pat, int grid, double ur, double up) {
      printf("%-8s %-18s %5d %9.2f %9.2f %7.2f %7.2f %+5.1f%%\n", sh.name, pat, grid, ur, up, bytes / ur / 1e6,
             bytes / up / 1e6, (ur / up - 1.0) * 100.0);
      fflush(stdout);
    };
    const int reps = 3 * rot;
#define DECP(BN_, S_)                                                                                            \
  do {                                                                                                           \
    dim3 g((sh.N + BN_ - 1) / BN_, S_);                                                                          \
    if (g.x * g.y < 128 || g.x * g.y > 1536) break;                                                              \
    double ur = time_us([&](int i) { dec_pattern_kernel<BN_, false><<<g, 256>>>(wptr(i), actbuf, sh.N, sh.K, out); }, reps); \
    double up = time_us([&](int i) { dec_pattern_kernel<BN_, true><<<g, 256>>>(wptr(i), actbuf, sh.N, sh.K, out); }, reps);  \
    char nm[64];                                                                                                 \
    snprintf(nm, sizeof nm, "dec 64x%d s%d ns%d", BN_, S_, dec_nsw<BN_>());                                      \
    row(nm, g.x * g.y, ur, up);                                                                                  \
  } while (0)
#define MIDP(NS_, BN_, S_)                                                                                       \
  do {                                                                                                           \
    dim3 g((sh.N + BN_ - 1) / BN_, S_);                                                                          \
    if (g.x * g.y < 128 || g.x * g.y > 1536) break;                                                              \
    double ur = time_us([&](int i) { mid_pattern_kernel<NS_, BN_, false><<<g, 256>>>(wptr(i), actbuf, sh.N, sh.K, out); }, reps); \
    double up = time_us([&](int i) { mid_pattern_kernel<NS_, BN_, true><<<g, 256>>>(wptr(i), actbuf, sh.N, sh.K, out); }, reps);  \
    char nm[64];                                                                                                 \
    snprintf(nm, sizeof nm, "mid 64x%d s%d ns%d", BN_, S_, NS_);                                                 \
    row(nm, g.x * g.y, ur, up);                                                                                  \
  } while (0)
    for (int s = 1; s <= 4; s *= 2) {
      if (s == 1) { DECP(16, 1); DECP(32, 1); DECP(48, 1); DECP(64, 1); MIDP(4, 96, 1); MIDP(5, 96, 1); MIDP(4, 64, 1); }
      if (s == 2) { DECP(16, 2); DECP(32, 2); DECP(48, 2); DECP(64, 2); MIDP(4, 96, 2); MIDP(5, 96, 2); MIDP(4, 64, 2); }
      if (s == 4) { DECP(16, 4); DECP(32, 4); DECP(48, 4); DECP(64, 4); MIDP(4, 96, 4); MIDP(5, 96, 4); MIDP(4, 64, 4); }
    }
#undef DECP
#undef MIDP
  }
}

int main(int argc, char** argv) {
  const size_t total = 768ull << 20;  // per pass; 3 rotating buffers: 2.3 GB, far beyond the 256 MiB MALL
  std::vector<char*> bufs(3);
  for (auto& p : bufs) {
    CK(hipMalloc(&p, total));
    CK(hipMemset(p, 1, total));
  }
  unsigned* out;
  CK(hipMalloc(&out, 1 << 20));
  auto report = [&](const char* name, int grid, double us) {
    printf("%-28s grid %5d  %8.1f us  %6.2f TB/s  %6.1f GB/s per WG\n", name, grid, us, total / us / 1e6,
           total / us / 1e3 / grid);
    fflush(stdout);
  };
#define DMA(NS_, L_, NW_, AUX_, G_)                                                                           \
  do {                                                                                                     \
    const int g = (G_);                                                                                    \
    const size_t chunk = total / g;                                                                        \
    double us = time_us([&](int i) { dma_kernel<NS_, L_, NW_, AUX_><<<g, 64 * NW_>>>(bufs[i % 3], chunk, out); }, 6); \
    char nm[64];                                                                                           \
    snprintf(nm, sizeof nm, "dma ns%d L%d nw%d aux%d", NS_, L_, NW_, AUX_);                                \
    report(nm, g, us);                                                                                     \
  } while (0)
#define VG(U_, NW_, G_)                                                                                       \
  do {                                                                                                     \
    const int g = (G_);                                                                                    \
    const size_t chunk = total / g;                                                                        \
    double us = time_us([&](int i) { vgpr_kernel<U_, NW_><<<g, 64 * NW_>>>(bufs[i % 3], chunk, out); }, 6);  \
    char nm[64];                                                                                           \
    snprintf(nm, sizeof nm, "vgpr u%d nw%d", U_, NW_);                                                     \
    report(nm, g, us);                                                                                     \
  } while (0)
#define TILE(NS_, BN_, NW_, KS_, P_, A_)                                                                      \
  do {                                                                                                     \
    const int K = 4096, rows = (int)(total / (K * 2));                                                     \
    const int g = rows / BN_ * KS_;                                                                        \
    double us = time_us([&](int i) {                                                                       \
      tile_kernel<NS_, BN_, NW_, P_, A_><<<g, 64 * NW_>>>(bufs[i % 3], actbuf, K, KS_, out); }, 6);        \
    char nm[64];                                                                                           \
    snprintf(nm, sizeof nm, "tile ns%d bn%d nw%d ks%d %s%s", NS_, BN_, NW_, KS_, P_ ? "packed" : "rows",   \
             A_ ? "+A" : "");                                                                              \
    report(nm, g, us);                                                                                     \
  } while (0)
  char* actbuf;
  CK(hipMalloc(&actbuf, 64 * 11008 * 2));
  CK(hipMemset(actbuf, 1, 64 * 11008 * 2));
  if (argc > 1 && std::string(argv[1]) == "decode") {  // only the decode-shape table
    decode_table(bufs, total, actbuf, out);
    return 0;
  }
  // the GEMM weight-tile pattern (96K rows of 8 KiB): row-major vs packed panels, without / with the A tile
  TILE(4, 128, 4, 1, false, true);
  TILE(4, 128, 4, 1, true, true);
  // one decode GEMM's worth (Llama-2-7B QKV: 12288 x 4096 bf16 = 100.7 MB) on GEMM-like grids
#define TILEQ(NS_, BN_, NW_, KS_, P_)                                                                         \
  do {                                                                                                     \
    const int K = 4096, rows = 12288;                                                                      \
    const int g = rows / BN_ * KS_;                                                                        \
    const size_t bytes = (size_t)rows * K * 2;                                                             \
    double us = time_us([&](int i) {                                                                       \
      tile_kernel<NS_, BN_, NW_, P_, true><<<g, 64 * NW_>>>(bufs[i % 3], actbuf, K, KS_, out); }, 20);     \
    printf("qkv-size tile ns%d bn%d ks%d %-6s grid %4d  %7.2f us  %5.2f TB/s\n", NS_, BN_, KS_,            \
           P_ ? "packed" : "rows", g, us, bytes / us / 1e6);                                               \
    fflush(stdout);                                                                                        \
  } while (0)
  TILEQ(4, 128, 4, 1, true);
  TILEQ(4, 128, 4, 2, true);
  TILEQ(4, 128, 4, 2, false);
  TILEQ(3, 128, 4, 2, true);
  TILEQ(2, 128, 4, 2, true);
  TILEQ(4, 128, 4, 4, true);
  TILEQ(3, 128, 4, 4, true);
  TILEQ(2, 128, 4, 4, true);
  TILEQ(2, 128, 4, 8, true);
  TILEQ(4, 64, 4, 1, true);
  TILEQ(3, 64, 4, 2, true);
  TILEQ(2, 64, 4, 2, true);
  TILEQ(2, 64, 4, 4, true);
  TILEQ(4, 256, 4, 4, true);
  TILEQ(4, 256, 4, 5, true);
  DMA(4, 4, 4, 2, 256);
  // row bytes per k-step: 128 (gemm_mid today) vs 256, one QKV-sized matrix, activation tile included
#define TILERB(NS_, BN_, NW_, KS_, RB_)                                                                       \
  do {                                                                                                     \
    const int K = 4096, rows = 12288;                                                                      \
    const int g = rows / BN_ * KS_;                                                                        \
    const size_t bytes = (size_t)rows * K * 2;                                                             \
    double us = time_us([&](int i) {                                                                       \
      tile_rb_kernel<NS_, BN_, NW_, RB_><<<g, 64 * NW_>>>(bufs[i % 3], actbuf, K, KS_, out); }, 20);       \
    printf("qkv-size rb%d tile ns%d bn%d nw%d ks%d grid %4d  %7.2f us  %5.2f TB/s\n", RB_, NS_, BN_, NW_, KS_, g, us, \
           bytes / us / 1e6);                                                                              \
    fflush(stdout);                                                                                        \
  } while (0)
  TILERB(4, 64, 4, 1, 128);
  TILERB(4, 64, 4, 1, 256);
  TILERB(3, 64, 4, 1, 256);
  TILERB(4, 128, 4, 2, 128);
  TILERB(3, 128, 4, 2, 256);
  TILERB(4, 192, 4, 4, 128);
  TILERB(2, 192, 4, 4, 256);
  TILERB(4, 96, 4, 2, 128);
  TILERB(3, 96, 4, 2, 256);
  decode_table(bufs, total, actbuf, out);
  return 0;
}
