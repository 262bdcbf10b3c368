// Panel packer for the decode GEMMs' packed-B variants (gemm_dec.hip / gemm_mid.hip PK, hint bit 2048 of launch_gemm):
//   P[ceil(N/16)][ceil(K/64)][16][64] bf16,  P[n / 16][k / 64][n % 16][k % 64] = W[n][k],  zeros past N and K
// from a row-major [N, K] bf16 weight of any row stride. Run once per weight at engine start (the weights are constant
// in serving); ops/reference.py pack_panels is its twin and oracle.
#include "common.h"

// one thread per 16-byte chunk (8 k) of the packed image; VEC: 16-byte source loads (row stride and base 16-B aligned)
template <bool VEC>
__global__ __launch_bounds__(256) void pack_panels_kernel(const bf16_t* __restrict__ W, int64_t ld,
                                                          bf16_t* __restrict__ P, int N, int K, int KP, int64_t chunks) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < chunks; i += (int64_t)gridDim.x * blockDim.x) {
    const int c = (int)(i & 7), r = (int)((i >> 3) & 15);
    const int64_t panel = i >> 7;
    const int kp = (int)(panel % KP);
    const int64_t n = (panel / KP) * 16 + r;
    const int k = kp * 64 + c * 8;
    u16x8 v = {0, 0, 0, 0, 0, 0, 0, 0};
    if (n < N && k < K) {
      const bf16_t* src = W + n * ld + k;
      if (VEC && k + 8 <= K) {
        v = *reinterpret_cast<const u16x8*>(src);
      } else {
#pragma unroll
        for (int j = 0; j < 8; ++j)
          if (k + j < K) v[j] = src[j];
      }
    }
    *reinterpret_cast<u16x8*>(P + i * 8) = v;
  }
}

void launch_pack_panels(const void* w, int64_t ld, void* p, int64_t N, int64_t K, hipStream_t st) {
  if (N <= 0 || K <= 0) return;
  if (N > INT32_MAX || K > INT32_MAX || ld < K) throw std::runtime_error("pack_panels: bad shape or row stride");
  const int64_t KP = (K + 63) / 64;
  const int64_t chunks = ((N + 15) / 16) * KP * 128;
  const int blocks = (int)std::min<int64_t>((chunks + 255) / 256, 256 * 16);
  const bool vec = ld % 8 == 0 && reinterpret_cast<uintptr_t>(w) % 16 == 0;
  if (vec)
    pack_panels_kernel<true><<<blocks, 256, 0, st>>>((const bf16_t*)w, ld, (bf16_t*)p, (int)N, (int)K, (int)KP, chunks);
  else
    pack_panels_kernel<false><<<blocks, 256, 0, st>>>((const bf16_t*)w, ld, (bf16_t*)p, (int)N, (int)K, (int)KP, chunks);
  HIP_CHECK_LAUNCH();
}
