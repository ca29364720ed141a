// The chunked Gram matrix of the bag tokens X[b] = [gx, gy, u_1 .. u_L] (T = L + 2 rows of S points),
// shared by the bag attentions of attn.hip (NIOFP2D_FNO_attn) and bagattn_mix.hip
// (NIOFP2D_Trans_attn).  The kernel is static: every translation unit launches its own copy.
#pragma once
#include "common.h"

namespace blindno {

constexpr int kGramPts = 32;    // points per LDS sub-tile of the Gram kernel
constexpr int kGramChunk = 512; // points per workgroup (partial sum) of the Gram kernel

__device__ __forceinline__ float token(const float* __restrict__ grid, const float* __restrict__ u,
                                       int b, int t, int p, int L, int S) {
  return t < 2 ? grid[(int64_t)p * 2 + t] : u[((int64_t)b * L + (t - 2)) * S + p];
}

// partial[b][c][T][T] = sum over the chunk c of X[t,p] X[s,p]; each thread owns one 4x4 block of
// the upper block triangle (blockIdx.y picks the round of 256 blocks) and mirrors it.
static __global__ __launch_bounds__(kBlock) void gram_kernel(const float* __restrict__ grid,
                                                      const float* __restrict__ u,
                                                      float* __restrict__ partial, int L, int S,
                                                      int nch) {
  extern __shared__ float xs[];          // [T][kGramPts + 1]
  const int T = L + 2, b = blockIdx.z, c = blockIdx.x;
  const int nb = (T + 3) / 4, nblk = nb * (nb + 1) / 2;
  const int blk = blockIdx.y * kBlock + threadIdx.x;
  int bi = 0, bj = 0;
  const bool own = blk < nblk;
  if (own) {                             // blk -> (bi <= bj) in row-major upper triangle
    int r = blk;
    while (r >= nb - bi) { r -= nb - bi; ++bi; }
    bj = bi + r;
  }
  float acc[4][4] = {};
  const int p0 = c * kGramChunk, p1 = min(S, p0 + kGramChunk);
  constexpr int LD = kGramPts + 1;
  for (int q0 = p0; q0 < p1; q0 += kGramPts) {
    __syncthreads();
    for (int e = threadIdx.x; e < T * kGramPts; e += blockDim.x) {
      const int t = e / kGramPts, q = e % kGramPts;
      xs[t * LD + q] = q0 + q < p1 ? token(grid, u, b, t, q0 + q, L, S) : 0.f;
    }
    __syncthreads();
    if (own) {
#pragma unroll 4
      for (int q = 0; q < kGramPts; ++q) {
        float a[4], v[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int ti = min(4 * bi + i, T - 1), tj = min(4 * bj + i, T - 1);
          a[i] = xs[ti * LD + q];
          v[i] = xs[tj * LD + q];
        }
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
          for (int j = 0; j < 4; ++j) acc[i][j] = fmaf(a[i], v[j], acc[i][j]);
      }
    }
  }
  if (!own) return;
  float* g = partial + ((int64_t)b * nch + c) * T * T;
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int t = 4 * bi + i, s = 4 * bj + j;
      if (t < T && s < T) {
        g[t * T + s] = acc[i][j];
        g[s * T + t] = acc[i][j];
      }
    }
}

}  // namespace blindno
