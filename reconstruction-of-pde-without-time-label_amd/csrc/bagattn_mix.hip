// Multiplicity-weighted bag token attention of NIOFP2D_Trans_attn (2d_FPE/NIOModules.py:241-278;
// NC copy 2d_Non_conservative_FPE/NIOModules.py:168-) on a deduplicated bag: the formulas and the
// argument layout are in include/blindno_bagattn_mix.h.
//
// Tokens of sample b: X[b] = [gx, gy, u_1 .. u_U] (V = U + 2 rows of S points), masses
// [1, 1, nu_1 .. nu_U].  The Gram matrix does not depend on the masses, so the forward starts with
// attn.hip's chunked gram_kernel (baggram.h); the masses enter the softmax's numerator and the
// three output rows r_k.  Unlike attn.hip's fusion (one weight for every token: column sums of A),
// the grid tokens' outputs and the snapshot tokens' mean output keep weights of their own, so three
// rows r_k (B, 3, V) and three point fields m_k, dm_k take the place of its c and dm.
//
// Launches: fwd  gram_kernel -> softmax_mix_kernel (one workgroup per bag) -> fuse_mix_kernel;
//           bwd  dr_kernel -> mix_bwd_kernel (one workgroup per bag) -> dx_mix_kernel.
// X is read once per launch that touches it (gram, fuse; dr, dx) and nothing of size V x S is
// written besides du.  Every reduction is a fixed-order sum (per-chunk partials added in index
// order, xor-butterfly wave sums): deterministic, no atomics.
#include "baggram.h"   // kGramPts, kGramChunk, token(), gram_kernel
#include "common.h"

#include "blindno.h"

namespace {

using namespace blindno;

constexpr int kMaxTokens = 256;  // V = U + 2 at most (dx_mix_kernel stages V x 64 floats: 64 KB)
constexpr int kDrChunk = 128;    // points per workgroup of the backward's first pass
constexpr int kPts = 64;         // points per workgroup of the two fusion passes (lane = point)

__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v = fmaxf(v, __shfl_xor(v, off, 64));
  return v;
}

// nu_t / L of snapshot token t >= 2 (1 for the grid tokens): the weight of row t of P in r_2
__device__ __forceinline__ float row_coef(const float* __restrict__ lw, float invU, int t) {
  return t < 2 ? 1.0f : (lw ? lw[t - 2] : invU);
}

// One workgroup per sample: G = sum of the chunk partials / sqrt(S), P = mass-weighted row
// softmax, r_0 = P[0,:], r_1 = P[1,:], r_2 = sum_{t>=2} (nu_t / L) P[t,:].
__global__ __launch_bounds__(kBlock) void softmax_mix_kernel(const float* __restrict__ partial,
                                                             const float* __restrict__ lw,
                                                             float* __restrict__ P,
                                                             float* __restrict__ r, int V, int S,
                                                             int nch, float Lf, float invU) {
  __shared__ float mass[kMaxTokens], coef[kMaxTokens];
  const int b = blockIdx.x;
  const float scale = rsqrtf((float)S);
  const float* pb = partial + (int64_t)b * nch * V * V;
  float* Pb = P + (int64_t)b * V * V;
  for (int e = threadIdx.x; e < V * V; e += blockDim.x) {
    float g = 0.f;
    for (int c = 0; c < nch; ++c) g += pb[(int64_t)c * V * V + e];
    Pb[e] = g * scale;
  }
  for (int v = threadIdx.x; v < V; v += blockDim.x) {
    mass[v] = (v < 2 || !lw) ? 1.0f : rintf(lw[v - 2] * Lf);
    coef[v] = row_coef(lw, invU, v);
  }
  __syncthreads();
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
  for (int t = wave; t < V; t += nw) {          // one wave per row, lanes over the columns
    float g[kMaxTokens / 64];
    float mx = -INFINITY;
#pragma unroll
    for (int i = 0; i < kMaxTokens / 64; ++i) {
      const int v = lane + 64 * i;
      g[i] = v < V ? Pb[t * V + v] : -INFINITY;
      mx = fmaxf(mx, g[i]);
    }
    mx = wave_max(mx);
    float den = 0.f;
#pragma unroll
    for (int i = 0; i < kMaxTokens / 64; ++i) {
      const int v = lane + 64 * i;
      g[i] = v < V ? mass[v] * expf(g[i] - mx) : 0.f;
      den += g[i];
    }
    const float inv = 1.0f / wave_sum(den);
#pragma unroll
    for (int i = 0; i < kMaxTokens / 64; ++i) {
      const int v = lane + 64 * i;
      if (v < V) Pb[t * V + v] = g[i] * inv;
    }
  }
  __syncthreads();
  float* rb = r + (int64_t)b * 3 * V;
  for (int v = threadIdx.x; v < V; v += blockDim.x) {
    float acc = 0.f;
    for (int t = 2; t < V; ++t) acc = fmaf(coef[t], Pb[t * V + v], acc);
    rb[v] = Pb[v];
    rb[V + v] = Pb[V + v];
    rb[2 * V + v] = acc;
  }
}

// m_k[p] = sum_v r_k[v] X[v,p]; y[b,p,ch] = sum_k W[ch,k] m_k[p] + bias[ch].  64 points per
// workgroup (lane = point); the waves split the token rows and their partial sums are added in
// wave order.
__global__ __launch_bounds__(kBlock) void fuse_mix_kernel(const float* __restrict__ grid,
                                                          const float* __restrict__ u,
                                                          const float* __restrict__ r,
                                                          const float* __restrict__ W,
                                                          const float* __restrict__ bias,
                                                          float* __restrict__ y, int U, int S,
                                                          int width) {
  __shared__ float part[kBlock / 64][3][kPts];
  __shared__ float ms[3][kPts];
  const int V = U + 2, b = blockIdx.y;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
  const int p0 = blockIdx.x * kPts, p = p0 + lane;
  const float* rb = r + (int64_t)b * 3 * V;
  const int per = (V + nw - 1) / nw, v0 = wave * per, v1 = min(V, v0 + per);
  float a0 = 0.f, a1 = 0.f, a2 = 0.f;
  if (p < S) {
    for (int v = v0; v < v1; ++v) {
      const float x = token(grid, u, b, v, p, U, S);
      a0 = fmaf(rb[v], x, a0);
      a1 = fmaf(rb[V + v], x, a1);
      a2 = fmaf(rb[2 * V + v], x, a2);
    }
  }
  part[wave][0][lane] = a0;
  part[wave][1][lane] = a1;
  part[wave][2][lane] = a2;
  __syncthreads();
  if (threadIdx.x < 3 * kPts) {
    const int k = threadIdx.x >> 6;
    float m = part[0][k][lane];
    for (int w = 1; w < nw; ++w) m += part[w][k][lane];
    ms[k][lane] = m;
  }
  __syncthreads();
  const int n = min(kPts, S - p0);
  float* yb = y + ((int64_t)b * S + p0) * width;
  for (int e = threadIdx.x; e < n * width; e += blockDim.x) {
    const int q = e / width, ch = e - q * width;
    float v = fmaf(W[ch * 3], ms[0][q], bias[ch]);
    v = fmaf(W[ch * 3 + 1], ms[1][q], v);
    yb[e] = fmaf(W[ch * 3 + 2], ms[2][q], v);
  }
}

// dm_k[b,p] = sum_ch W[ch,k] dy[b,p,ch]; partial[b][c][k][v] = sum_{p in chunk c} X[v,p] dm_k[p]
// (one wave per token row, lanes over the chunk's points: coalesced).
__global__ __launch_bounds__(kBlock) void dr_kernel(const float* __restrict__ grid,
                                                    const float* __restrict__ u,
                                                    const float* __restrict__ dy,
                                                    const float* __restrict__ W,
                                                    float* __restrict__ dm,
                                                    float* __restrict__ partial, int U, int S,
                                                    int width, int nch) {
  __shared__ float dml[3][kDrChunk];
  const int V = U + 2, b = blockIdx.y, c = blockIdx.x;
  const int p0 = c * kDrChunk, n = min(S - p0, kDrChunk);
  for (int e = threadIdx.x; e < 3 * n; e += blockDim.x) {
    const int k = e / n, q = e - k * n;
    const float* d = dy + ((int64_t)b * S + p0 + q) * width;
    float v = 0.f;
    for (int ch = 0; ch < width; ++ch) v = fmaf(W[ch * 3 + k], d[ch], v);
    dml[k][q] = v;
    dm[((int64_t)b * 3 + k) * S + p0 + q] = v;
  }
  __syncthreads();
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
  float* pc = partial + ((int64_t)b * nch + c) * 3 * V;
  for (int v = wave; v < V; v += nw) {
    float a0 = 0.f, a1 = 0.f, a2 = 0.f;
    for (int q = lane; q < n; q += 64) {
      const float x = token(grid, u, b, v, p0 + q, U, S);
      a0 = fmaf(x, dml[0][q], a0);
      a1 = fmaf(x, dml[1][q], a1);
      a2 = fmaf(x, dml[2][q], a2);
    }
    a0 = wave_sum(a0);
    a1 = wave_sum(a1);
    a2 = wave_sum(a2);
    if (lane == 0) {
      pc[v] = a0;
      pc[V + v] = a1;
      pc[2 * V + v] = a2;
    }
  }
}

// One workgroup per sample: dr = sum of the chunk partials; dP[t,:] = coef_t dr_{min(t,2)};
// dG = P o (dP - rowsum(P o dP)); M = (dG + dG^T) / sqrt(S).
__global__ __launch_bounds__(kBlock) void mix_bwd_kernel(const float* __restrict__ partial,
                                                         const float* __restrict__ P,
                                                         const float* __restrict__ lw,
                                                         float* __restrict__ M, int V, int S,
                                                         int nch, float invU) {
  __shared__ float dr[3][kMaxTokens], rs[kMaxTokens], coef[kMaxTokens];
  const int b = blockIdx.x;
  const float scale = rsqrtf((float)S);
  const float* Pb = P + (int64_t)b * V * V;
  for (int e = threadIdx.x; e < 3 * V; e += blockDim.x) {
    const int k = e / V, v = e - k * V;
    float a = 0.f;
    for (int c = 0; c < nch; ++c) a += partial[((int64_t)b * nch + c) * 3 * V + e];
    dr[k][v] = a;
  }
  for (int v = threadIdx.x; v < V; v += blockDim.x) coef[v] = row_coef(lw, invU, v);
  __syncthreads();
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
  for (int t = wave; t < V; t += nw) {          // rs[t] = sum_v P[t,v] dr_{k(t)}[v]
    const float* d = dr[min(t, 2)];
    float a = 0.f;
    for (int v = lane; v < V; v += 64) a = fmaf(Pb[t * V + v], d[v], a);
    a = wave_sum(a);
    if (lane == 0) rs[t] = a;
  }
  __syncthreads();
  float* Mb = M + (int64_t)b * V * V;
  for (int e = threadIdx.x; e < V * V; e += blockDim.x) {
    const int t = e / V, v = e - t * V;
    const float d1 = Pb[t * V + v] * coef[t] * (dr[min(t, 2)][v] - rs[t]);
    const float d2 = Pb[v * V + t] * coef[v] * (dr[min(v, 2)][t] - rs[v]);
    Mb[e] = (d1 + d2) * scale;
  }
}

// dX[v,p] = sum_k r_k[v] dm_k[p] + sum_t M[v,t] X[t,p]: the workgroup stages X[:, 64 points] in
// LDS, lane = point, each wave produces 8 token rows per pass.  Rows 0,1 (grid tokens) go to dgt
// (B,2,S) when it is non-null, rows v >= 2 to du (B,U,S).
constexpr int kDxRows = 8;
__global__ __launch_bounds__(kBlock) void dx_mix_kernel(const float* __restrict__ grid,
                                                        const float* __restrict__ u,
                                                        const float* __restrict__ dm,
                                                        const float* __restrict__ r,
                                                        const float* __restrict__ M,
                                                        float* __restrict__ du,
                                                        float* __restrict__ dgt, int U, int S) {
  extern __shared__ float xs[];          // [V][64]
  const int V = U + 2, b = blockIdx.y;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
  const int p0 = blockIdx.x * kPts, p = p0 + lane;
  const bool ok = p < S;
  for (int e = threadIdx.x; e < V * kPts; e += blockDim.x) {
    const int t = e >> 6, q = e & 63;
    xs[e] = p0 + q < S ? token(grid, u, b, t, p0 + q, U, S) : 0.f;
  }
  __syncthreads();
  float dmp[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) dmp[k] = ok ? dm[((int64_t)b * 3 + k) * S + p] : 0.f;
  const float* Mb = M + (int64_t)b * V * V;
  const float* rb = r + (int64_t)b * 3 * V;
  const int v_first = dgt ? 0 : 2;
  for (int s0 = v_first + wave * kDxRows; s0 < V; s0 += nw * kDxRows) {
    float acc[kDxRows];
    const float* mr[kDxRows];
#pragma unroll
    for (int i = 0; i < kDxRows; ++i) {
      const int s = min(s0 + i, V - 1);
      mr[i] = Mb + (int64_t)s * V;
      acc[i] = fmaf(rb[2 * V + s], dmp[2], fmaf(rb[V + s], dmp[1], rb[s] * dmp[0]));
    }
    for (int t = 0; t < V; ++t) {
      const float x = xs[t * kPts + lane];
#pragma unroll
      for (int i = 0; i < kDxRows; ++i) acc[i] = fmaf(mr[i][t], x, acc[i]);
    }
    if (ok) {
#pragma unroll
      for (int i = 0; i < kDxRows; ++i) {
        const int s = s0 + i;
        if (s >= V) break;
        if (s < 2) dgt[((int64_t)b * 2 + s) * S + p] = acc[i];
        else du[((int64_t)b * U + (s - 2)) * S + p] = acc[i];
      }
    }
  }
}

inline bool shape_ok(int B, int U, int S, int width) {
  return B >= 1 && B <= 65535 && U >= 1 && U + 2 <= kMaxTokens && S >= 1 && width >= 1;
}

}  // namespace

BLINDNO_API int blindno_bagattn_mix_ok(int B, int U, int S, int width) {
  return shape_ok(B, U, S, width) ? 1 : 0;
}

BLINDNO_API int blindno_bagattn_mix_nchunk(int S) {
  return S >= 1 ? (S + kGramChunk - 1) / kGramChunk : -1;
}

BLINDNO_API int blindno_bagattn_mix_bwd_nchunk(int S) {
  return S >= 1 ? (S + kDrChunk - 1) / kDrChunk : -1;
}

BLINDNO_API int64_t blindno_bagattn_mix_fwd_scratch_floats(int B, int U, int S) {
  if (!shape_ok(B, U, S, 1)) return -1;
  const int64_t V = U + 2;
  return (int64_t)B * blindno_bagattn_mix_nchunk(S) * V * V;
}

BLINDNO_API int64_t blindno_bagattn_mix_bwd_scratch_floats(int B, int U, int S) {
  if (!shape_ok(B, U, S, 1)) return -1;
  const int64_t V = U + 2;
  return (int64_t)B * 3 * S + (int64_t)B * blindno_bagattn_mix_bwd_nchunk(S) * 3 * V +
         (int64_t)B * V * V;
}

BLINDNO_API int blindno_bagattn_mix_fwd(const float* grid, const float* u, const float* W,
                                        const float* bias, const float* lw, float* scratch,
                                        float* P, float* r, float* y, int B, int U, int S,
                                        int width, int L, blindno_stream_t stream) {
  if (!shape_ok(B, U, S, width) || !grid || !u || !W || !bias || !scratch || !P || !r || !y ||
      (lw && L < U))
    return (int)hipErrorInvalidValue;
  const int V = U + 2, nch = blindno_bagattn_mix_nchunk(S);
  const int nb = (V + 3) / 4, rounds = (nb * (nb + 1) / 2 + kBlock - 1) / kBlock;
  const float invU = 1.0f / (float)U;
  hipStream_t st = (hipStream_t)stream;
  gram_kernel<<<dim3(nch, rounds, B), kBlock, V * (kGramPts + 1) * sizeof(float), st>>>(
      grid, u, scratch, U, S, nch);
  softmax_mix_kernel<<<B, kBlock, 0, st>>>(scratch, lw, P, r, V, S, nch, (float)L, invU);
  fuse_mix_kernel<<<dim3((S + kPts - 1) / kPts, B), kBlock, 0, st>>>(grid, u, r, W, bias, y, U, S,
                                                                    width);
  return (int)hipGetLastError();
}

BLINDNO_API int blindno_bagattn_mix_bwd(const float* grid, const float* u, const float* dy,
                                        const float* W, const float* lw, const float* P,
                                        const float* r, float* scratch, float* du, float* dgt,
                                        int B, int U, int S, int width, int L,
                                        blindno_stream_t stream) {
  if (!shape_ok(B, U, S, width) || !grid || !u || !dy || !W || !P || !r || !scratch || !du ||
      (lw && L < U))
    return (int)hipErrorInvalidValue;
  const int V = U + 2, nch = blindno_bagattn_mix_bwd_nchunk(S);
  const float invU = 1.0f / (float)U;
  float* dm = scratch;
  float* partial = dm + (int64_t)B * 3 * S;
  float* M = partial + (int64_t)B * nch * 3 * V;
  hipStream_t st = (hipStream_t)stream;
  dr_kernel<<<dim3(nch, B), kBlock, 0, st>>>(grid, u, dy, W, dm, partial, U, S, width, nch);
  mix_bwd_kernel<<<B, kBlock, 0, st>>>(partial, P, lw, M, V, S, nch, invU);
  dx_mix_kernel<<<dim3((S + kPts - 1) / kPts, B), kBlock, V * kPts * sizeof(float), st>>>(
      grid, u, dm, r, M, du, dgt, U, S);
  return (int)hipGetLastError();
}
