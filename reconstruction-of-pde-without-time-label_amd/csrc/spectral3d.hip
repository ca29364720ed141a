// The 3D Fourier layer: SpectralConv3d / FNO3d.
//
// Reference operation (yl602019618/Reconstruction-of-PDE-without-Time-Label):
//   SpectralConv3d.forward  2d_FPE/FNOModules.py:270-288  (rfftn over the last three axes ->
//   compl_mul3d on the four kept corner blocks, assigned in the order weights1..4 ->
//   irfftn(s = (P1, P2, P3)));  FNO3d.forward 2d_FPE/FNOModules.py:334-366.
// The padded field x[n][c][x][y][z] is the 2D field x[n][c][h][w] with h = x P2 + y (P1 P2 rows)
// and w = z, so the last-axis transforms, the 1x1 conv epilogue and the conv weight gradient are
// the 2D row kernels on that view (spectral.hip, rowinv.hip, fields.hip).  This file adds what
// the view cannot give: the two truncated transforms over y and x around the channel mix
// (blindno_colpass3d), the four-corner weight pack, and the lift / projection with a pad and a
// crop on three axes.
#include "common.h"
#include "blindno.h"
#include "kernels.h"

using namespace blindno;

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

// ------------------------------------------------------------------------ complex tile GEMM
// One wave: D (the 16 x 16 tile at (i0, j0)) = sum_{k < K} A[i][k] B[k][j], complex, as four
// real v_mfma_f32_16x16x4f32 per 4-deep K step (exact fp32 products, fp32 accumulation, k in
// ascending order: a fixed summation order).  Lane l supplies A[i0 + (l & 15)][k0 + (l >> 4)] and
// B[k0 + (l >> 4)][j0 + (l & 15)] and ends with D[i0 + 4 (l >> 4) + r][j0 + (l & 15)] in
// component r.  Element (i, k) of A is A[i a_si + k a_sk], (k, j) of B is B[k b_sk + j b_sj];
// operands outside M x K / K x N count as zero and are never read.  CA / CB conjugate A / B.
template <bool CA, bool CB>
__device__ __forceinline__ void cgemm_tile(const float2* A, int a_si, int a_sk, const float2* B,
                                           int b_sk, int b_sj, int M, int N, int K, int i0,
                                           int j0, f32x4& dre, f32x4& dim) {
  const int lane = threadIdx.x & 63, c16 = lane & 15, g4 = lane >> 4;
  const int ai = i0 + c16, bj = j0 + c16;
  const bool aok = ai < M, bok = bj < N;
  dre = f32x4{0.f, 0.f, 0.f, 0.f};
  dim = f32x4{0.f, 0.f, 0.f, 0.f};
  for (int k0 = 0; k0 < K; k0 += 4) {
    const int k = k0 + g4;
    float2 a = make_float2(0.f, 0.f), b = make_float2(0.f, 0.f);
    if (aok && k < K) a = A[ai * a_si + k * a_sk];
    if (bok && k < K) b = B[k * b_sk + bj * b_sj];
    if (CA) a.y = -a.y;
    if (CB) b.y = -b.y;
    dre = __builtin_amdgcn_mfma_f32_16x16x4f32(a.x, b.x, dre, 0, 0, 0);
    dre = __builtin_amdgcn_mfma_f32_16x16x4f32(-a.y, b.y, dre, 0, 0, 0);
    dim = __builtin_amdgcn_mfma_f32_16x16x4f32(a.x, b.y, dim, 0, 0, 0);
    dim = __builtin_amdgcn_mfma_f32_16x16x4f32(a.y, b.x, dim, 0, 0, 0);
  }
}

// ------------------------------------------------------------------------ colpass3d
// Forward transforms of one (sample, k3, channel) plane: workgroup b = (n m3 + k3) C + c reads
// the P1 x P2 complex plane At[b][x P2 + y], forms T1[x][jy] = sum_y plane[x][y] Ty[y][jy] in LDS
// (y first: the plane shrinks to P1 x K2), then Xs[b][jx K2 + jy] = sum_x Tx[x][jx] T1[x][jy].
// Ty (P2 x K2), Tx (P1 x K1): e^{-2 pi i r_j p / P} at the kept frequencies r_j.
__global__ __launch_bounds__(256) void dft3d_kernel(const float2* __restrict__ At,
                                                    float2* __restrict__ Xs,
                                                    const float2* __restrict__ Ty,
                                                    const float2* __restrict__ Tx, int P1, int P2,
                                                    int K1, int K2) {
  extern __shared__ float smem3d[];
  float2* T1 = reinterpret_cast<float2*>(smem3d);                 // [P1][K2]
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, c16 = lane & 15, g4 = lane >> 4;
  const float2* plane = At + (int64_t)blockIdx.x * P1 * P2;
  const int ntj = (K2 + 15) >> 4;
  f32x4 dre, dim;
  for (int t = wave; t < ((P1 + 15) >> 4) * ntj; t += 4) {
    const int i0 = (t / ntj) * 16, j0 = (t % ntj) * 16;
    cgemm_tile<false, false>(plane, P2, 1, Ty, K2, 1, P1, K2, P2, i0, j0, dre, dim);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int i = i0 + 4 * g4 + r, j = j0 + c16;
      if (i < P1 && j < K2) T1[i * K2 + j] = make_float2(dre[r], dim[r]);
    }
  }
  __syncthreads();
  float2* out = Xs + (int64_t)blockIdx.x * K1 * K2;
  for (int t = wave; t < ((K1 + 15) >> 4) * ntj; t += 4) {
    const int i0 = (t / ntj) * 16, j0 = (t % ntj) * 16;
    cgemm_tile<false, false>(Tx, 1, K1, T1, K2, 1, K1, K2, P1, i0, j0, dre, dim);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int i = i0 + 4 * g4 + r, j = j0 + c16;
      if (i < K1 && j < K2) out[i * K2 + j] = make_float2(dre[r], dim[r]);
    }
  }
}

// Channel mix at every kept (k3, j): DIR 0  Y[b][o][j] = sum_i Xs[b][i][j] Wt[k3][j][i][o],
// DIR 1 (adjoint)  Y[b][i][j] = sum_o Xs[b][o][j] conj(Wt[k3][j][i][o]); channels in ascending
// order.
template <int DIR>
__global__ __launch_bounds__(256) void mix3d_kernel(const float2* __restrict__ Xs,
                                                    const float2* __restrict__ Wt,
                                                    float2* __restrict__ Y, int64_t total, int Ci,
                                                    int Co, int KK, int m3) {
  const int cin = DIR ? Co : Ci, cout = DIR ? Ci : Co;
  for (int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x; idx < total;
       idx += (int64_t)gridDim.x * 256) {
    const int j = (int)(idx % KK);
    const int64_t t = idx / KK;
    const int o = (int)(t % cout);
    const int64_t b = t / cout;
    const int k3 = (int)(b % m3);
    const float2* x = Xs + b * cin * KK + j;
    const float2* w = Wt + ((int64_t)k3 * KK + j) * Ci * Co;
    float re = 0.f, im = 0.f;
    for (int i = 0; i < cin; ++i) {
      const float2 a = x[(int64_t)i * KK];
      float2 wv = DIR ? w[o * Co + i] : w[i * Co + o];
      if (DIR) wv.y = -wv.y;
      re = fmaf(a.x, wv.x, fmaf(-a.y, wv.y, re));
      im = fmaf(a.x, wv.y, fmaf(a.y, wv.x, im));
    }
    Y[idx] = make_float2(re, im);
  }
}

// Inverse transforms of one (sample, k3, channel): workgroup b C + c reads Y[b][c][jx K2 + jy],
// forms U[x][jy] = sum_jx conj(Tx[x][jx]) Y[jx][jy] in LDS, then the row coefficients
// Z[n][x P2 + y][k3][c] = sum_jy U[x][jy] conj(Ty[y][jy]).  TILE: Z in the A-tile order of
// blindno_spectrum_tile_layout (the wide row inverse's), else Z[n][h][k][c].
template <bool TILE>
__global__ __launch_bounds__(256) void idft3d_kernel(const float2* __restrict__ Y,
                                                     float* __restrict__ Z,
                                                     const float2* __restrict__ Ty,
                                                     const float2* __restrict__ Tx, int C, int P1,
                                                     int P2, int K1, int K2, int m3) {
  extern __shared__ float smem3d[];
  float2* U = reinterpret_cast<float2*>(smem3d);                  // [P1][K2]
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, c16 = lane & 15, g4 = lane >> 4;
  const int c = blockIdx.x % C, b = blockIdx.x / C;
  const int k3 = b % m3, n = b / m3;
  const float2* yo = Y + (int64_t)blockIdx.x * K1 * K2;
  const int ntj = (K2 + 15) >> 4;
  f32x4 dre, dim;
  for (int t = wave; t < ((P1 + 15) >> 4) * ntj; t += 4) {
    const int i0 = (t / ntj) * 16, j0 = (t % ntj) * 16;
    cgemm_tile<true, false>(Tx, K1, 1, yo, K2, 1, P1, K2, K1, i0, j0, dre, dim);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int i = i0 + 4 * g4 + r, j = j0 + c16;
      if (i < P1 && j < K2) U[i * K2 + j] = make_float2(dre[r], dim[r]);
    }
  }
  __syncthreads();
  const int nty = (P2 + 15) >> 4;
  const int64_t row0 = (int64_t)n * P1 * P2;
  for (int t = wave; t < ((P1 + 15) >> 4) * nty; t += 4) {
    const int i0 = (t / nty) * 16, j0 = (t % nty) * 16;
    cgemm_tile<false, true>(U, K2, 1, Ty, 1, K2, P1, P2, K2, i0, j0, dre, dim);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int x = i0 + 4 * g4 + r, y = j0 + c16;
      if (x < P1 && y < P2) {
        const int64_t R = row0 + (int64_t)x * P2 + y;
        if (TILE) {
          const int64_t q = R >> 2;
          const int ri = (int)(R & 3), g = c >> 2, ci = c & 3;
#pragma unroll
          for (int p = 0; p < 2; ++p) {
            const int kk = 2 * k3 + p;
            const int l = (kk & 3) * 16 + ri * 4 + ci;
            Z[((q * (C >> 2) + g) * (m3 >> 1) + (kk >> 2)) * 64 + l] = p ? dim[r] : dre[r];
          }
        } else {
          reinterpret_cast<float2*>(Z)[(R * m3 + k3) * C + c] = make_float2(dre[r], dim[r]);
        }
      }
    }
  }
}

// ------------------------------------------------------------------------ weight pack
// The corner (0..3 = weights1..4) that owns frequency (r1, r2) of the kept set: the reference
// assigns weights1..4 in order, so the last corner that contains the frequency wins.
__device__ __forceinline__ int corner_of(int r1, int r2, int m1, int m2, int P1, int P2) {
  const bool hi1 = r1 >= P1 - m1, hi2 = r2 >= P2 - m2, lo1 = r1 < m1;
  if (hi1 && hi2) return 3;
  if (lo1 && hi2) return 2;
  if (hi1) return 1;
  return 0;
}

struct W3d {
  float2* w[4];
};

// DIR 0: Wt[k3][jx K2 + jy][ci][co] = s_k3 w_q[ci][co][ix][iy][k3] with q the owning corner and
// s_k3 = c_k3 / (P1 P2 P3) (the Hermitian weight of the last-axis C2R and irfftn's 1/N).
// DIR 1: dw_q[ci][co][ix][iy][k3] = s_k3 dWt[...] where corner q owns its frequency, else 0.
template <int DIR>
__global__ __launch_bounds__(256) void packw3d_kernel(W3d ws, float2* __restrict__ Wt, int Ci,
                                                      int Co, int m1, int m2, int m3, int P1,
                                                      int P2, int P3, float inv, int64_t total) {
  const int K1 = kept_rows_count(m1, P1), K2 = kept_rows_count(m2, P2);
  for (int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x; idx < total;
       idx += (int64_t)gridDim.x * 256) {
    if (DIR == 0) {
      const int co = (int)(idx % Co);
      int64_t t = idx / Co;
      const int ci = (int)(t % Ci);
      t /= Ci;
      const int j = (int)(t % (K1 * K2)), k3 = (int)(t / (K1 * K2));
      const int r1 = kept_row(j / K2, K1, m1, P1), r2 = kept_row(j % K2, K2, m2, P2);
      const int q = corner_of(r1, r2, m1, m2, P1, P2);
      const int ix = (q & 1) ? r1 - (P1 - m1) : r1, iy = (q & 2) ? r2 - (P2 - m2) : r2;
      const float2 v = ws.w[q][((((int64_t)ci * Co + co) * m1 + ix) * m2 + iy) * m3 + k3];
      const float s = c2r_weight(k3, P3) * inv;
      Wt[idx] = make_float2(v.x * s, v.y * s);
    } else {
      const int k3 = (int)(idx % m3);
      int64_t t = idx / m3;
      const int iy = (int)(t % m2);
      t /= m2;
      const int ix = (int)(t % m1);
      t /= m1;
      const int co = (int)(t % Co);
      t /= Co;
      const int ci = (int)(t % Ci), q = (int)(t / Ci);
      const int r1 = (q & 1) ? P1 - m1 + ix : ix, r2 = (q & 2) ? P2 - m2 + iy : iy;
      float2 v = make_float2(0.f, 0.f);
      if (corner_of(r1, r2, m1, m2, P1, P2) == q) {
        const int jx = (K1 == P1 || r1 < m1) ? r1 : r1 - (P1 - 2 * m1);
        const int jy = (K2 == P2 || r2 < m2) ? r2 : r2 - (P2 - 2 * m2);
        const float2 g = Wt[(((int64_t)k3 * K1 * K2 + jx * K2 + jy) * Ci + ci) * Co + co];
        const float s = c2r_weight(k3, P3) * inv;
        v = make_float2(g.x * s, g.y * s);
      }
      ws.w[q][((((int64_t)ci * Co + co) * m1 + ix) * m2 + iy) * m3 + k3] = v;
    }
  }
}

// ------------------------------------------------------------------------ lift
// x0[n][c][x][y][z] = b0[c] + sum_i w0[c][i] in[n][x][y][z][i] inside the N1 x N2 x N3 grid,
// 0 on the right pad of every axis.
__global__ __launch_bounds__(256) void lift3d_fwd_kernel(const float* __restrict__ in,
                                                         const float* __restrict__ w0,
                                                         const float* __restrict__ b0,
                                                         float* __restrict__ x0, int64_t total,
                                                         int N1, int N2, int N3, int Cin, int C,
                                                         int P1, int P2, int P3) {
  for (int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x; idx < total;
       idx += (int64_t)gridDim.x * 256) {
    const int z = (int)(idx % P3);
    int64_t t = idx / P3;
    const int y = (int)(t % P2);
    t /= P2;
    const int x = (int)(t % P1);
    t /= P1;
    const int c = (int)(t % C);
    const int64_t n = t / C;
    float v = 0.f;
    if (x < N1 && y < N2 && z < N3) {
      const float* ip = in + (((n * N1 + x) * N2 + y) * N3 + z) * Cin;
      v = b0[c];
      for (int i = 0; i < Cin; ++i) v = fmaf(w0[c * Cin + i], ip[i], v);
    }
    x0[idx] = v;
  }
}

constexpr int kLiftStride = 257;   // LDS row stride of a 256-point tile (odd: no bank conflicts)

// Backward of the lift over tiles of 256 grid points: d_in[p][i] = sum_c dx0[c][p] w0[c][i]
// (optional) and the workgroup's partial sums [dW0[c][i] = sum_p dx0[c][p] in[p][i] | db0[c]],
// parameter e owned by thread e % 256, points in ascending order.
__global__ __launch_bounds__(256) void lift3d_bwd_kernel(
    const float* __restrict__ dx0, const float* __restrict__ in, const float* __restrict__ w0,
    float* __restrict__ d_in, float* __restrict__ partial, int64_t npts, int N1, int N2, int N3,
    int Cin, int C, int P1, int P2, int P3) {
  extern __shared__ float smem3d[];
  float* sd = smem3d;                              // [C][257]
  float* si = smem3d + C * kLiftStride;            // [Cin][257]
  const int tid = threadIdx.x;
  const int np = C * Cin + C;
  float acc[4] = {0.f, 0.f, 0.f, 0.f};
  const int64_t ntiles = (npts + 255) / 256;
  for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const int64_t pt = tile * 256 + tid;
    if (pt < npts) {
      const int z = (int)(pt % N3);
      int64_t t = pt / N3;
      const int y = (int)(t % N2);
      t /= N2;
      const int x = (int)(t % N1);
      const int64_t n = t / N1;
      for (int c = 0; c < C; ++c)
        sd[c * kLiftStride + tid] = dx0[(((n * C + c) * P1 + x) * P2 + y) * P3 + z];
      for (int i = 0; i < Cin; ++i) si[i * kLiftStride + tid] = in[pt * Cin + i];
      if (d_in) {
        for (int i = 0; i < Cin; ++i) {
          float s = 0.f;
          for (int c = 0; c < C; ++c) s = fmaf(sd[c * kLiftStride + tid], w0[c * Cin + i], s);
          d_in[pt * Cin + i] = s;
        }
      }
    } else {
      for (int c = 0; c < C; ++c) sd[c * kLiftStride + tid] = 0.f;
      for (int i = 0; i < Cin; ++i) si[i * kLiftStride + tid] = 0.f;
    }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int e = tid + 256 * q;
      if (e < np) {
        float s = acc[q];
        if (e < C * Cin) {
          const float* a = sd + (e / Cin) * kLiftStride;
          const float* b = si + (e % Cin) * kLiftStride;
          for (int t = 0; t < 256; ++t) s = fmaf(a[t], b[t], s);
        } else {
          const float* a = sd + (e - C * Cin) * kLiftStride;
          for (int t = 0; t < 256; ++t) s += a[t];
        }
        acc[q] = s;
      }
    }
    __syncthreads();
  }
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int e = tid + 256 * q;
    if (e < np) partial[(int64_t)blockIdx.x * np + e] = acc[q];
  }
}

// ------------------------------------------------------------------------ projection
constexpr int kProjMaxCout = 8;

// out[n][x][y][z][o] = b2[o] + sum_j w2[o][j] GELU(b1[j] + sum_c w1[j][c] z[n][c][x][y][z]) on
// the crop x < N1, y < N2, z < N3; one thread per point, its channel column in LDS.
__global__ __launch_bounds__(256) void project3d_fwd_kernel(
    const float* __restrict__ z, const float* __restrict__ w1, const float* __restrict__ b1,
    const float* __restrict__ w2, const float* __restrict__ b2, float* __restrict__ out,
    int64_t npts, int C, int P1, int P2, int P3, int N1, int N2, int N3, int Hd, int Cout) {
  extern __shared__ float smem3d[];
  float* zs = smem3d;                              // [C][256]
  const int tid = threadIdx.x;
  const int64_t pt = (int64_t)blockIdx.x * 256 + tid;
  if (pt >= npts) return;                          // no barrier below: each thread reads its own column
  const int zz = (int)(pt % N3);
  int64_t t = pt / N3;
  const int y = (int)(t % N2);
  t /= N2;
  const int x = (int)(t % N1);
  const int64_t n = t / N1;
  for (int c = 0; c < C; ++c) zs[c * 256 + tid] = z[(((n * C + c) * P1 + x) * P2 + y) * P3 + zz];
  float acc[kProjMaxCout];
#pragma unroll
  for (int o = 0; o < kProjMaxCout; ++o) acc[o] = o < Cout ? b2[o] : 0.f;
  for (int j = 0; j < Hd; ++j) {
    float h = b1[j];
    for (int c = 0; c < C; ++c) h = fmaf(w1[j * C + c], zs[c * 256 + tid], h);
    const float g = gelu_f(h);
#pragma unroll
    for (int o = 0; o < kProjMaxCout; ++o)
      if (o < Cout) acc[o] = fmaf(w2[o * Hd + j], g, acc[o]);
  }
#pragma unroll
  for (int o = 0; o < kProjMaxCout; ++o)
    if (o < Cout) out[pt * Cout + o] = acc[o];
}

constexpr int kPbPts = 32;      // points per tile of the projection backward
constexpr int kPbStride = 33;

// Backward of the projection over tiles of 32 crop points, the hidden layer recomputed in LDS
// (never written to HBM): dz on the crop, and the workgroup's partial sums
// [dW1 (Hd C) | db1 (Hd) | dW2 (Cout Hd) | db2 (Cout)] kept in its own row of `partial` across its
// tiles (parameter e owned by thread e % 256, tiles and points in ascending order).
__global__ __launch_bounds__(256) void project3d_bwd_kernel(
    const float* __restrict__ z, const float* __restrict__ w1, const float* __restrict__ b1,
    const float* __restrict__ w2, const float* __restrict__ dout, float* __restrict__ dz,
    float* __restrict__ partial, int64_t npts, int C, int P1, int P2, int P3, int N1, int N2,
    int N3, int Hd, int Cout) {
  extern __shared__ float smem3d[];
  float* sg = smem3d;                              // [Hd][33] GELU(h)
  float* sdh = sg + Hd * kPbStride;                // [Hd][33] dL/dh
  float* zs = sdh + Hd * kPbStride;                // [C][33]
  float* dos = zs + C * kPbStride;                 // [Cout][33]
  __shared__ int64_t sbase[kPbPts];
  const int tid = threadIdx.x;
  const int np = Hd * C + Hd + Cout * Hd + Cout;
  float* prow = partial + (int64_t)blockIdx.x * np;
  const int64_t ntiles = (npts + kPbPts - 1) / kPbPts;
  bool first = true;
  for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    if (tid < kPbPts) {
      const int64_t pt = tile * kPbPts + tid;
      int64_t base = -1;
      if (pt < npts) {
        const int zz = (int)(pt % N3);
        int64_t t = pt / N3;
        const int y = (int)(t % N2);
        t /= N2;
        const int x = (int)(t % N1);
        const int64_t n = t / N1;
        base = ((n * C * P1 + x) * P2 + y) * P3 + zz;
      }
      sbase[tid] = base;
    }
    __syncthreads();
    const int64_t cs = (int64_t)P1 * P2 * P3;
    for (int e = tid; e < (C + Cout) * kPbPts; e += 256) {
      const int p = e & (kPbPts - 1), r = e / kPbPts;
      const int64_t base = sbase[p];
      if (r < C) zs[r * kPbStride + p] = base >= 0 ? z[base + r * cs] : 0.f;
      else dos[(r - C) * kPbStride + p] = base >= 0 ? dout[(tile * kPbPts + p) * Cout + (r - C)] : 0.f;
    }
    __syncthreads();
    for (int e = tid; e < Hd * kPbPts; e += 256) {
      const int p = e & (kPbPts - 1), j = e / kPbPts;
      float h = b1[j];
      for (int c = 0; c < C; ++c) h = fmaf(w1[j * C + c], zs[c * kPbStride + p], h);
      float g, dg;
      gelu_both(h, g, dg);
      float ds = 0.f;
      for (int o = 0; o < Cout; ++o) ds = fmaf(w2[o * Hd + j], dos[o * kPbStride + p], ds);
      sg[j * kPbStride + p] = g;
      sdh[j * kPbStride + p] = ds * dg;
    }
    __syncthreads();
    for (int e = tid; e < C * kPbPts; e += 256) {
      const int p = e & (kPbPts - 1), c = e / kPbPts;
      const int64_t base = sbase[p];
      if (base >= 0) {
        float s = 0.f;
        for (int j = 0; j < Hd; ++j) s = fmaf(w1[j * C + c], sdh[j * kPbStride + p], s);
        dz[base + c * cs] = s;
      }
    }
    for (int e = tid; e < np; e += 256) {
      float s = first ? 0.f : prow[e];
      int r = e;
      if (r < Hd * C) {
        const float* a = sdh + (r / C) * kPbStride;
        const float* b = zs + (r % C) * kPbStride;
        for (int p = 0; p < kPbPts; ++p) s = fmaf(a[p], b[p], s);
      } else if ((r -= Hd * C) < Hd) {
        const float* a = sdh + r * kPbStride;
        for (int p = 0; p < kPbPts; ++p) s += a[p];
      } else if ((r -= Hd) < Cout * Hd) {
        const float* a = dos + (r / Hd) * kPbStride;
        const float* b = sg + (r % Hd) * kPbStride;
        for (int p = 0; p < kPbPts; ++p) s = fmaf(a[p], b[p], s);
      } else {
        const float* a = dos + (r - Cout * Hd) * kPbStride;
        for (int p = 0; p < kPbPts; ++p) s += a[p];
      }
      prow[e] = s;
    }
    first = false;
    __syncthreads();
  }
}

constexpr size_t kLds3d = 64 * 1024;   // dynamic LDS the kernels of this file may ask for

bool spec3d_shape_ok(int Bn, int Ci, int Co, int P1, int P2, int P3, int m1, int m2, int m3) {
  if (Bn <= 0 || Ci <= 0 || Co <= 0 || Ci > 32 || Co > 32 || P1 <= 0 || P2 <= 0 || P3 <= 0 ||
      m1 <= 0 || m2 <= 0 || m3 <= 0 || m1 > P1 || m2 > P2 || m3 > P3 / 2 + 1 || m3 > 48)
    return false;
  const int K1 = kept_rows_count(m1, P1), K2 = kept_rows_count(m2, P2);
  const int Cm = Ci > Co ? Ci : Co;
  if (sizeof(float2) * (size_t)P1 * K2 > kLds3d) return false;
  // 32-bit element offsets inside a plane / a table, and the row kernels' own limits on the view
  if ((int64_t)P1 * P2 >= (1 << 24) || (int64_t)K1 * K2 * Cm * Cm * m3 >= INT32_MAX / 2) return false;
  if ((int64_t)Bn * m3 * Cm >= INT32_MAX) return false;
  if ((int64_t)Bn * P1 * P2 * m3 * Cm * 2 >= INT32_MAX) return false;
  if ((int64_t)Bn * Cm * P1 * P2 >= INT32_MAX) return false;
  return true;
}

}  // namespace

BLINDNO_API int blindno_spectral3d_ok(int Bn, int Ci, int Co, int P1, int P2, int P3, int m1,
                                      int m2, int m3) {
  return spec3d_shape_ok(Bn, Ci, Co, P1, P2, P3, m1, m2, m3) ? 1 : 0;
}

BLINDNO_API int blindno_colpass3d(const float* At, const float* Wt, float* Xs, float* Y, float* Z,
                                  const float* Tx, const float* Ty, int Bn, int Ci, int Co, int P1,
                                  int P2, int P3, int m1, int m2, int m3, int dir, void* stream) {
  if (!spec3d_shape_ok(Bn, Ci, Co, P1, P2, P3, m1, m2, m3) || (dir != 0 && dir != 1) || !At ||
      !Wt || !Xs || !Y || !Z || !Tx || !Ty)
    return (int)hipErrorInvalidValue;
  const int K1 = kept_rows_count(m1, P1), K2 = kept_rows_count(m2, P2);
  const int cin = dir ? Co : Ci, cout = dir ? Ci : Co;
  hipStream_t st = (hipStream_t)stream;
  const size_t sh = sizeof(float2) * (size_t)P1 * K2;
  dft3d_kernel<<<Bn * m3 * cin, 256, sh, st>>>((const float2*)At, (float2*)Xs, (const float2*)Ty,
                                               (const float2*)Tx, P1, P2, K1, K2);
  int e = (int)hipGetLastError();
  if (e) return e;
  const int64_t total = (int64_t)Bn * m3 * cout * K1 * K2;
  if (dir == 0)
    mix3d_kernel<0><<<grid_for(total, 256, 65536), 256, 0, st>>>(
        (const float2*)Xs, (const float2*)Wt, (float2*)Y, total, Ci, Co, K1 * K2, m3);
  else
    mix3d_kernel<1><<<grid_for(total, 256, 65536), 256, 0, st>>>(
        (const float2*)Xs, (const float2*)Wt, (float2*)Y, total, Ci, Co, K1 * K2, m3);
  e = (int)hipGetLastError();
  if (e) return e;
  if (rowinv_tile_layout(Bn, cout, P1 * P2, P3, m3))
    idft3d_kernel<true><<<Bn * m3 * cout, 256, sh, st>>>((const float2*)Y, Z, (const float2*)Ty,
                                                         (const float2*)Tx, cout, P1, P2, K1, K2, m3);
  else
    idft3d_kernel<false><<<Bn * m3 * cout, 256, sh, st>>>((const float2*)Y, Z, (const float2*)Ty,
                                                          (const float2*)Tx, cout, P1, P2, K1, K2, m3);
  return (int)hipGetLastError();
}

static int packw3d(float* w1, float* w2, float* w3, float* w4, float* Wt, int Ci, int Co, int m1,
                   int m2, int m3, int P1, int P2, int P3, int dir, void* stream) {
  if (!spec3d_shape_ok(1, Ci, Co, P1, P2, P3, m1, m2, m3) || !w1 || !w2 || !w3 || !w4 || !Wt)
    return (int)hipErrorInvalidValue;
  const W3d ws{{(float2*)w1, (float2*)w2, (float2*)w3, (float2*)w4}};
  const float inv = (float)(1.0 / ((double)P1 * P2 * P3));
  const int K1 = kept_rows_count(m1, P1), K2 = kept_rows_count(m2, P2);
  if (dir == 0) {
    const int64_t total = (int64_t)m3 * K1 * K2 * Ci * Co;
    packw3d_kernel<0><<<grid_for(total, 256, 65536), 256, 0, (hipStream_t)stream>>>(
        ws, (float2*)Wt, Ci, Co, m1, m2, m3, P1, P2, P3, inv, total);
  } else {
    const int64_t total = 4 * (int64_t)Ci * Co * m1 * m2 * m3;
    packw3d_kernel<1><<<grid_for(total, 256, 65536), 256, 0, (hipStream_t)stream>>>(
        ws, (float2*)Wt, Ci, Co, m1, m2, m3, P1, P2, P3, inv, total);
  }
  return (int)hipGetLastError();
}

BLINDNO_API int blindno_pack_w3d(const float* w1, const float* w2, const float* w3,
                                 const float* w4, float* Wt, int Ci, int Co, int m1, int m2,
                                 int m3, int P1, int P2, int P3, void* stream) {
  return packw3d(const_cast<float*>(w1), const_cast<float*>(w2), const_cast<float*>(w3),
                 const_cast<float*>(w4), Wt, Ci, Co, m1, m2, m3, P1, P2, P3, 0, stream);
}

BLINDNO_API int blindno_unpack_w3d(const float* dWt, float* dw1, float* dw2, float* dw3,
                                   float* dw4, int Ci, int Co, int m1, int m2, int m3, int P1,
                                   int P2, int P3, void* stream) {
  return packw3d(dw1, dw2, dw3, dw4, const_cast<float*>(dWt), Ci, Co, m1, m2, m3, P1, P2, P3, 1,
                 stream);
}

static bool lift3d_ok(int Bn, int N1, int N2, int N3, int Cin, int C, int P1, int P2, int P3) {
  return Bn > 0 && N1 > 0 && N2 > 0 && N3 > 0 && Cin > 0 && C > 0 && Cin <= 32 && C <= 32 &&
         P1 >= N1 && P2 >= N2 && P3 >= N3 && C * Cin + C <= 1024;
}

BLINDNO_API int blindno_lift3d_fwd(const float* in, const float* w0, const float* b0, float* x0,
                                   int Bn, int N1, int N2, int N3, int Cin, int C, int P1, int P2,
                                   int P3, void* stream) {
  if (!lift3d_ok(Bn, N1, N2, N3, Cin, C, P1, P2, P3) || !in || !w0 || !b0 || !x0)
    return (int)hipErrorInvalidValue;
  const int64_t total = (int64_t)Bn * C * P1 * P2 * P3;
  lift3d_fwd_kernel<<<grid_for(total, 256, 1 << 20), 256, 0, (hipStream_t)stream>>>(
      in, w0, b0, x0, total, N1, N2, N3, Cin, C, P1, P2, P3);
  return (int)hipGetLastError();
}

BLINDNO_API int blindno_lift3d_bwd_nchunk(int Bn, int N1, int N2, int N3) {
  const int64_t tiles = ((int64_t)Bn * N1 * N2 * N3 + 255) / 256;
  return (int)(tiles < 1 ? 1 : (tiles > 1024 ? 1024 : tiles));
}

BLINDNO_API int blindno_lift3d_bwd(const float* dx0, const float* in, const float* w0,
                                   float* d_in, float* partial, int nchunk, int Bn, int N1, int N2,
                                   int N3, int Cin, int C, int P1, int P2, int P3, void* stream) {
  if (!lift3d_ok(Bn, N1, N2, N3, Cin, C, P1, P2, P3) || !dx0 || !in || !w0 || !partial ||
      nchunk != blindno_lift3d_bwd_nchunk(Bn, N1, N2, N3))
    return (int)hipErrorInvalidValue;
  const size_t sh = sizeof(float) * (size_t)(C + Cin) * kLiftStride;
  lift3d_bwd_kernel<<<nchunk, 256, sh, (hipStream_t)stream>>>(
      dx0, in, w0, d_in, partial, (int64_t)Bn * N1 * N2 * N3, N1, N2, N3, Cin, C, P1, P2, P3);
  return (int)hipGetLastError();
}

static bool project3d_ok(int Bn, int C, int P1, int P2, int P3, int N1, int N2, int N3, int Hd,
                         int Cout) {
  return Bn > 0 && C > 0 && C <= 32 && N1 > 0 && N2 > 0 && N3 > 0 && P1 >= N1 && P2 >= N2 &&
         P3 >= N3 && Hd > 0 && Hd <= 128 && Cout > 0 && Cout <= kProjMaxCout;
}

BLINDNO_API int blindno_project3d_fwd(const float* z, const float* w1, const float* b1,
                                      const float* w2, const float* b2, float* out, int Bn, int C,
                                      int P1, int P2, int P3, int N1, int N2, int N3, int Hd,
                                      int Cout, void* stream) {
  if (!project3d_ok(Bn, C, P1, P2, P3, N1, N2, N3, Hd, Cout) || !z || !w1 || !b1 || !w2 || !b2 ||
      !out)
    return (int)hipErrorInvalidValue;
  const int64_t npts = (int64_t)Bn * N1 * N2 * N3;
  if ((npts + 255) / 256 >= INT32_MAX) return (int)hipErrorInvalidValue;
  project3d_fwd_kernel<<<(unsigned)((npts + 255) / 256), 256, sizeof(float) * C * 256,
                         (hipStream_t)stream>>>(z, w1, b1, w2, b2, out, npts, C, P1, P2, P3, N1,
                                                N2, N3, Hd, Cout);
  return (int)hipGetLastError();
}

BLINDNO_API int blindno_project3d_bwd_nchunk(int Bn, int N1, int N2, int N3) {
  const int64_t tiles = ((int64_t)Bn * N1 * N2 * N3 + kPbPts - 1) / kPbPts;
  return (int)(tiles < 1 ? 1 : (tiles > 1024 ? 1024 : tiles));
}

BLINDNO_API int blindno_project3d_bwd(const float* z, const float* w1, const float* b1,
                                      const float* w2, const float* dout, float* dz,
                                      float* partial, int nchunk, int Bn, int C, int P1, int P2,
                                      int P3, int N1, int N2, int N3, int Hd, int Cout,
                                      void* stream) {
  if (!project3d_ok(Bn, C, P1, P2, P3, N1, N2, N3, Hd, Cout) || !z || !w1 || !b1 || !w2 ||
      !dout || !dz || !partial || nchunk != blindno_project3d_bwd_nchunk(Bn, N1, N2, N3))
    return (int)hipErrorInvalidValue;
  hipStream_t st = (hipStream_t)stream;
  // dz is zero on the padding: the whole field is cleared, the kernel writes the crop
  int e = (int)hipMemsetAsync(dz, 0, sizeof(float) * (size_t)Bn * C * P1 * P2 * P3, st);
  if (e) return e;
  const size_t sh = sizeof(float) * (size_t)(2 * Hd + C + Cout) * kPbStride;
  project3d_bwd_kernel<<<nchunk, 256, sh, st>>>(z, w1, b1, w2, dout, dz, partial,
                                                (int64_t)Bn * N1 * N2 * N3, C, P1, P2, P3, N1, N2,
                                                N3, Hd, Cout);
  return (int)hipGetLastError();
}
