// Physics attention of the structured-mesh Transolver (model/Physics_Attention.py:60-116, as
// NIOFP2D_Trans builds it: 4 heads, D = 8 channels per head, G = 16 slices, 32 channels) and the
// LayerNorm over the 32 channel planes, forward and backward, on the plane layout (S, C, H W) that
// blindno_conv2d_* reads and writes.  include/blindno_physattn.h has the formulas.
//
// A thread owns a point: its channels are one coalesced load per plane.  Every reduction over the
// points is a per-workgroup partial (kPts points) followed by a sum of the partials in index
// order; there are no atomics, so a second call is bit-identical.
//
// The workgroup reduction of the 16 x 9 accumulators of a head (tokens, d otok, d Ws): each
// thread puts its 16 slice values and 8 channel values into LDS rows of stride kPts + 1 (an odd
// stride: the 16 rows a wave reads at one point index fall into 16 banks, equal rows broadcast),
// then thread g * 9 + c sums its product over the points in index order with one accumulator.
// No per-thread accumulator array exists, so nothing spills.
#include "common.h"
#include "blindno.h"

using namespace blindno;

namespace {

constexpr int kH = 4;                      // heads
constexpr int kD = 8;                      // channels per head
constexpr int kG = 16;                     // slices
constexpr int kC = kH * kD;                // 32 channels
constexpr int kPts = kBlock;               // points per workgroup: one per thread
constexpr int kE = kG * (kD + 1);          // 144 accumulators of a head: [g][c], c = kD the norm
constexpr int kLd = kPts + 1;              // LDS row stride of the outer reduction
constexpr int kWoE = kC * kC + kC;         // d Wo and d bo of a workgroup
constexpr int kWsE = kE + kH;              // d Ws, d bs ([g][c], c = kD the bias) and d temperature
constexpr int kQkvE = 3 * kD * kD;
constexpr int kLdP = kC + 2;               // row stride of the d Wo tiles (even: 8-B aligned pairs)
constexpr int kSeg = 16;                   // segments of the ordered partial sum
constexpr float kNormEps = 1e-5f;
// the token kernels give thread tid entry tid of the 16 x 16 attention matrix, unguarded
static_assert(kBlock == kG * kG, "token_fwd_kernel / token_bwd_kernel index a[tid], tid < kBlock");

__device__ __forceinline__ float clamp_t(float t) { return fminf(fmaxf(t, 0.1f), 5.0f); }

// acc[g * 9 + c] = sum_p a[p][g] * (c < 8 ? b[p][c] : 1) over the workgroup's points, p in order
__device__ __forceinline__ float outer_reduce(float* __restrict__ sa, float* __restrict__ sb,
                                              const float* a, const float* b, int tid) {
  __syncthreads();
#pragma unroll
  for (int g = 0; g < kG; ++g) sa[g * kLd + tid] = a[g];
#pragma unroll
  for (int c = 0; c < kD; ++c) sb[c * kLd + tid] = b[c];
  __syncthreads();
  float acc = 0.f;
  if (tid < kE) {
    const int g = tid / (kD + 1), c = tid - g * (kD + 1);
    const float* pa = sa + g * kLd;
    if (c < kD) {
      const float* pb = sb + c * kLd;
#pragma unroll 8
      for (int p = 0; p < kPts; ++p) acc = fmaf(pa[p], pb[p], acc);
    } else {
#pragma unroll 8
      for (int p = 0; p < kPts; ++p) acc += pa[p];
    }
  }
  return acc;
}

// slice logits of one point and head: (Ws x + bs) / T
__device__ __forceinline__ void slice_logits(const float* __restrict__ Ws,
                                             const float* __restrict__ bs, const float* x,
                                             float inv_t, float* z) {
#pragma unroll
  for (int g = 0; g < kG; ++g) {
    float acc = bs[g];
#pragma unroll
    for (int c = 0; c < kD; ++c) acc = fmaf(Ws[g * kD + c], x[c], acc);
    z[g] = acc * inv_t;
  }
}

// w (S, 4, G, N) and the workgroup's partials of norm and of the unnormalised tokens
__global__ __launch_bounds__(kBlock) void slice_kernel(
    const float* __restrict__ xm, const float* __restrict__ fm, int64_t sstride,
    const float* __restrict__ temperature, const float* __restrict__ Ws,
    const float* __restrict__ bs, float* __restrict__ w, float* __restrict__ part, int N,
    int nblk) {
  __shared__ float sa[kG * kLd];
  __shared__ float sb[kD * kLd];
  const int tid = threadIdx.x, blk = blockIdx.x, s = blockIdx.y;
  const int n = blk * kPts + tid;
  const bool valid = n < N;
  const float* xs = xm + (int64_t)s * sstride + n;
  const float* fs = fm + (int64_t)s * sstride + n;
#pragma unroll 1
  for (int h = 0; h < kH; ++h) {
    float x[kD], f[kD], z[kG];
#pragma unroll
    for (int c = 0; c < kD; ++c) {
      x[c] = valid ? xs[(int64_t)(h * kD + c) * N] : 0.f;
      f[c] = valid ? fs[(int64_t)(h * kD + c) * N] : 0.f;
    }
    slice_logits(Ws, bs, x, 1.0f / clamp_t(temperature[h]), z);
    float mx = z[0];
#pragma unroll
    for (int g = 1; g < kG; ++g) mx = fmaxf(mx, z[g]);
    float den = 0.f;
#pragma unroll
    for (int g = 0; g < kG; ++g) {
      z[g] = expf(z[g] - mx);
      den += z[g];
    }
    const float inv = valid ? 1.0f / den : 0.f;
    float* wo = w + ((int64_t)(s * kH + h) * kG) * N + n;
#pragma unroll
    for (int g = 0; g < kG; ++g) {
      z[g] *= inv;
      if (valid) wo[(int64_t)g * N] = z[g];
    }
    const float acc = outer_reduce(sa, sb, z, f, tid);
    if (tid < kE) part[((int64_t)(s * kH + h) * nblk + blk) * kE + tid] = acc;
  }
}

// per (s, h): tokens from the partials, q / k / v, the 16 x 16 softmax and A v
__global__ __launch_bounds__(kBlock) void token_fwd_kernel(
    const float* __restrict__ part, const float* __restrict__ Wq, const float* __restrict__ Wk,
    const float* __restrict__ Wv, float* __restrict__ tok, float* __restrict__ norm,
    float* __restrict__ A, float* __restrict__ otok, int nblk) {
  __shared__ float T[kE], tk[kG * kD], q[kG * kD], k[kG * kD], v[kG * kD], a[kG * kG];
  const int tid = threadIdx.x, sh = blockIdx.x;
  if (tid < kE) {
    float acc = 0.f;
    for (int b = 0; b < nblk; ++b) acc += part[((int64_t)sh * nblk + b) * kE + tid];
    T[tid] = acc;
  }
  __syncthreads();
  if (tid < kG * kD) {
    const int g = tid / kD, c = tid - g * kD;
    const float t = T[g * (kD + 1) + c] / (T[g * (kD + 1) + kD] + kNormEps);
    tk[tid] = t;
    tok[(int64_t)sh * kG * kD + tid] = t;
  }
  if (tid < kG) norm[sh * kG + tid] = T[tid * (kD + 1) + kD];
  __syncthreads();
  if (tid < kG * kD) {
    const int g = tid / kD, j = tid - g * kD;
    float aq = 0.f, ak = 0.f, av = 0.f;
#pragma unroll
    for (int c = 0; c < kD; ++c) {
      const float t = tk[g * kD + c];
      aq = fmaf(t, Wq[j * kD + c], aq);
      ak = fmaf(t, Wk[j * kD + c], ak);
      av = fmaf(t, Wv[j * kD + c], av);
    }
    q[tid] = aq;
    k[tid] = ak;
    v[tid] = av;
  }
  __syncthreads();
  {
    const int i = tid / kG, j = tid - i * kG;
    float acc = 0.f;
#pragma unroll
    for (int c = 0; c < kD; ++c) acc = fmaf(q[i * kD + c], k[j * kD + c], acc);
    a[tid] = acc * 0.35355339059327376f;       // D^-1/2
  }
  __syncthreads();
  if (tid < kG) {
    float mx = a[tid * kG];
    for (int j = 1; j < kG; ++j) mx = fmaxf(mx, a[tid * kG + j]);
    float den = 0.f;
    for (int j = 0; j < kG; ++j) {
      const float e = expf(a[tid * kG + j] - mx);
      a[tid * kG + j] = e;
      den += e;
    }
    const float inv = 1.0f / den;
    for (int j = 0; j < kG; ++j) a[tid * kG + j] *= inv;
  }
  __syncthreads();
  A[(int64_t)sh * kG * kG + tid] = a[tid];
  if (tid < kG * kD) {
    const int g = tid / kD, c = tid - g * kD;
    float acc = 0.f;
#pragma unroll
    for (int j = 0; j < kG; ++j) acc = fmaf(a[g * kG + j], v[j * kD + c], acc);
    otok[(int64_t)sh * kG * kD + tid] = acc;
  }
}

// ox of one point from w and otok (uniform loads of otok)
__device__ __forceinline__ void deslice_point(const float* __restrict__ w,
                                              const float* __restrict__ otok, int s, int n, int N,
                                              bool valid, float* ox) {
#pragma unroll
  for (int h = 0; h < kH; ++h) {
    const float* wp = w + ((int64_t)(s * kH + h) * kG) * N + n;
    const float* ot = otok + (int64_t)(s * kH + h) * kG * kD;
#pragma unroll
    for (int c = 0; c < kD; ++c) ox[h * kD + c] = 0.f;
#pragma unroll
    for (int g = 0; g < kG; ++g) {
      const float wv = valid ? wp[(int64_t)g * N] : 0.f;
#pragma unroll
      for (int c = 0; c < kD; ++c) ox[h * kD + c] = fmaf(wv, ot[g * kD + c], ox[h * kD + c]);
    }
  }
}

// y = to_out(ox) (+ res), ox formed per point and never stored
__global__ __launch_bounds__(kBlock) void deslice_kernel(
    const float* __restrict__ w, const float* __restrict__ otok, const float* __restrict__ Wo,
    const float* __restrict__ bo, const float* __restrict__ res, float* __restrict__ y, int N) {
  const int s = blockIdx.y, n = blockIdx.x * kPts + threadIdx.x;
  if (n >= N) return;
  float ox[kC];
  deslice_point(w, otok, s, n, N, true, ox);
  const int64_t base = (int64_t)s * kC * N + n;
#pragma unroll
  for (int o = 0; o < kC; ++o) {
    float acc = bo[o];
#pragma unroll
    for (int i = 0; i < kC; ++i) acc = fmaf(Wo[o * kC + i], ox[i], acc);
    if (res) acc += res[base + (int64_t)o * N];
    y[base + (int64_t)o * N] = acc;
  }
}

// First point pass of the backward: dox = dy Wo (kept for the second pass), the partials of
// d otok, and the workgroup's d Wo = dy^T ox and d bo.
__global__ __launch_bounds__(kBlock) void bwd_point1_kernel(
    const float* __restrict__ dy, const float* __restrict__ w, const float* __restrict__ otok,
    const float* __restrict__ Wo, float* __restrict__ dox, float* __restrict__ dpart,
    float* __restrict__ wopart, int N, int nblk) {
  // 69.6 KB of static LDS: above the 64 KB of older parts, within gfx950's 160 KB per workgroup
  __shared__ __attribute__((aligned(16))) float lds[2 * kPts * kLdP];
  float* sa = lds;
  float* sb = lds + kG * kLd;
  const int tid = threadIdx.x, blk = blockIdx.x, s = blockIdx.y;
  const int n = blk * kPts + tid;
  const bool valid = n < N;
  const int64_t base = (int64_t)s * kC * N + n;
  float g_[kC], d[kC], ox[kC];
#pragma unroll
  for (int o = 0; o < kC; ++o) g_[o] = valid ? dy[base + (int64_t)o * N] : 0.f;
#pragma unroll
  for (int i = 0; i < kC; ++i) {
    float acc = 0.f;
#pragma unroll
    for (int o = 0; o < kC; ++o) acc = fmaf(g_[o], Wo[o * kC + i], acc);
    d[i] = acc;
    if (valid) dox[base + (int64_t)i * N] = acc;
  }
  deslice_point(w, otok, s, n, N, valid, ox);
#pragma unroll
  for (int h = 0; h < kH; ++h) {
    float wv[kG];
    const float* wp = w + ((int64_t)(s * kH + h) * kG) * N + n;
#pragma unroll
    for (int g = 0; g < kG; ++g) wv[g] = valid ? wp[(int64_t)g * N] : 0.f;
    const float acc = outer_reduce(sa, sb, wv, &d[h * kD], tid);
    if (tid < kE) dpart[((int64_t)(s * kH + h) * nblk + blk) * kE + tid] = acc;
  }
  __syncthreads();
  float* dyl = lds;
  float* oxl = lds + kPts * kLdP;
#pragma unroll
  for (int o = 0; o < kC; ++o) {
    dyl[tid * kLdP + o] = g_[o];
    oxl[tid * kLdP + o] = ox[o];
  }
  __syncthreads();
  const int to = (tid >> 4) * 2, ti = (tid & 15) * 2;
  float a00 = 0.f, a01 = 0.f, a10 = 0.f, a11 = 0.f;
#pragma unroll 4
  for (int p = 0; p < kPts; ++p) {
    const float2 a = *reinterpret_cast<const float2*>(dyl + p * kLdP + to);
    const float2 b = *reinterpret_cast<const float2*>(oxl + p * kLdP + ti);
    a00 = fmaf(a.x, b.x, a00);
    a01 = fmaf(a.x, b.y, a01);
    a10 = fmaf(a.y, b.x, a10);
    a11 = fmaf(a.y, b.y, a11);
  }
  float* wp = wopart + ((int64_t)s * nblk + blk) * kWoE;
  wp[to * kC + ti] = a00;
  wp[to * kC + ti + 1] = a01;
  wp[(to + 1) * kC + ti] = a10;
  wp[(to + 1) * kC + ti + 1] = a11;
  if (tid < kC) {
    float acc = 0.f;
    for (int p = 0; p < kPts; ++p) acc += dyl[p * kLdP + tid];
    wp[kC * kC + tid] = acc;
  }
}

// per (s, h): the backward of the token attention.  dtoks = d tok / (norm + eps), cterm =
// -sum_c tok d tok / (norm + eps) (what the second point pass needs), and this (s, h)'s d Wq / d Wk
// / d Wv.
__global__ __launch_bounds__(kBlock) void token_bwd_kernel(
    const float* __restrict__ dpart, const float* __restrict__ tok, const float* __restrict__ norm,
    const float* __restrict__ A, const float* __restrict__ Wq, const float* __restrict__ Wk,
    const float* __restrict__ Wv, float* __restrict__ dtoks, float* __restrict__ cterm,
    float* __restrict__ qkvpart, int nblk) {
  __shared__ float dot[kG * kD], tk[kG * kD], q[kG * kD], k[kG * kD], v[kG * kD], a[kG * kG],
      ds[kG * kG], dq[kG * kD], dk[kG * kD], dv[kG * kD], dt[kG * kD];
  const int tid = threadIdx.x, sh = blockIdx.x;
  if (tid < kE) {
    const int g = tid / (kD + 1), c = tid - g * (kD + 1);
    float acc = 0.f;
    for (int b = 0; b < nblk; ++b) acc += dpart[((int64_t)sh * nblk + b) * kE + tid];
    if (c < kD) dot[g * kD + c] = acc;
  }
  a[tid] = A[(int64_t)sh * kG * kG + tid];
  if (tid < kG * kD) tk[tid] = tok[(int64_t)sh * kG * kD + tid];
  __syncthreads();
  if (tid < kG * kD) {
    const int g = tid / kD, j = tid - g * kD;
    float aq = 0.f, ak = 0.f, av = 0.f;
#pragma unroll
    for (int c = 0; c < kD; ++c) {
      const float t = tk[g * kD + c];
      aq = fmaf(t, Wq[j * kD + c], aq);
      ak = fmaf(t, Wk[j * kD + c], ak);
      av = fmaf(t, Wv[j * kD + c], av);
    }
    q[tid] = aq;
    k[tid] = ak;
    v[tid] = av;
  }
  __syncthreads();
  {
    const int g = tid / kG, j = tid - g * kG;       // dA[g][j]
    float acc = 0.f;
#pragma unroll
    for (int c = 0; c < kD; ++c) acc = fmaf(dot[g * kD + c], v[j * kD + c], acc);
    ds[tid] = acc;
  }
  if (tid < kG * kD) {
    const int j = tid / kD, c = tid - j * kD;       // dv[j][c] = sum_g A[g][j] dotok[g][c]
    float acc = 0.f;
#pragma unroll
    for (int g = 0; g < kG; ++g) acc = fmaf(a[g * kG + j], dot[g * kD + c], acc);
    dv[tid] = acc;
  }
  __syncthreads();
  float rs = 0.f;
  {
    const int g = tid / kG;
#pragma unroll
    for (int j = 0; j < kG; ++j) rs = fmaf(a[g * kG + j], ds[g * kG + j], rs);
  }
  __syncthreads();
  ds[tid] = a[tid] * (ds[tid] - rs) * 0.35355339059327376f;
  __syncthreads();
  if (tid < kG * kD) {
    const int g = tid / kD, c = tid - g * kD;
    float aq = 0.f, ak = 0.f;
#pragma unroll
    for (int j = 0; j < kG; ++j) {
      aq = fmaf(ds[g * kG + j], k[j * kD + c], aq);     // dq[g][c]
      ak = fmaf(ds[j * kG + g], q[j * kD + c], ak);     // dk[g][c] = sum_j dS[j][g] q[j][c]
    }
    dq[tid] = aq;
    dk[tid] = ak;
  }
  __syncthreads();
  if (tid < kG * kD) {
    const int g = tid / kD, c = tid - g * kD;
    float acc = 0.f;
#pragma unroll
    for (int j = 0; j < kD; ++j) {
      acc = fmaf(dq[g * kD + j], Wq[j * kD + c], acc);
      acc = fmaf(dk[g * kD + j], Wk[j * kD + c], acc);
      acc = fmaf(dv[g * kD + j], Wv[j * kD + c], acc);
    }
    dt[tid] = acc;
    dtoks[(int64_t)sh * kG * kD + tid] = acc / (norm[sh * kG + g] + kNormEps);
  }
  if (tid >= kG * kD && tid < kG * kD + kQkvE / 3) {
    // d W[j][c] = sum_g d(q|k|v)[g][j] tok[g][c]
    const int e = tid - kG * kD, j = e / kD, c = e - j * kD;
    float aq = 0.f, ak = 0.f, av = 0.f;
#pragma unroll
    for (int g = 0; g < kG; ++g) {
      const float t = tk[g * kD + c];
      aq = fmaf(dq[g * kD + j], t, aq);
      ak = fmaf(dk[g * kD + j], t, ak);
      av = fmaf(dv[g * kD + j], t, av);
    }
    float* qp = qkvpart + (int64_t)sh * kQkvE;
    qp[e] = aq;
    qp[kD * kD + e] = ak;
    qp[2 * kD * kD + e] = av;
  }
  __syncthreads();
  if (tid < kG) {
    float acc = 0.f;
#pragma unroll
    for (int c = 0; c < kD; ++c) acc = fmaf(tk[tid * kD + c], dt[tid * kD + c], acc);
    cterm[sh * kG + tid] = -acc / (norm[sh * kG + tid] + kNormEps);
  }
}

// Second point pass: d w, the slice softmax backward, d fm, d xm and the workgroup's partials of
// d Ws, d bs (summed over the heads, which share them) and d temperature.
__global__ __launch_bounds__(kBlock) void bwd_point2_kernel(
    const float* __restrict__ xm, const float* __restrict__ fm, int64_t sstride,
    const float* __restrict__ temperature, const float* __restrict__ Ws,
    const float* __restrict__ bs, const float* __restrict__ w, const float* __restrict__ otok,
    const float* __restrict__ dox, const float* __restrict__ dtoks,
    const float* __restrict__ cterm, float* __restrict__ dxm, float* __restrict__ dfm,
    int64_t dstride, float* __restrict__ wspart, int N, int nblk) {
  __shared__ float sa[kG * kLd];
  __shared__ float sb[kD * kLd];
  __shared__ float sw[kBlock / 64];
  const int tid = threadIdx.x, blk = blockIdx.x, s = blockIdx.y;
  const int n = blk * kPts + tid;
  const bool valid = n < N;
  const float* xs = xm + (int64_t)s * sstride + n;
  const float* fs = fm + (int64_t)s * sstride + n;
  float* wp = wspart + ((int64_t)s * nblk + blk) * kWsE;
  float wsacc = 0.f;
#pragma unroll 1
  for (int h = 0; h < kH; ++h) {
    const int sh = s * kH + h;
    const float traw = temperature[h];
    const float inv_t = 1.0f / clamp_t(traw);
    const float* ot = otok + (int64_t)sh * kG * kD;
    const float* dtk = dtoks + (int64_t)sh * kG * kD;
    float x[kD], f[kD], d[kD], wv[kG], z[kG];
#pragma unroll
    for (int c = 0; c < kD; ++c) {
      x[c] = valid ? xs[(int64_t)(h * kD + c) * N] : 0.f;
      f[c] = valid ? fs[(int64_t)(h * kD + c) * N] : 0.f;
      d[c] = valid ? dox[((int64_t)s * kC + h * kD + c) * N + n] : 0.f;
    }
    const float* wg = w + ((int64_t)sh * kG) * N + n;
#pragma unroll
    for (int g = 0; g < kG; ++g) wv[g] = valid ? wg[(int64_t)g * N] : 0.f;
    float sdot = 0.f;
#pragma unroll
    for (int g = 0; g < kG; ++g) {
      float acc = cterm[sh * kG + g];
#pragma unroll
      for (int c = 0; c < kD; ++c) {
        acc = fmaf(ot[g * kD + c], d[c], acc);
        acc = fmaf(dtk[g * kD + c], f[c], acc);
      }
      z[g] = acc;                                   // d w[g]
      sdot = fmaf(wv[g], acc, sdot);
    }
#pragma unroll
    for (int c = 0; c < kD; ++c) {
      float acc = 0.f;
#pragma unroll
      for (int g = 0; g < kG; ++g) acc = fmaf(wv[g], dtk[g * kD + c], acc);
      if (valid) dfm[(int64_t)s * dstride + (int64_t)(h * kD + c) * N + n] = acc;
    }
#pragma unroll
    for (int g = 0; g < kG; ++g) wv[g] *= z[g] - sdot;      // d logit[g] (of the scaled logits)
    slice_logits(Ws, bs, x, inv_t, z);
    // sum_g dlogit[g] = 0, so the logits enter d T centred on their maximum: the dominant slice
    // then contributes nothing and the products that cancel are small
    float mx = z[0];
#pragma unroll
    for (int g = 1; g < kG; ++g) mx = fmaxf(mx, z[g]);
    float tsum = 0.f;
#pragma unroll
    for (int g = 0; g < kG; ++g) {
      tsum = fmaf(wv[g], z[g] - mx, tsum);
      wv[g] *= inv_t;                                        // d (Ws x + bs)[g]
    }
#pragma unroll
    for (int c = 0; c < kD; ++c) {
      float acc = 0.f;
#pragma unroll
      for (int g = 0; g < kG; ++g) acc = fmaf(wv[g], Ws[g * kD + c], acc);
      if (valid) dxm[(int64_t)s * dstride + (int64_t)(h * kD + c) * N + n] = acc;
    }
    wsacc += outer_reduce(sa, sb, wv, x, tid);
    // d clamp(T) = -sum dlogit z / T; the clamp passes it where 0.1 <= T <= 5
    const float pass = (traw >= 0.1f && traw <= 5.0f) ? -inv_t : 0.f;
    const float ts = wave_sum(tsum);
    if ((tid & 63) == 0) sw[tid >> 6] = ts;
    __syncthreads();
    if (tid == 0) {
      float acc = sw[0];
      for (int k = 1; k < kBlock / 64; ++k) acc += sw[k];
      wp[kE + h] = acc * pass;
    }
  }
  if (tid < kE) wp[tid] = wsacc;
}

// sum of rows [0, n) of one column of a partial table: kSeg contiguous row ranges, each summed in
// row order by one thread, then added in segment order
__device__ __forceinline__ float seg_reduce(float* __restrict__ sl, const float* __restrict__ src,
                                            int64_t stride, int n, int el, int seg, bool live) {
  const int per = (n + kSeg - 1) / kSeg;
  const int r0 = seg * per, r1 = min(n, r0 + per);
  float acc = 0.f;
  if (live) {
#pragma unroll 8
    for (int r = r0; r < r1; ++r) acc += src[(int64_t)r * stride];
  }
  sl[seg * kSeg + el] = acc;
  __syncthreads();
  float tot = 0.f;
  if (seg == 0)
    for (int k = 0; k < kSeg; ++k) tot += sl[k * kSeg + el];
  return tot;
}

struct FinArgs {
  const float* wopart;
  const float* wspart;
  const float* qkvpart;
  int nA, nB;
  float *dWo, *dbo, *dWs, *dbs, *dtemp, *dWq, *dWk, *dWv;
};

__global__ __launch_bounds__(kBlock) void finish_kernel(FinArgs a) {
  __shared__ float sl[kSeg * kSeg];
  const int el = threadIdx.x & (kSeg - 1), seg = threadIdx.x / kSeg;
  const int e = blockIdx.x * kSeg + el;
  const float* src = nullptr;
  float* dst = nullptr;
  int64_t stride = 0;
  int n = 0;
  if (e < kWoE) {
    src = a.wopart + e, stride = kWoE, n = a.nA;
    dst = e < kC * kC ? a.dWo + e : a.dbo + (e - kC * kC);
  } else if (e < kWoE + kWsE) {
    const int k = e - kWoE;
    src = a.wspart + k, stride = kWsE, n = a.nA;
    if (k < kE) {
      const int g = k / (kD + 1), c = k - g * (kD + 1);
      dst = c < kD ? a.dWs + g * kD + c : a.dbs + g;
    } else {
      dst = a.dtemp + (k - kE);
    }
  } else if (e < kWoE + kWsE + kQkvE) {
    const int k = e - kWoE - kWsE;
    src = a.qkvpart + k, stride = kQkvE, n = a.nB;
    dst = k < kD * kD ? a.dWq + k : (k < 2 * kD * kD ? a.dWk + (k - kD * kD) : a.dWv + (k - 2 * kD * kD));
  }
  const float tot = seg_reduce(sl, src, stride, n, el, seg, dst != nullptr);
  if (seg == 0 && dst) *dst = tot;
}

// ------------------------------------------------------------------ LayerNorm over the planes

__global__ __launch_bounds__(kBlock) void ln_fwd_kernel(const float* __restrict__ x,
                                                        const float* __restrict__ gamma,
                                                        const float* __restrict__ beta,
                                                        float* __restrict__ y,
                                                        float* __restrict__ mean,
                                                        float* __restrict__ rstd, int N, float eps) {
  const int s = blockIdx.y, n = blockIdx.x * kPts + threadIdx.x;
  if (n >= N) return;
  const int64_t base = (int64_t)s * kC * N + n;
  float v[kC];
  float m = 0.f;
#pragma unroll
  for (int c = 0; c < kC; ++c) {
    v[c] = x[base + (int64_t)c * N];
    m += v[c];
  }
  m *= 1.0f / kC;
  float var = 0.f;
#pragma unroll
  for (int c = 0; c < kC; ++c) {
    v[c] -= m;
    var = fmaf(v[c], v[c], var);
  }
  const float r = 1.0f / sqrtf(var * (1.0f / kC) + eps);
  mean[(int64_t)s * N + n] = m;
  rstd[(int64_t)s * N + n] = r;
#pragma unroll
  for (int c = 0; c < kC; ++c) y[base + (int64_t)c * N] = fmaf(v[c] * r, gamma[c], beta[c]);
}

__global__ __launch_bounds__(kBlock) void ln_bwd_kernel(
    const float* __restrict__ dy, const float* __restrict__ x, const float* __restrict__ gamma,
    const float* __restrict__ mean, const float* __restrict__ rstd, float* __restrict__ dx,
    float* __restrict__ part, int N, int nblk) {
  __shared__ float sw[(kBlock / 64) * 2 * kC];
  const int tid = threadIdx.x, blk = blockIdx.x, s = blockIdx.y;
  const int n = blk * kPts + tid;
  const bool valid = n < N;
  const int64_t base = (int64_t)s * kC * N + n;
  const float m = valid ? mean[(int64_t)s * N + n] : 0.f;
  const float r = valid ? rstd[(int64_t)s * N + n] : 0.f;
  float xh[kC], g[kC];
  float s1 = 0.f, s2 = 0.f;
#pragma unroll
  for (int c = 0; c < kC; ++c) {
    xh[c] = valid ? (x[base + (int64_t)c * N] - m) * r : 0.f;
    g[c] = valid ? dy[base + (int64_t)c * N] : 0.f;
    const float gh = g[c] * gamma[c];
    s1 += gh;
    s2 = fmaf(gh, xh[c], s2);
  }
  s1 *= 1.0f / kC;
  s2 *= 1.0f / kC;
  const int lane = tid & 63, wave = tid >> 6;
#pragma unroll
  for (int c = 0; c < kC; ++c) {
    if (valid) dx[base + (int64_t)c * N] = r * (g[c] * gamma[c] - s1 - xh[c] * s2);
    const float a = wave_sum(g[c] * xh[c]);
    const float b = wave_sum(g[c]);
    if (lane == 0) {
      sw[wave * 2 * kC + c] = a;
      sw[wave * 2 * kC + kC + c] = b;
    }
  }
  __syncthreads();
  if (tid < 2 * kC) {
    float acc = sw[tid];
    for (int k = 1; k < kBlock / 64; ++k) acc += sw[k * 2 * kC + tid];
    part[((int64_t)s * nblk + blk) * 2 * kC + tid] = acc;
  }
}

__global__ __launch_bounds__(kBlock) void ln_finish_kernel(const float* __restrict__ part,
                                                           float* __restrict__ dgamma,
                                                           float* __restrict__ dbeta, int n) {
  __shared__ float sl[kSeg * kSeg];
  const int el = threadIdx.x & (kSeg - 1), seg = threadIdx.x / kSeg;
  const int e = blockIdx.x * kSeg + el;      // < 2 kC: the grid is 2 kC / kSeg workgroups
  const float tot = seg_reduce(sl, part + e, 2 * kC, n, el, seg, true);
  if (seg == 0) {
    if (e < kC) dgamma[e] = tot;
    else dbeta[e - kC] = tot;
  }
}

bool shape_ok(int S, int H, int W) {
  return S >= 1 && H >= 1 && W >= 1 && (int64_t)H * W <= (1 << 24) && S <= 65535 &&
         (int64_t)S * kH * kG * H * W < ((int64_t)1 << 40);
}

}  // namespace

BLINDNO_API int blindno_physattn_ok(int S, int H, int W, int heads, int D, int G) {
  return (shape_ok(S, H, W) && heads == kH && D == kD && G == kG) ? 1 : 0;
}

BLINDNO_API int blindno_physattn_nblk(int H, int W) {
  return (H < 1 || W < 1 || (int64_t)H * W > (1 << 24)) ? -1 : cdiv((int64_t)H * W, kPts);
}

BLINDNO_API int64_t blindno_physattn_fwd_scratch_floats(int S, int H, int W) {
  if (!shape_ok(S, H, W)) return -1;
  return (int64_t)S * kH * cdiv((int64_t)H * W, kPts) * kE;
}

BLINDNO_API int blindno_physattn_fwd(const float* xm, const float* fm, int64_t sstride,
                                     const float* temperature, const float* Ws, const float* bs,
                                     const float* Wq, const float* Wk, const float* Wv,
                                     const float* Wo, const float* bo, const float* res, float* w,
                                     float* tok, float* norm, float* A, float* otok,
                                     float* scratch, float* y, int S, int H, int W,
                                     void* stream) {
  const int64_t N64 = (int64_t)H * W;
  if (!shape_ok(S, H, W) || sstride < kC * N64 || !xm || !fm || !temperature || !Ws || !bs ||
      !Wq || !Wk || !Wv || !Wo || !bo || !w || !tok || !norm || !A || !otok || !scratch || !y)
    return (int)hipErrorInvalidValue;
  const int N = (int)N64, nblk = cdiv(N, kPts);
  hipStream_t st = (hipStream_t)stream;
  slice_kernel<<<dim3(nblk, S), kBlock, 0, st>>>(xm, fm, sstride, temperature, Ws, bs, w, scratch,
                                                N, nblk);
  token_fwd_kernel<<<S * kH, kBlock, 0, st>>>(scratch, Wq, Wk, Wv, tok, norm, A, otok, nblk);
  deslice_kernel<<<dim3(nblk, S), kBlock, 0, st>>>(w, otok, Wo, bo, res, y, N);
  return (int)hipGetLastError();
}

BLINDNO_API int64_t blindno_physattn_bwd_scratch_floats(int S, int H, int W) {
  if (!shape_ok(S, H, W)) return -1;
  const int64_t N = (int64_t)H * W, nblk = cdiv(N, kPts);
  return (int64_t)S * kC * N + (int64_t)S * kH * nblk * kE + (int64_t)S * nblk * kWoE +
         (int64_t)S * kH * (kG * kD + kG + kQkvE) + (int64_t)S * nblk * kWsE;
}

BLINDNO_API int blindno_physattn_bwd(
    const float* dy, const float* xm, const float* fm, int64_t sstride, const float* temperature,
    const float* Ws, const float* bs, const float* Wq, const float* Wk, const float* Wv,
    const float* Wo, const float* w, const float* tok, const float* norm, const float* A,
    const float* otok, float* scratch, float* dxm, float* dfm, int64_t dstride,
    float* dtemperature, float* dWs, float* dbs, float* dWq, float* dWk, float* dWv, float* dWo,
    float* dbo, int S, int H, int W, void* stream) {
  const int64_t N64 = (int64_t)H * W;
  if (!shape_ok(S, H, W) || sstride < kC * N64 || dstride < kC * N64 || !dy || !xm || !fm ||
      !temperature || !Ws || !bs || !Wq || !Wk || !Wv || !Wo || !w || !tok || !norm || !A ||
      !otok || !scratch || !dxm || !dfm || !dtemperature || !dWs || !dbs || !dWq || !dWk ||
      !dWv || !dWo || !dbo)
    return (int)hipErrorInvalidValue;
  const int N = (int)N64, nblk = cdiv(N, kPts);
  float* dox = scratch;                                        // (S, 32, N)
  float* dpart = dox + (int64_t)S * kC * N;                    // (S 4, nblk, 144)
  float* wopart = dpart + (int64_t)S * kH * nblk * kE;         // (S nblk, 1056)
  float* dtoks = wopart + (int64_t)S * nblk * kWoE;            // (S 4, 16, 8)
  float* cterm = dtoks + (int64_t)S * kH * kG * kD;            // (S 4, 16)
  float* qkvpart = cterm + (int64_t)S * kH * kG;               // (S 4, 192)
  float* wspart = qkvpart + (int64_t)S * kH * kQkvE;           // (S nblk, 148)
  hipStream_t st = (hipStream_t)stream;
  bwd_point1_kernel<<<dim3(nblk, S), kBlock, 0, st>>>(dy, w, otok, Wo, dox, dpart, wopart, N, nblk);
  token_bwd_kernel<<<S * kH, kBlock, 0, st>>>(dpart, tok, norm, A, Wq, Wk, Wv, dtoks, cterm,
                                              qkvpart, nblk);
  bwd_point2_kernel<<<dim3(nblk, S), kBlock, 0, st>>>(xm, fm, sstride, temperature, Ws, bs, w, otok,
                                                     dox, dtoks, cterm, dxm, dfm, dstride, wspart,
                                                     N, nblk);
  FinArgs fa{wopart, wspart, qkvpart, S * nblk, S * kH, dWo, dbo, dWs, dbs, dtemperature,
             dWq,    dWk,    dWv};
  finish_kernel<<<cdiv(kWoE + kWsE + kQkvE, kSeg), kBlock, 0, st>>>(fa);
  return (int)hipGetLastError();
}

BLINDNO_API int blindno_ln_planes_nblk(int HW) {
  return (HW < 1 || HW > (1 << 24)) ? -1 : cdiv(HW, kPts);
}

BLINDNO_API int blindno_ln_planes_fwd(const float* x, const float* gamma, const float* beta,
                                      float* y, float* mean, float* rstd, int S, int C, int HW,
                                      float eps, void* stream) {
  if (S < 1 || S > 65535 || C != kC || HW < 1 || HW > (1 << 24) || !x || !gamma || !beta || !y ||
      !mean || !rstd)
    return (int)hipErrorInvalidValue;
  ln_fwd_kernel<<<dim3(cdiv(HW, kPts), S), kBlock, 0, (hipStream_t)stream>>>(x, gamma, beta, y, mean,
                                                                            rstd, HW, eps);
  return (int)hipGetLastError();
}

BLINDNO_API int blindno_ln_planes_bwd(const float* dy, const float* x, const float* gamma,
                                      const float* mean, const float* rstd, float* dx,
                                      float* dgamma, float* dbeta, float* partial, int S, int C,
                                      int HW, void* stream) {
  if (S < 1 || S > 65535 || C != kC || HW < 1 || HW > (1 << 24) || !dy || !x || !gamma || !mean ||
      !rstd || !dx || !dgamma || !dbeta || !partial)
    return (int)hipErrorInvalidValue;
  const int nblk = cdiv(HW, kPts);
  hipStream_t st = (hipStream_t)stream;
  ln_bwd_kernel<<<dim3(nblk, S), kBlock, 0, st>>>(dy, x, gamma, mean, rstd, dx, partial, HW, nblk);
  ln_finish_kernel<<<2 * kC / kSeg, kBlock, 0, st>>>(partial, dgamma, dbeta, S * nblk);
  return (int)hipGetLastError();
}
