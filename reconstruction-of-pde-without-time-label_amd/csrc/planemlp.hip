// The fused per-point MLP over channel planes (S, C, N): LayerNorm (optional), Linear, GELU,
// Linear and the residual in one thread per point, forward and backward, for the token MLPs of
// the structured-mesh Transolver.  include/blindno_planemlp.h has the formulas.
//
// A thread owns a point: a channel is one coalesced load per plane.  The weights are read at
// wave-uniform, compile-time offsets (every channel loop is fully unrolled), so they arrive as
// scalar loads and enter the FMAs as scalar operands; no weight sits in a vector register.  The
// forward holds the input and the hidden vector (Cin + Chid values) and forms one output channel
// at a time.  The backward walks the hidden layer in chunks of 32 and recomputes it.
//
// Weight gradients: per chunk the workgroup puts two 32-wide rows per point into LDS tiles
// (dy and gelu(z); dz and u) and thread (a, b) sums a 2 x 2 block of their outer product over the
// 256 points in index order; the column sums of the first tile are the bias gradients.  Each
// workgroup writes one row of partials, a second launch adds the rows in index order.  No atomics.
#include "common.h"
#include "blindno.h"

using namespace blindno;

namespace {

constexpr int kPts = kBlock;               // points per workgroup: one per thread
constexpr int kHC = 32;                    // hidden channels per backward chunk = tile width
constexpr int kLdT = kHC + 2;              // tile row stride (even: 8-B aligned pairs)
constexpr int kSeg = 16;                   // segments of the ordered partial sum
constexpr int kParts = kPts / 32;          // row groups of the column sum

__host__ __device__ constexpr int partial_floats(int cin, int chid, int cout) {
  return chid * cin + chid + cout * chid + cout + 2 * cin;
}

// GELU in the exact erf form and its derivative, through the device library's erff / expf (a few
// ulp).  common.h's gelu_f (|error| 4e-7) is not used here: this MLP sits inside every block of
// the Transolver, in front of gradients that cancel heavily (the token attention's to_q / to_k),
// which magnify an absolute error of that size past fp32 torch's own.
__device__ __forceinline__ void gelu_erf(float z, float& g, float& dg) {
  const float cdf = 0.5f * (1.0f + erff(z * 0.70710678118654752f));
  g = z * cdf;
  dg = fmaf(z, 0.39894228040143268f * expf(-0.5f * z * z), cdf);
}

__device__ __forceinline__ float gelu_erf(float z) {
  return 0.5f * z * (1.0f + erff(z * 0.70710678118654752f));
}

template <int CIN, bool LN>
__device__ __forceinline__ void normalise(float* v, const float* __restrict__ gamma,
                                          const float* __restrict__ beta, float eps, float& m,
                                          float& r) {
  if constexpr (LN) {
    m = 0.f;
#pragma unroll
    for (int c = 0; c < CIN; ++c) m += v[c];
    m *= 1.0f / CIN;
    float var = 0.f;
#pragma unroll
    for (int c = 0; c < CIN; ++c) {
      v[c] -= m;
      var = fmaf(v[c], v[c], var);
    }
    r = 1.0f / sqrtf(var * (1.0f / CIN) + eps);
#pragma unroll
    for (int c = 0; c < CIN; ++c) v[c] = fmaf(v[c] * r, gamma[c], beta[c]);
  }
}

template <int CIN, int CHID, int COUT, bool LN>
__global__ __launch_bounds__(kBlock) void mlp_fwd_kernel(
    const float* __restrict__ x, int64_t xstride, const float* __restrict__ gamma,
    const float* __restrict__ beta, const float* __restrict__ W1, const float* __restrict__ b1,
    const float* __restrict__ W2, const float* __restrict__ b2, const float* __restrict__ res,
    int64_t rstride, float* __restrict__ y, int64_t ystride, float* __restrict__ mean,
    float* __restrict__ rstd, int N, float eps) {
  const int s = blockIdx.y, n = blockIdx.x * kPts + threadIdx.x;
  if (n >= N) return;
  const float* xs = x + (int64_t)s * xstride + n;
  float u[CIN], h[CHID];
#pragma unroll
  for (int c = 0; c < CIN; ++c) u[c] = xs[(int64_t)c * N];
  float m = 0.f, r = 0.f;
  normalise<CIN, LN>(u, gamma, beta, eps, m, r);
  if constexpr (LN) {
    mean[(int64_t)s * N + n] = m;
    rstd[(int64_t)s * N + n] = r;
  }
#pragma unroll
  for (int j = 0; j < CHID; ++j) {
    float acc = b1[j];
#pragma unroll
    for (int i = 0; i < CIN; ++i) acc = fmaf(W1[j * CIN + i], u[i], acc);
    h[j] = gelu_erf(acc);
  }
  float* ys = y + (int64_t)s * ystride + n;
  const float* rs = res ? res + (int64_t)s * rstride + n : nullptr;
#pragma unroll
  for (int o = 0; o < COUT; ++o) {
    float acc = b2[o];
#pragma unroll
    for (int j = 0; j < CHID; ++j) acc = fmaf(W2[o * CHID + j], h[j], acc);
    if (rs) acc += rs[(int64_t)o * N];
    ys[(int64_t)o * N] = acc;
  }
}

// out[a ldo + b] = sum_p ta[p][a] tb[p][b] for a < 32, b < NB, and colsum[a] = sum_p ta[p][a]
// (where colsum is given), p in index order.  The tiles were written before the last barrier.
template <int NB>
__device__ __forceinline__ void outer_store(const float* __restrict__ ta,
                                            const float* __restrict__ tb, float* __restrict__ out,
                                            int ldo, float* __restrict__ colsum, int tid) {
  constexpr int BW = NB / 2;               // 2 x 2 blocks along b
  static_assert(NB % 2 == 0 && (kHC / 2) * BW <= kBlock, "a thread per 2 x 2 block");
  if (tid >= (kHC / 2) * BW) return;
  const int to = (tid / BW) * 2, ti = (tid % BW) * 2;
  float a00 = 0.f, a01 = 0.f, a10 = 0.f, a11 = 0.f, s0 = 0.f, s1 = 0.f;
#pragma unroll 4
  for (int p = 0; p < kPts; ++p) {
    const float2 a = *reinterpret_cast<const float2*>(ta + p * kLdT + to);
    const float2 b = *reinterpret_cast<const float2*>(tb + p * kLdT + ti);
    a00 = fmaf(a.x, b.x, a00);
    a01 = fmaf(a.x, b.y, a01);
    a10 = fmaf(a.y, b.x, a10);
    a11 = fmaf(a.y, b.y, a11);
    s0 += a.x;
    s1 += a.y;
  }
  out[to * ldo + ti] = a00;
  out[to * ldo + ti + 1] = a01;
  out[(to + 1) * ldo + ti] = a10;
  out[(to + 1) * ldo + ti + 1] = a11;
  if (colsum && ti == 0) {
    colsum[to] = s0;
    colsum[to + 1] = s1;
  }
}

// dx and one row of partials [dW1 | db1 | dW2 | db2 | dgamma | dbeta] per workgroup
template <int CIN, int CHID, int COUT, bool LN>
__global__ __launch_bounds__(kBlock) void mlp_bwd_kernel(
    const float* __restrict__ dy, int64_t dystride, const float* __restrict__ x, int64_t xstride,
    const float* __restrict__ gamma, const float* __restrict__ beta,
    const float* __restrict__ W1, const float* __restrict__ b1, const float* __restrict__ W2,
    const float* __restrict__ mean, const float* __restrict__ rstd, float* __restrict__ dx,
    int64_t dxstride, float* __restrict__ part, int N, int nblk) {
  static_assert(CHID % kHC == 0 && COUT == kHC && CIN <= kHC && (!LN || CIN == kHC),
                "tiles are 32 wide; the LayerNorm variant has 32 channels");
  constexpr int kE = partial_floats(CIN, CHID, COUT);
  constexpr int oW1 = 0, ob1 = CHID * CIN, oW2 = ob1 + CHID, ob2 = oW2 + COUT * CHID,
                oG = ob2 + COUT;
  // 69.6 KB of static LDS: above the 64 KB of older parts, within gfx950's 160 KB per workgroup
  __shared__ __attribute__((aligned(16))) float lds[2 * kPts * kLdT];
  __shared__ float red[2 * kParts * kHC];
  float* ta = lds;
  float* tb = lds + kPts * kLdT;
  const int tid = threadIdx.x, blk = blockIdx.x, s = blockIdx.y;
  const int n = blk * kPts + tid;
  const bool valid = n < N;
  const float* xs = x + (int64_t)s * xstride + n;
  const float* gs = dy + (int64_t)s * dystride + n;
  float* wp = part + ((int64_t)s * nblk + blk) * kE;

  // xh = (x - mean) rstd with LayerNorm (u = xh gamma + beta), else xh = u = x
  float xh[CIN], g[COUT], du[CIN];
  float r = 0.f;
  if constexpr (LN) {
    const float m = valid ? mean[(int64_t)s * N + n] : 0.f;
    r = valid ? rstd[(int64_t)s * N + n] : 0.f;
#pragma unroll
    for (int c = 0; c < CIN; ++c) xh[c] = valid ? (xs[(int64_t)c * N] - m) * r : 0.f;
  } else {
#pragma unroll
    for (int c = 0; c < CIN; ++c) xh[c] = valid ? xs[(int64_t)c * N] : 0.f;
  }
#pragma unroll
  for (int o = 0; o < COUT; ++o) g[o] = valid ? gs[(int64_t)o * N] : 0.f;
#pragma unroll
  for (int i = 0; i < CIN; ++i) du[i] = 0.f;

#pragma unroll
  for (int c0 = 0; c0 < CHID; c0 += kHC) {
    float z[kHC], dh[kHC];
    // z: the chunk's pre-activations, then gelu'(z); gelu(z) goes straight to its tile
#pragma unroll
    for (int j = 0; j < kHC; ++j) {
      float acc = b1[c0 + j];
#pragma unroll
      for (int i = 0; i < CIN; ++i) {
        const float ui = LN ? fmaf(xh[i], gamma[i], beta[i]) : xh[i];
        acc = fmaf(W1[(c0 + j) * CIN + i], ui, acc);
      }
      z[j] = acc;
    }
    __syncthreads();                       // the tiles' previous readers are done
#pragma unroll
    for (int j = 0; j < kHC; ++j) {
      float hv, gp;
      gelu_erf(z[j], hv, gp);
      z[j] = gp;
      tb[tid * kLdT + j] = hv;
    }
#pragma unroll
    for (int o = 0; o < COUT; ++o) ta[tid * kLdT + o] = g[o];
    __syncthreads();
    // dW2[:, chunk] = dy^T gelu(z), db2 = sum dy
    outer_store<kHC>(ta, tb, wp + oW2 + c0, CHID, c0 == 0 ? wp + ob2 : nullptr, tid);
    // dz = gelu'(z) * (W2[:, chunk]^T dy)
#pragma unroll
    for (int j = 0; j < kHC; ++j) dh[j] = 0.f;
#pragma unroll
    for (int o = 0; o < COUT; ++o) {
#pragma unroll
      for (int j = 0; j < kHC; ++j) dh[j] = fmaf(W2[o * CHID + c0 + j], g[o], dh[j]);
    }
#pragma unroll
    for (int j = 0; j < kHC; ++j) dh[j] *= z[j];
    __syncthreads();
#pragma unroll
    for (int j = 0; j < kHC; ++j) ta[tid * kLdT + j] = dh[j];
#pragma unroll
    for (int i = 0; i < CIN; ++i) tb[tid * kLdT + i] = LN ? fmaf(xh[i], gamma[i], beta[i]) : xh[i];
    __syncthreads();
    // dW1[chunk, :] = dz^T u, db1[chunk] = sum dz
    outer_store<CIN>(ta, tb, wp + oW1 + c0 * CIN, CIN, wp + ob1 + c0, tid);
#pragma unroll
    for (int j = 0; j < kHC; ++j) {
#pragma unroll
      for (int i = 0; i < CIN; ++i) du[i] = fmaf(W1[(c0 + j) * CIN + i], dh[j], du[i]);
    }
  }

  float* ds = dx + (int64_t)s * dxstride + n;
  if constexpr (LN) {
    // dgamma = sum du xh, dbeta = sum du: column sums of two tiles, 32 rows per thread, then the
    // 8 row groups in order
    __syncthreads();
#pragma unroll
    for (int i = 0; i < CIN; ++i) {
      ta[tid * kLdT + i] = du[i] * xh[i];
      tb[tid * kLdT + i] = du[i];
    }
    __syncthreads();
    {
      const int col = tid & (kHC - 1), grp = tid / kHC;
      float sa = 0.f, sb = 0.f;
#pragma unroll 8
      for (int k = 0; k < kPts / kParts; ++k) {
        sa += ta[(grp * (kPts / kParts) + k) * kLdT + col];
        sb += tb[(grp * (kPts / kParts) + k) * kLdT + col];
      }
      red[grp * kHC + col] = sa;
      red[(kParts + grp) * kHC + col] = sb;
    }
    float s1 = 0.f, s2 = 0.f;
#pragma unroll
    for (int i = 0; i < CIN; ++i) {
      du[i] *= gamma[i];
      s1 += du[i];
      s2 = fmaf(du[i], xh[i], s2);
    }
    s1 *= 1.0f / CIN;
    s2 *= 1.0f / CIN;
    if (valid) {
#pragma unroll
      for (int i = 0; i < CIN; ++i) ds[(int64_t)i * N] = r * (du[i] - s1 - xh[i] * s2);
    }
    __syncthreads();
    if (tid < 2 * kHC) {
      const int which = tid / kHC, col = tid & (kHC - 1);
      float acc = 0.f;
#pragma unroll
      for (int k = 0; k < kParts; ++k) acc += red[(which * kParts + k) * kHC + col];
      wp[oG + which * CIN + col] = acc;
    }
  } else {
    if (valid) {
#pragma unroll
      for (int i = 0; i < CIN; ++i) ds[(int64_t)i * N] = du[i];
    }
    if (tid < 2 * CIN) wp[oG + tid] = 0.f;   // the table has the columns; nothing reads them
  }
}

// sum of rows [0, n) of one column of the partial table: kSeg contiguous row ranges, each summed
// in row order by one thread, then added in segment order
struct FinArgs {
  const float* part;
  int n, E, eb1, eW2, eb2, eG, eB;          // column ranges: dW1 < eb1 <= db1 < eW2 <= ...
  float *dW1, *db1, *dW2, *db2, *dgamma, *dbeta;
};

__global__ __launch_bounds__(kBlock) void mlp_finish_kernel(FinArgs a) {
  __shared__ float sl[kSeg * kSeg];
  const int el = threadIdx.x & (kSeg - 1), seg = threadIdx.x / kSeg;
  const int e = blockIdx.x * kSeg + el;
  float* dst = nullptr;
  if (e < a.eb1) dst = a.dW1 + e;
  else if (e < a.eW2) dst = a.db1 + (e - a.eb1);
  else if (e < a.eb2) dst = a.dW2 + (e - a.eW2);
  else if (e < a.eG) dst = a.db2 + (e - a.eb2);
  else if (e < a.eB) dst = a.dgamma ? a.dgamma + (e - a.eG) : nullptr;
  else if (e < a.E) dst = a.dbeta ? a.dbeta + (e - a.eB) : nullptr;
  const int per = (a.n + kSeg - 1) / kSeg;
  const int r0 = seg * per, r1 = min(a.n, r0 + per);
  float acc = 0.f;
  if (dst) {
    const float* src = a.part + e;
#pragma unroll 8
    for (int r = r0; r < r1; ++r) acc += src[(int64_t)r * a.E];
  }
  sl[seg * kSeg + el] = acc;
  __syncthreads();
  if (seg == 0 && dst) {
    float tot = 0.f;
    for (int k = 0; k < kSeg; ++k) tot += sl[k * kSeg + el];
    *dst = tot;
  }
}

// 0: (32, 32, 32) with LayerNorm; 1: (4, 64, 32) without; -1: refused
int config_of(int Cin, int Chid, int Cout, bool has_ln) {
  if (Cin == 32 && Chid == 32 && Cout == 32 && has_ln) return 0;
  if (Cin == 4 && Chid == 64 && Cout == 32 && !has_ln) return 1;
  return -1;
}

bool shape_ok(int S, int N) { return S >= 1 && S <= 65535 && N >= 1 && N <= (1 << 24); }

}  // namespace

BLINDNO_API int blindno_plane_mlp_ok(int Cin, int Chid, int Cout, int has_ln) {
  return config_of(Cin, Chid, Cout, has_ln != 0) >= 0 ? 1 : 0;
}

BLINDNO_API int blindno_plane_mlp_nblk(int N) {
  return (N < 1 || N > (1 << 24)) ? -1 : cdiv(N, kPts);
}

BLINDNO_API int blindno_plane_mlp_fwd(const float* x, int64_t xstride, const float* gamma,
                                      const float* beta, const float* W1, const float* b1,
                                      const float* W2, const float* b2, const float* res,
                                      int64_t rstride, float* y, int64_t ystride, float* mean,
                                      float* rstd, int S, int N, int Cin, int Chid, int Cout,
                                      float eps, void* stream) {
  const bool ln = gamma != nullptr;
  const int cfg = config_of(Cin, Chid, Cout, ln);
  if (cfg < 0 || !shape_ok(S, N) || !x || !W1 || !b1 || !W2 || !b2 || !y ||
      (ln && (!beta || !mean || !rstd)) || (!ln && (beta || mean || rstd)) ||
      xstride < (int64_t)Cin * N || ystride < (int64_t)Cout * N ||
      (res && rstride < (int64_t)Cout * N))
    return (int)hipErrorInvalidValue;
  const dim3 grid(cdiv(N, kPts), S);
  hipStream_t st = (hipStream_t)stream;
  if (cfg == 0)
    mlp_fwd_kernel<32, 32, 32, true><<<grid, kBlock, 0, st>>>(
        x, xstride, gamma, beta, W1, b1, W2, b2, res, rstride, y, ystride, mean, rstd, N, eps);
  else
    mlp_fwd_kernel<4, 64, 32, false><<<grid, kBlock, 0, st>>>(
        x, xstride, gamma, beta, W1, b1, W2, b2, res, rstride, y, ystride, mean, rstd, N, eps);
  return (int)hipGetLastError();
}

BLINDNO_API int64_t blindno_plane_mlp_bwd_scratch_floats(int S, int N, int Cin, int Chid,
                                                         int Cout) {
  if (!shape_ok(S, N) || (config_of(Cin, Chid, Cout, true) < 0 && config_of(Cin, Chid, Cout, false) < 0))
    return -1;
  return (int64_t)S * cdiv(N, kPts) * partial_floats(Cin, Chid, Cout);
}

BLINDNO_API int blindno_plane_mlp_bwd(const float* dy, int64_t dystride, const float* x,
                                      int64_t xstride, const float* gamma, const float* beta,
                                      const float* W1, const float* b1, const float* W2,
                                      const float* mean, const float* rstd, float* scratch,
                                      float* dx, int64_t dxstride, float* dW1, float* db1,
                                      float* dW2, float* db2, float* dgamma, float* dbeta, int S,
                                      int N, int Cin, int Chid, int Cout, void* stream) {
  const bool ln = gamma != nullptr;
  const int cfg = config_of(Cin, Chid, Cout, ln);
  if (cfg < 0 || !shape_ok(S, N) || !dy || !x || !W1 || !b1 || !W2 || !scratch || !dx || !dW1 ||
      !db1 || !dW2 || !db2 || (ln && (!beta || !mean || !rstd || !dgamma || !dbeta)) ||
      (!ln && (beta || mean || rstd || dgamma || dbeta)) || dystride < (int64_t)Cout * N ||
      xstride < (int64_t)Cin * N || dxstride < (int64_t)Cin * N)
    return (int)hipErrorInvalidValue;
  const int nblk = cdiv(N, kPts);
  const dim3 grid(nblk, S);
  hipStream_t st = (hipStream_t)stream;
  if (cfg == 0)
    mlp_bwd_kernel<32, 32, 32, true><<<grid, kBlock, 0, st>>>(
        dy, dystride, x, xstride, gamma, beta, W1, b1, W2, mean, rstd, dx, dxstride, scratch, N, nblk);
  else
    mlp_bwd_kernel<4, 64, 32, false><<<grid, kBlock, 0, st>>>(
        dy, dystride, x, xstride, gamma, beta, W1, b1, W2, mean, rstd, dx, dxstride, scratch, N, nblk);
  const int E = partial_floats(Cin, Chid, Cout);
  FinArgs fa{scratch, S * nblk, E, Chid * Cin, Chid * Cin + Chid, Chid * Cin + Chid + Cout * Chid,
             Chid * Cin + Chid + Cout * Chid + Cout, E - Cin, dW1, db1, dW2, db2, dgamma, dbeta};
  mlp_finish_kernel<<<cdiv(E, kSeg), kBlock, 0, st>>>(fa);
  return (int)hipGetLastError();
}
