// Bag token attention of NIOFP2D_attn (2d_FPE/NIOModules.py:410-504; NC copy
// 2d_Non_conservative_FPE/NIOModules.py:406-) in coefficient space.
//
// The model's tokens are X_b = [gx, gy, u_1 .. u_L] with u_l = (w_l . basis + b0) / sqrt(P)
// (DeepOnetNoBiasOrg.forward), so X_b = C_b Phi^T with
//   Phi (S, Q) = [gx, gy, scale basis_0 .. scale basis_{P-1}, scale 1],  Q = P + 3, scale = 1/sqrt(P),
//   C_b (T, Q): rows 0, 1 = e_0, e_1, row 2 + l = [0, 0, w[b, l, :], b0],  T = L + 2.
// Forward:  M = Phi^T Phi (the only reduction over S, shared by the batch);
//   per bag  A = softmax_rows(C M C^T / sqrt(S)), cs_s = sum_t A[t, s], v = C^T cs / T;
//   y[b, p, c] = fc0w[c] (Phi[p] . v_b) + fc0b[c]     (= the reference's (A X)^T w0 / T + bias).
// Backward: dm = dy . fc0w, dv_b = sum_p dm[b, p] Phi[p], dcs = C dv / T,
//   dS = A o (dcs_row - A dcs), E = dS C, F = dS^T C,
//   dC = cs dv^T / T + (E + F) M / sqrt(S)             ((dS + dS^T) C M, regrouped: C M is not needed),
//   dM = sum_b C^T E / sqrt(S),  dPhi[p] = Phi[p] (dM + dM^T) + sum_b dm[b, p] v_b.
// Nothing of size B L S or T S exists: S appears in three streaming passes over basis (moments,
// expansion to y, dv and dbasis).  Every reduction is a fixed-order sum (per-workgroup partials
// added in index order, bags in index order); there are no atomics.
#include "common.h"
#include "blindno.h"

using namespace blindno;

namespace {

constexpr int kMaxP = 64;                  // basis functions, as csrc/deeponet.hip
constexpr int kMaxT = 256;                 // tokens, as csrc/attn.hip
constexpr int kMaxQ = kMaxP + 3;
constexpr int kMomChunk = 128;             // points per workgroup (one partial) of the moments
constexpr int kPts = 128;                  // points per workgroup of the backward's passes
constexpr int kWaves = kBlock / 64;
constexpr int kMaxDevices = 64;

__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v = fmaxf(v, __shfl_xor(v, off, 64));
  return v;
}

// Phi[p, j]
__device__ __forceinline__ float phi_at(const float* __restrict__ grid,
                                        const float* __restrict__ basis, int64_t p, int j, int P,
                                        float scale) {
  if (j < 2) return grid[p * 2 + j];
  return j < P + 2 ? scale * basis[p * P + (j - 2)] : scale;
}

// C[t, j] of bag b
__device__ __forceinline__ float coef_at(const float* __restrict__ w, const float* __restrict__ b0,
                                         int b, int t, int j, int L, int P) {
  if (t < 2) return j == t ? 1.0f : 0.0f;
  if (j < 2) return 0.0f;
  return j < P + 2 ? w[((int64_t)b * L + (t - 2)) * P + (j - 2)] : b0[0];
}

// partial[blk][i Q + j] = sum over the workgroup's points of Phi[p, i] Phi[p, j].  The workgroup
// stages its kMomChunk points once; each thread then takes the entries tid, tid + kBlock, .. one
// after the other, each a rolled sum over the points with one accumulator (no per-thread array, so
// nothing spills).  (i, j) and (j, i) run the same products in the same order, so M is symmetric
// bit for bit.
__global__ __launch_bounds__(kBlock) void moments_kernel(const float* __restrict__ grid,
                                                         const float* __restrict__ basis,
                                                         float* __restrict__ partial, int S, int P,
                                                         float scale) {
  __shared__ float sphi[kMomChunk * kMaxQ];      // [point][Q]
  const int Q = P + 3, QQ = Q * Q, tid = threadIdx.x;
  const int64_t p0 = (int64_t)blockIdx.x * kMomChunk;
  const int n = (int)min((int64_t)kMomChunk, S - p0);
  for (int e = tid; e < n * Q; e += kBlock) {
    const int q = e / Q, j = e - q * Q;
    sphi[e] = phi_at(grid, basis, p0 + q, j, P, scale);
  }
  __syncthreads();
  float* pp = partial + (int64_t)blockIdx.x * QQ;
  for (int e = tid; e < QQ; e += kBlock) {
    const int i = e / Q, j = e - i * Q;
    const float* a = sphi + i;
    const float* b = sphi + j;
    float acc = 0.f;
#pragma unroll 4
    for (int q = 0; q < n; ++q) acc = fmaf(a[q * Q], b[q * Q], acc);
    pp[e] = acc;
  }
}

__global__ __launch_bounds__(kBlock) void moments_finish_kernel(const float* __restrict__ partial,
                                                                float* __restrict__ M, int nblk,
                                                                int QQ) {
  const int e = blockIdx.x * kBlock + threadIdx.x;
  if (e >= QQ) return;
  float acc = 0.f;
  for (int j = 0; j < nblk; ++j) acc += partial[(int64_t)j * QQ + e];
  M[e] = acc;
}

// LDS floats of the per-bag kernels (row stride Qp = Q | 1: odd, so lanes over rows hit 64 banks)
__host__ __device__ inline int row_stride(int Q) { return Q | 1; }
inline size_t coef_fwd_lds(int T, int Q) {
  return sizeof(float) * ((size_t)2 * T * row_stride(Q) + (size_t)(kWaves + 1) * T);
}
inline size_t coef_bwd_lds(int T, int Q) {
  return sizeof(float) * ((size_t)2 * T * row_stride(Q) + (size_t)(2 * kWaves + 4) * T +
                          (size_t)(kWaves + 1) * row_stride(Q));
}

// One workgroup per bag: C and C M in LDS; one wave per row of the logits, lanes over the columns
// (up to four per lane), so a row's softmax never leaves registers and A goes straight to memory.
__global__ __launch_bounds__(kBlock) void coef_fwd_kernel(const float* __restrict__ w,
                                                          const float* __restrict__ b0,
                                                          const float* __restrict__ M,
                                                          float* __restrict__ A,
                                                          float* __restrict__ cs,
                                                          float* __restrict__ v, int L, int P,
                                                          float inv_sqrt_s) {
  extern __shared__ float lds[];
  const int T = L + 2, Q = P + 3, Qp = row_stride(Q), b = blockIdx.x, tid = threadIdx.x;
  float* Cs = lds;                       // [T][Qp]
  float* CMs = Cs + T * Qp;              // [T][Qp]
  float* csw = CMs + T * Qp;             // [kWaves][T] column sums of each wave's rows
  float* css = csw + kWaves * T;         // [T]
  for (int e = tid; e < T * Q; e += kBlock) {
    const int t = e / Q, j = e - t * Q;
    Cs[t * Qp + j] = coef_at(w, b0, b, t, j, L, P);
  }
  __syncthreads();
  for (int e = tid; e < T * Q; e += kBlock) {
    const int t = e / Q, j = e - t * Q;
    float acc = 0.f;
    for (int k = 0; k < Q; ++k) acc = fmaf(Cs[t * Qp + k], M[k * Q + j], acc);
    CMs[t * Qp + j] = acc;
  }
  __syncthreads();
  const int lane = tid & 63, wave = tid >> 6;
  float ccol[4] = {0.f, 0.f, 0.f, 0.f};
  float* Ab = A + (int64_t)b * T * T;
  for (int t = wave; t < T; t += kWaves) {
    float lg[4];
    float mx = -INFINITY;
#pragma unroll
    for (int jj = 0; jj < 4; ++jj) {
      const int s = lane + 64 * jj;
      lg[jj] = -INFINITY;
      if (s < T) {
        float acc = 0.f;
        for (int k = 0; k < Q; ++k) acc = fmaf(CMs[t * Qp + k], Cs[s * Qp + k], acc);
        lg[jj] = acc * inv_sqrt_s;
        mx = fmaxf(mx, lg[jj]);
      }
    }
    mx = wave_max(mx);
    float den = 0.f;
#pragma unroll
    for (int jj = 0; jj < 4; ++jj) {
      lg[jj] = lane + 64 * jj < T ? expf(lg[jj] - mx) : 0.f;
      den += lg[jj];
    }
    den = wave_sum(den);
    const float inv = 1.0f / den;
#pragma unroll
    for (int jj = 0; jj < 4; ++jj) {
      const int s = lane + 64 * jj;
      if (s < T) {
        const float a = lg[jj] * inv;
        Ab[t * T + s] = a;
        ccol[jj] += a;
      }
    }
  }
#pragma unroll
  for (int jj = 0; jj < 4; ++jj)
    if (lane + 64 * jj < T) csw[wave * T + lane + 64 * jj] = ccol[jj];
  __syncthreads();
  for (int s = tid; s < T; s += kBlock) {
    float c = csw[s];
    for (int k = 1; k < kWaves; ++k) c += csw[k * T + s];
    css[s] = c;
    cs[(int64_t)b * T + s] = c;
  }
  __syncthreads();
  const float inv_t = 1.0f / (float)T;
  for (int j = tid; j < Q; j += kBlock) {
    float acc = 0.f;
    for (int t = 0; t < T; ++t) acc = fmaf(Cs[t * Qp + j], css[t], acc);
    v[(int64_t)b * Q + j] = acc * inv_t;
  }
}

// y[b, p, c] = fc0w[c] (Phi[p] . v_b) + fc0b[c]
__global__ __launch_bounds__(kBlock) void expand_kernel(const float* __restrict__ basis,
                                                        const float* __restrict__ grid,
                                                        const float* __restrict__ v,
                                                        const float* __restrict__ fc0w,
                                                        const float* __restrict__ fc0b,
                                                        float* __restrict__ y, int B, int S, int P,
                                                        int width, float scale) {
  __shared__ float sv[kMaxQ];
  const int Q = P + 3, tid = threadIdx.x;
  const int64_t p = (int64_t)blockIdx.x * kBlock + tid;
  for (int b = blockIdx.y; b < B; b += gridDim.y) {
    __syncthreads();
    if (tid < Q) sv[tid] = v[(int64_t)b * Q + tid];
    __syncthreads();
    if (p < S) {
      const float* bp = basis + p * P;
      float acc = sv[Q - 1];
      for (int k = 0; k < P; ++k) acc = fmaf(sv[2 + k], bp[k], acc);
      const float m = fmaf(scale, acc, fmaf(sv[0], grid[p * 2], sv[1] * grid[p * 2 + 1]));
      float* yo = y + ((int64_t)b * S + p) * width;
      for (int c = 0; c < width; ++c) yo[c] = fmaf(fc0w[c], m, fc0b[c]);
    }
  }
}

// dm[b, p] = sum_c fc0w[c] dy[b, p, c] and the workgroup's partial of dv:
//   partial[blk][b][j] = sum_{p in blk} dm[b, p] Phi[p, j]
// (the basis tile is staged once for all bags; one wave per j, lanes over the points).
__global__ __launch_bounds__(kBlock) void dv_kernel(const float* __restrict__ dy,
                                                    const float* __restrict__ basis,
                                                    const float* __restrict__ grid,
                                                    const float* __restrict__ fc0w,
                                                    float* __restrict__ dm,
                                                    float* __restrict__ partial, int B, int S,
                                                    int P, int width, float scale) {
  extern __shared__ float lds[];
  const int Q = P + 3, Pp = row_stride(P), tid = threadIdx.x;
  float* sb = lds;                       // [kPts][Pp]
  float* sg = sb + kPts * Pp;            // [kPts][2]
  float* dml = sg + kPts * 2;            // [kPts]
  const int64_t p0 = (int64_t)blockIdx.x * kPts;
  const int n = (int)min((int64_t)kPts, S - p0);
  for (int e = tid; e < kPts * P; e += kBlock) {
    const int q = e / P, k = e - q * P;
    sb[q * Pp + k] = q < n ? basis[(p0 + q) * P + k] : 0.f;
  }
  for (int e = tid; e < kPts * 2; e += kBlock) sg[e] = (e >> 1) < n ? grid[p0 * 2 + e] : 0.f;
  const int lane = tid & 63, wave = tid >> 6;
  for (int b = 0; b < B; ++b) {
    __syncthreads();
    if (tid < kPts) {
      float a = 0.f;
      if (tid < n) {
        const int64_t o = (int64_t)b * S + p0 + tid;
        for (int c = 0; c < width; ++c) a = fmaf(fc0w[c], dy[o * width + c], a);
        dm[o] = a;
      }
      dml[tid] = a;
    }
    __syncthreads();
    for (int j = wave; j < Q; j += kWaves) {
      float acc = 0.f;
      for (int q = lane; q < kPts; q += 64) {
        const float ph = j < 2 ? sg[q * 2 + j] : (j < Q - 1 ? scale * sb[q * Pp + (j - 2)] : scale);
        acc = fmaf(ph, dml[q], acc);
      }
      acc = wave_sum(acc);
      if (lane == 0) partial[((int64_t)blockIdx.x * B + b) * Q + j] = acc;
    }
  }
}

// One workgroup per bag: dv from its partials, dcs, the softmax backward, E = dS C and F = dS^T C
// one row per wave, dC's rows (dw and the b0 column) from (E + F) M, and the bag's dM = C^T E.
__global__ __launch_bounds__(kBlock) void coef_bwd_kernel(
    const float* __restrict__ w, const float* __restrict__ b0, const float* __restrict__ M,
    const float* __restrict__ A, const float* __restrict__ cs, const float* __restrict__ dvpart,
    float* __restrict__ dw, float* __restrict__ dMb, float* __restrict__ db0part, int nblk, int B,
    int L, int P, float inv_sqrt_s) {
  extern __shared__ float lds[];
  const int T = L + 2, Q = P + 3, Qp = row_stride(Q), b = blockIdx.x, tid = threadIdx.x;
  float* Cs = lds;                       // [T][Qp]
  float* Es = Cs + T * Qp;               // [T][Qp]
  float* rowE = Es + T * Qp;             // [kWaves][T]  dS[t, :] of the wave's row
  float* rowF = rowE + kWaves * T;       // [kWaves][T]  dS[:, t]
  float* dcs = rowF + kWaves * T;        // [T]
  float* r = dcs + T;                    // [T]  A dcs
  float* css = r + T;                    // [T]
  float* dlast = css + T;                // [T]  dC[t, Q - 1]
  float* hrow = dlast + T;               // [kWaves][Qp]  (E + F)[t, :]
  float* dvs = hrow + kWaves * Qp;       // [Qp]
  const float* Ab = A + (int64_t)b * T * T;
  const float inv_t = 1.0f / (float)T;
  for (int e = tid; e < T * Q; e += kBlock) {
    const int t = e / Q, j = e - t * Q;
    Cs[t * Qp + j] = coef_at(w, b0, b, t, j, L, P);
  }
  for (int j = tid; j < Q; j += kBlock) {
    float acc = 0.f;
    for (int k = 0; k < nblk; ++k) acc += dvpart[((int64_t)k * B + b) * Q + j];
    dvs[j] = acc;
  }
  for (int s = tid; s < T; s += kBlock) css[s] = cs[(int64_t)b * T + s];
  __syncthreads();
  for (int t = tid; t < T; t += kBlock) {
    float acc = 0.f;
    for (int j = 0; j < Q; ++j) acc = fmaf(Cs[t * Qp + j], dvs[j], acc);
    dcs[t] = acc * inv_t;
  }
  __syncthreads();
  const int lane = tid & 63, wave = tid >> 6;
  for (int t = wave; t < T; t += kWaves) {
    float acc = 0.f;
    for (int s = lane; s < T; s += 64) acc = fmaf(Ab[t * T + s], dcs[s], acc);
    acc = wave_sum(acc);
    if (lane == 0) r[t] = acc;
  }
  __syncthreads();
  float* re = rowE + wave * T;
  float* rf = rowF + wave * T;
  float* hr = hrow + wave * Qp;
  // every wave runs the same number of rounds (the barriers are workgroup-wide); a wave past the
  // last row repeats row T - 1 into its own buffers and writes nothing
  for (int t0 = 0; t0 < T; t0 += kWaves) {
    const bool live = t0 + wave < T;
    const int t = live ? t0 + wave : T - 1;
    const float rt = r[t], dt = dcs[t];
    for (int s = lane; s < T; s += 64) {
      re[s] = Ab[t * T + s] * (dcs[s] - rt);
      rf[s] = Ab[s * T + t] * (dt - r[s]);
    }
    __syncthreads();
    for (int j = lane; j < Q; j += 64) {
      float e = 0.f, f = 0.f;
      for (int s = 0; s < T; ++s) {
        const float c = Cs[s * Qp + j];
        e = fmaf(re[s], c, e);
        f = fmaf(rf[s], c, f);
      }
      if (live) Es[t * Qp + j] = e;
      hr[j] = e + f;
    }
    __syncthreads();
    if (live && t >= 2) {
      const float ct = css[t] * inv_t;
      for (int j = 2 + lane; j < Q; j += 64) {
        float g = 0.f;
        for (int i = 0; i < Q; ++i) g = fmaf(hr[i], M[i * Q + j], g);
        const float dc = fmaf(g, inv_sqrt_s, ct * dvs[j]);
        if (j < Q - 1) dw[((int64_t)b * L + (t - 2)) * P + (j - 2)] = dc;
        else dlast[t] = dc;
      }
    }
    __syncthreads();
  }
  __syncthreads();
  const int QQ = Q * Q;
  for (int e = tid; e < QQ; e += kBlock) {
    const int i = e / Q, j = e - i * Q;
    float acc = 0.f;
    for (int t = 0; t < T; ++t) acc = fmaf(Cs[t * Qp + i], Es[t * Qp + j], acc);
    dMb[(int64_t)b * QQ + e] = acc * inv_sqrt_s;
  }
  if (tid == 0) {
    float acc = 0.f;
    for (int t = 2; t < T; ++t) acc += dlast[t];
    db0part[b] = acc;
  }
}

// dMsym = sum_b (dM_b + dM_b^T) and db0 = sum_b db0part[b], bags in index order
__global__ __launch_bounds__(kBlock) void dm_finish_kernel(const float* __restrict__ dMb,
                                                           const float* __restrict__ db0part,
                                                           float* __restrict__ dMsym,
                                                           float* __restrict__ db0, int B, int Q) {
  const int QQ = Q * Q, e = blockIdx.x * kBlock + threadIdx.x;
  if (e == 0) {
    float acc = 0.f;
    for (int b = 0; b < B; ++b) acc += db0part[b];
    db0[0] = acc;
  }
  if (e >= QQ) return;
  const int i = e / Q, j = e - i * Q;
  float acc = 0.f;
  for (int b = 0; b < B; ++b) acc += dMb[(int64_t)b * QQ + e] + dMb[(int64_t)b * QQ + j * Q + i];
  dMsym[e] = acc;
}

// dbasis[p, k] = scale (Phi[p] . dMsym[:, 2 + k] + sum_b dm[b, p] v_b[2 + k])
__global__ __launch_bounds__(kBlock) void dbasis_kernel(const float* __restrict__ basis,
                                                        const float* __restrict__ grid,
                                                        const float* __restrict__ dMsym,
                                                        const float* __restrict__ dm,
                                                        const float* __restrict__ v,
                                                        float* __restrict__ dbasis, int B, int S,
                                                        int P, float scale) {
  extern __shared__ float lds[];         // [kPts][Qp]
  const int Q = P + 3, Qp = row_stride(Q), tid = threadIdx.x;
  const int64_t p0 = (int64_t)blockIdx.x * kPts;
  const int n = (int)min((int64_t)kPts, S - p0);
  for (int e = tid; e < n * Q; e += kBlock) {
    const int q = e / Q, j = e - q * Q;
    lds[q * Qp + j] = phi_at(grid, basis, p0 + q, j, P, scale);
  }
  __syncthreads();
  for (int e = tid; e < n * P; e += kBlock) {
    const int q = e / P, k = e - q * P;
    float acc = 0.f;
    for (int i = 0; i < Q; ++i) acc = fmaf(lds[q * Qp + i], dMsym[i * Q + 2 + k], acc);
    for (int b = 0; b < B; ++b) acc = fmaf(dm[(int64_t)b * S + p0 + q], v[(int64_t)b * Q + 2 + k], acc);
    dbasis[(p0 + q) * P + k] = scale * acc;
  }
}

bool field_ok(int S, int P) { return S >= 1 && P >= 1 && P <= kMaxP; }
bool bag_ok(int B, int L, int S, int P, int width) {
  return field_ok(S, P) && B >= 1 && L >= 1 && L + 2 <= kMaxT && width >= 1;
}

// More dynamic LDS than the default 64 KB cap: raise the kernel's limit to what its largest shape
// needs, once per device (a refusal surfaces as the launch's own error; no error is cleared here).
template <typename K>
void allow_lds(K kernel, size_t cap_bytes, bool* done) {
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= kMaxDevices || done[dev]) return;
  done[dev] = true;
  (void)hipFuncSetAttribute(reinterpret_cast<const void*>(kernel),
                            hipFuncAttributeMaxDynamicSharedMemorySize, (int)cap_bytes);
}

}  // namespace

BLINDNO_API int blindno_nioattn_moments_nblk(int S) { return S < 1 ? -1 : cdiv(S, kMomChunk); }

BLINDNO_API int64_t blindno_nioattn_moments_scratch_floats(int S, int P) {
  if (!field_ok(S, P)) return -1;
  return (int64_t)cdiv(S, kMomChunk) * (P + 3) * (P + 3);
}

BLINDNO_API int blindno_nioattn_moments(const float* grid, const float* basis, float* partial,
                                        float* M, int nblk, int S, int P, void* stream) {
  if (!field_ok(S, P) || !grid || !basis || !partial || !M ||
      nblk != blindno_nioattn_moments_nblk(S))
    return (int)hipErrorInvalidValue;
  const int Q = P + 3;
  const float scale = 1.0f / sqrtf((float)P);
  hipStream_t st = (hipStream_t)stream;
  moments_kernel<<<nblk, kBlock, 0, st>>>(grid, basis, partial, S, P, scale);
  moments_finish_kernel<<<cdiv(Q * Q, kBlock), kBlock, 0, st>>>(partial, M, nblk, Q * Q);
  return (int)hipGetLastError();
}

BLINDNO_API int blindno_nioattn_fwd(const float* w, const float* b0, const float* basis,
                                    const float* grid, const float* M, const float* fc0w,
                                    const float* fc0b, float* A, float* cs, float* v, float* y,
                                    int B, int L, int S, int P, int width, void* stream) {
  if (!bag_ok(B, L, S, P, width) || !w || !b0 || !basis || !grid || !M || !fc0w || !fc0b || !A ||
      !cs || !v || !y)
    return (int)hipErrorInvalidValue;
  const int T = L + 2, Q = P + 3;
  const float scale = 1.0f / sqrtf((float)P), inv_sqrt_s = 1.0f / sqrtf((float)S);
  hipStream_t st = (hipStream_t)stream;
  const size_t lds = coef_fwd_lds(T, Q);
  if (lds > 64 * 1024) {
    static bool done[kMaxDevices];
    allow_lds(&coef_fwd_kernel, coef_fwd_lds(kMaxT, kMaxQ), done);
  }
  coef_fwd_kernel<<<B, kBlock, lds, st>>>(w, b0, M, A, cs, v, L, P, inv_sqrt_s);
  expand_kernel<<<dim3(cdiv(S, kBlock), B < 1024 ? B : 1024), kBlock, 0, st>>>(
      basis, grid, v, fc0w, fc0b, y, B, S, P, width, scale);
  return (int)hipGetLastError();
}

BLINDNO_API int blindno_nioattn_bwd_nblk(int S) { return S < 1 ? -1 : cdiv(S, kPts); }

BLINDNO_API int64_t blindno_nioattn_bwd_scratch_floats(int B, int S, int P) {
  if (!field_ok(S, P) || B < 1) return -1;
  const int64_t Q = P + 3;
  return (int64_t)B * S + (int64_t)cdiv(S, kPts) * B * Q + (int64_t)B * Q * Q + Q * Q + B;
}

BLINDNO_API int blindno_nioattn_bwd(const float* dy, const float* w, const float* b0,
                                    const float* basis, const float* grid, const float* M,
                                    const float* fc0w, const float* A, const float* cs,
                                    const float* v, float* scratch, float* dw, float* dbasis,
                                    float* db0, int nblk, int B, int L, int S, int P, int width,
                                    void* stream) {
  if (!bag_ok(B, L, S, P, width) || !dy || !w || !b0 || !basis || !grid || !M || !fc0w || !A ||
      !cs || !v || !scratch || !dw || !dbasis || !db0 || nblk != blindno_nioattn_bwd_nblk(S))
    return (int)hipErrorInvalidValue;
  const int T = L + 2, Q = P + 3;
  const float scale = 1.0f / sqrtf((float)P), inv_sqrt_s = 1.0f / sqrtf((float)S);
  float* dm = scratch;                                   // (B, S)
  float* dvpart = dm + (int64_t)B * S;                   // (nblk, B, Q)
  float* dMb = dvpart + (int64_t)nblk * B * Q;           // (B, Q, Q)
  float* dMsym = dMb + (int64_t)B * Q * Q;               // (Q, Q)
  float* db0part = dMsym + (int64_t)Q * Q;               // (B)
  hipStream_t st = (hipStream_t)stream;
  const size_t lds_dv = sizeof(float) * ((size_t)kPts * row_stride(P) + kPts * 3);
  dv_kernel<<<nblk, kBlock, lds_dv, st>>>(dy, basis, grid, fc0w, dm, dvpart, B, S, P, width, scale);
  const size_t lds = coef_bwd_lds(T, Q);
  if (lds > 64 * 1024) {
    static bool done[kMaxDevices];
    allow_lds(&coef_bwd_kernel, coef_bwd_lds(kMaxT, kMaxQ), done);
  }
  coef_bwd_kernel<<<B, kBlock, lds, st>>>(w, b0, M, A, cs, dvpart, dw, dMb, db0part, nblk, B, L, P,
                                          inv_sqrt_s);
  dm_finish_kernel<<<cdiv(Q * Q, kBlock), kBlock, 0, st>>>(dMb, db0part, dMsym, db0, B, Q);
  const size_t lds_db = sizeof(float) * (size_t)kPts * row_stride(Q);
  dbasis_kernel<<<nblk, kBlock, lds_db, st>>>(basis, grid, dMsym, dm, v, dbasis, B, S, P, scale);
  return (int)hipGetLastError();
}
