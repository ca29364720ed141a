// 3D kernels of the attention UNet on 3D bags, PermInvUNet_attn3D (blindno/unet3d.py): what
// csrc/unet.hip does in 2D and has no 3D form.
//
//   dwconv3d   7x7x7 depthwise convolution of ConvNeXtBlock3D (groups = C, same padding; any odd
//              extents <= 7 per axis), its input gradient (the same kernel on the
//              point-reflected taps) and its weight gradient
//   maxpool3d  MaxPool3d(2) (floor; first maximum in scan order, NaN wins)
//   convt3d    ConvTranspose3d(kernel = stride = 2, output_padding) of the up path
//
// Depthwise convolution.  343 taps per output voxel: the 2D kernel's one-thread-per-output loop
// over global memory would read 343 values per FMA chain.  Here a workgroup owns one
// kTD x kTH x kTW = 5 x 10 x 40 output tile of one (n, c) volume (a 40^3 volume is 8 x 4 x 1
// tiles exactly).  It stages the tile with its halo once in LDS -- (5+6) x (10+6) rows of 48
// columns (the 40 + 2 x 3 halo columns, widened to 4 on each side so that a thread's window
// starts 16-B aligned), row stride 52 floats = 13 16-B slots (odd: neighbouring rows start on
// different slots): 11 x 16 x 52 x 4 B = 36 608 B, four workgroups = 16 waves per CU =
// 4 waves per SIMD.  A thread produces 8 consecutive outputs along W: per (i, j) tap row it
// reads its 16-float window and feeds 7 x 8 = 56 FMAs from it (3.5 FMA per LDS dword); the 7
// taps of the row are wave-uniform and come through the scalar cache as FMA operands.  (hipcc
// packs the FMAs into v_pk_fma_f32 and reads the window as ds_read2_b32 pairs, not as 16-B
// reads: the LDS read rate is what the kernel runs at)
// 250 of the 256 threads compute (5 along W x 10 x 5); all 256 stage.
//
// Weight gradient.  343 + 1 sums per channel do not fit a thread, so the taps are split over
// the grid: workgroup (split, c, i) owns depth tap i -- at most 49 + 1 accumulators per thread
// -- and walks its range of the channel's (n, tile) items with the same tile and thread map:
// the x tile shifted by i (5 planes with their (j, k) halo) is staged in LDS, a thread holds its
// 8 dy values in registers and accumulates dy x window for every (j, k).  One fixed-order block
// reduction per accumulator at the end; ranges are summed in range order.
#include "common.h"
#include "blindno.h"

using namespace blindno;

namespace {

constexpr int kTD = 5, kTH = 10, kTW = 40;   // output tile
constexpr int kRW = 8;                       // outputs per thread along W
constexpr int kNW = kTW / kRW;               // threads along W
constexpr int kMaxK = 7;
constexpr int kPD = kTD + kMaxK - 1;         // staged planes
constexpr int kPH = kTH + kMaxK - 1;         // staged rows per plane
constexpr int kLW = kTW + 8;                 // staged columns: x columns [w0 - 4, w0 + 44)
constexpr int kLS = 52;                      // LDS row stride (floats)
constexpr int kDwThreads = kNW * kTH * kTD;  // 250 computing threads
static_assert(kDwThreads <= kBlock && kPH == 16 && kLW == 48 && kLS % 4 == 0 && kLS >= kLW, "tile");

struct DwTiles {
  int ntd, nth, ntw;
  __host__ __device__ int count() const { return ntd * nth * ntw; }
};

inline DwTiles dw_tiles(int D, int H, int W) {
  return DwTiles{(D + kTD - 1) / kTD, (H + kTH - 1) / kTH, (W + kTW - 1) / kTW};
}

// Stage planes [dlo, dlo + np) x rows [hlo, hlo + nr) x columns [w0 - 4, w0 + 44) of one volume
// into s[(p kPH + r) kLS + col], zero outside the volume.  16 rows x 16 columns per pass.
__device__ __forceinline__ void dw_stage(float* __restrict__ s, const float* __restrict__ xp, int D,
                                         int H, int W, int dlo, int np, int hlo, int nr, int w0) {
  const int cg = threadIdx.x & 15, rs = threadIdx.x >> 4;
  for (int p = 0; p < np; ++p) {
    const int gd = dlo + p;
    const bool dok = gd >= 0 && gd < D;
    for (int r = rs; r < nr; r += 16) {
      const int gh = hlo + r;
      const bool ok = dok && gh >= 0 && gh < H;
      const float* row = xp + ((int64_t)gd * H + gh) * W;
      float* dst = s + (p * kPH + r) * kLS;
#pragma unroll
      for (int q = 0; q < kLW / 16; ++q) {
        const int col = cg + 16 * q, gw = w0 - 4 + col;
        dst[col] = (ok && gw >= 0 && gw < W) ? row[gw] : 0.f;
      }
    }
  }
}

__device__ __forceinline__ void dw_window(float (&in)[16], const float* sp) {
  const float4* v = reinterpret_cast<const float4*>(sp);
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const float4 a = v[q];
    in[4 * q] = a.x;
    in[4 * q + 1] = a.y;
    in[4 * q + 2] = a.z;
    in[4 * q + 3] = a.w;
  }
}

// y = b + conv(x, W) (FLIP false) or conv(x, point-reflected W) (FLIP true: the input gradient)
template <int KW, bool FLIP>
__global__ __launch_bounds__(kBlock) void dwconv3d_kernel(
    const float* __restrict__ x, const float* __restrict__ wt, const float* __restrict__ b,
    float* __restrict__ y, int C, int D, int H, int W, int KD, int KH, DwTiles nt) {
  __shared__ __align__(16) float s[kPD * kPH * kLS];
  const unsigned ntile = (unsigned)nt.count();
  const unsigned nc = blockIdx.x / ntile, tile = blockIdx.x - nc * ntile;
  const int c = (int)(nc % (unsigned)C);
  const int w0 = (int)(tile % nt.ntw) * kTW;
  const int h0 = (int)((tile / nt.ntw) % nt.nth) * kTH;
  const int d0 = (int)(tile / (nt.ntw * nt.nth)) * kTD;
  const int64_t vol = (int64_t)D * H * W;
  dw_stage(s, x + (int64_t)nc * vol, D, H, W, d0 - KD / 2, kTD + KD - 1, h0 - KH / 2, kTH + KH - 1, w0);
  __syncthreads();
  if (threadIdx.x >= kDwThreads) return;
  const int tw = threadIdx.x % kNW, th = (threadIdx.x / kNW) % kTH, td = threadIdx.x / (kNW * kTH);
  const int T = KD * KH * KW;
  const float* wp = wt + (int64_t)c * T;
  float acc[kRW];
  const float bias = b ? b[c] : 0.f;
#pragma unroll
  for (int o = 0; o < kRW; ++o) acc[o] = bias;
  for (int i = 0; i < KD; ++i)
    for (int j = 0; j < KH; ++j) {
      float in[16];
      dw_window(in, s + ((td + i) * kPH + th + j) * kLS + kRW * tw);
      const int t0 = (i * KH + j) * KW;
#pragma unroll
      for (int k = 0; k < KW; ++k) {
        const float wv = FLIP ? wp[T - 1 - t0 - k] : wp[t0 + k];
#pragma unroll
        for (int o = 0; o < kRW; ++o) acc[o] = fmaf(wv, in[o + k + 4 - KW / 2], acc[o]);
      }
    }
  const int gd = d0 + td, gh = h0 + th, gw = w0 + kRW * tw;
  if (gd >= D || gh >= H) return;
  float* yp = y + (int64_t)nc * vol + ((int64_t)gd * H + gh) * W;
#pragma unroll
  for (int o = 0; o < kRW; ++o)
    if (gw + o < W) yp[gw + o] = acc[o];
}

__device__ __forceinline__ float block_sum(float v, float* red) {
  // red: >= 4 floats of LDS; returns the sum in every thread (fixed order)
  v = wave_sum(v);
  const int w = threadIdx.x >> 6, nw = (blockDim.x + 63) >> 6;
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[w] = v;
  __syncthreads();
  float s = 0.f;
  for (int i = 0; i < nw; ++i) s += red[i];
  return s;
}

// partial[split][c][KD KH KW + 1]: workgroup (split, c, i) writes the KH KW sums of depth tap i
// over its range of the channel's (n, tile) items; the i = 0 workgroup also the bias sum.
template <int KW>
__global__ __launch_bounds__(kBlock) void dwconv3d_wgrad_kernel(
    const float* __restrict__ dy, const float* __restrict__ x, float* __restrict__ partial, int N,
    int C, int D, int H, int W, int KD, int KH, DwTiles nt, int nsplit) {
  __shared__ __align__(16) float s[kTD * kPH * kLS];
  __shared__ float red[8];
  const int split = blockIdx.x, c = blockIdx.y, i = blockIdx.z;
  const int ntile = nt.count();
  const int64_t items = (int64_t)N * ntile;
  const int64_t per = (items + nsplit - 1) / nsplit;
  const int64_t it0 = split * per, it1 = it0 + per < items ? it0 + per : items;
  const int64_t vol = (int64_t)D * H * W;
  const bool comp = threadIdx.x < kDwThreads;
  const int tw = threadIdx.x % kNW, th = (threadIdx.x / kNW) % kTH, td = threadIdx.x / (kNW * kTH);
  float acc[kMaxK][KW];
  float accb = 0.f;
#pragma unroll
  for (int j = 0; j < kMaxK; ++j)
#pragma unroll
    for (int k = 0; k < KW; ++k) acc[j][k] = 0.f;
  for (int64_t it = it0; it < it1; ++it) {
    const int n = (int)(it / ntile), tile = (int)(it - (int64_t)n * ntile);
    const int w0 = (tile % nt.ntw) * kTW;
    const int h0 = ((tile / nt.ntw) % nt.nth) * kTH;
    const int d0 = (tile / (nt.ntw * nt.nth)) * kTD;
    const int64_t base = ((int64_t)n * C + c) * vol;
    __syncthreads();
    dw_stage(s, x + base, D, H, W, d0 + i - KD / 2, kTD, h0 - KH / 2, kTH + KH - 1, w0);
    __syncthreads();
    const int gd = d0 + td, gh = h0 + th, gw = w0 + kRW * tw;
    if (comp && gd < D && gh < H) {
      const float* gp = dy + base + ((int64_t)gd * H + gh) * W;
      float g[kRW];
#pragma unroll
      for (int o = 0; o < kRW; ++o) {
        g[o] = gw + o < W ? gp[gw + o] : 0.f;
        accb += g[o];
      }
#pragma unroll
      for (int j = 0; j < kMaxK; ++j) {
        if (j < KH) {
          float in[16];
          dw_window(in, s + (td * kPH + th + j) * kLS + kRW * tw);
#pragma unroll
          for (int k = 0; k < KW; ++k)
#pragma unroll
            for (int o = 0; o < kRW; ++o) acc[j][k] = fmaf(g[o], in[o + k + 4 - KW / 2], acc[j][k]);
        }
      }
    }
  }
  const int T = KD * KH * KW;
  float* out = partial + ((int64_t)split * C + c) * (T + 1);
#pragma unroll
  for (int j = 0; j < kMaxK; ++j) {
    if (j < KH) {
#pragma unroll
      for (int k = 0; k < KW; ++k) {
        const float v = block_sum(acc[j][k], red);
        if (threadIdx.x == 0) out[(i * KH + j) * KW + k] = v;
      }
    }
  }
  if (i == 0) {
    const float v = block_sum(accb, red);
    if (threadIdx.x == 0) out[T] = v;
  }
}

// ---------------------------------------------------------------------- max pool
__global__ __launch_bounds__(kBlock) void maxpool3d_fwd_kernel(
    const float* __restrict__ x, float* __restrict__ y, uint8_t* __restrict__ arg, int D, int H,
    int W, int Do, int Ho, int Wo, int KD, int KH, int KW, int64_t total) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= total) return;
  const int wo = (int)(e % Wo);
  const int ho = (int)((e / Wo) % Ho);
  const int od = (int)((e / ((int64_t)Wo * Ho)) % Do);
  const int64_t nc = e / ((int64_t)Wo * Ho * Do);
  const float* xp = x + nc * D * H * W + ((int64_t)(od * KD) * H + ho * KH) * W + wo * KW;
  float m = xp[0];
  int a = 0;
  for (int i = 0; i < KD; ++i)
    for (int j = 0; j < KH; ++j)
      for (int k = 0; k < KW; ++k) {
        const float v = xp[((int64_t)i * H + j) * W + k];
        if (v > m || isnan(v)) {       // first maximum wins; a NaN propagates (torch's rule)
          m = v;
          a = (i * KH + j) * KW + k;
        }
      }
  y[e] = m;
  arg[e] = (uint8_t)a;
}

__global__ __launch_bounds__(kBlock) void maxpool3d_bwd_kernel(
    const float* __restrict__ dy, const uint8_t* __restrict__ arg, float* __restrict__ dx, int D,
    int H, int W, int Do, int Ho, int Wo, int KD, int KH, int KW, int64_t total) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= total) return;
  const int w = (int)(e % W);
  const int h = (int)((e / W) % H);
  const int d = (int)((e / ((int64_t)W * H)) % D);
  const int64_t nc = e / ((int64_t)W * H * D);
  const int od = d / KD, ho = h / KH, wo = w / KW;
  float v = 0.f;
  if (od < Do && ho < Ho && wo < Wo) {
    const int64_t o = ((nc * Do + od) * Ho + ho) * Wo + wo;
    if ((int)arg[o] == ((d - od * KD) * KH + (h - ho * KH)) * KW + (w - wo * KW)) v = dy[o];
  }
  dx[e] = v;
}

// ---------------------------------------------------------------------- transposed conv
// kernel = stride = 2 on three axes; weight (Ci, Co, 2, 2, 2); the output planes past 2 Di / 2 Hi
// / 2 Wi are output_padding: bias only
__global__ __launch_bounds__(kBlock) void convt3d_fwd_kernel(
    const float* __restrict__ x, const float* __restrict__ wt, const float* __restrict__ b,
    float* __restrict__ y, int Ci, int Di, int Hi, int Wi, int Co, int Do, int Ho, int Wo,
    int64_t total) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= total) return;
  const int wo = (int)(e % Wo);
  const int ho = (int)((e / Wo) % Ho);
  const int od = (int)((e / ((int64_t)Wo * Ho)) % Do);
  const int64_t nco = e / ((int64_t)Wo * Ho * Do);
  const int co = (int)(nco % Co);
  const int64_t n = nco / Co;
  float acc = b ? b[co] : 0.f;
  const int di = od >> 1, hi = ho >> 1, wi = wo >> 1;
  if (di < Di && hi < Hi && wi < Wi) {
    const int64_t voli = (int64_t)Di * Hi * Wi;
    const int t = ((od & 1) * 2 + (ho & 1)) * 2 + (wo & 1);
    const float* xp = x + n * Ci * voli + ((int64_t)di * Hi + hi) * Wi + wi;
    const float* wp = wt + (int64_t)co * 8 + t;
    for (int ci = 0; ci < Ci; ++ci) acc = fmaf(xp[ci * voli], wp[(int64_t)ci * Co * 8], acc);
  }
  y[e] = acc;
}

__global__ __launch_bounds__(kBlock) void convt3d_bwd_data_kernel(
    const float* __restrict__ dy, const float* __restrict__ wt, float* __restrict__ dx, int Ci,
    int Di, int Hi, int Wi, int Co, int Do, int Ho, int Wo, int64_t total) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= total) return;
  const int wi = (int)(e % Wi);
  const int hi = (int)((e / Wi) % Hi);
  const int di = (int)((e / ((int64_t)Wi * Hi)) % Di);
  const int64_t nci = e / ((int64_t)Wi * Hi * Di);
  const int ci = (int)(nci % Ci);
  const int64_t n = nci / Ci;
  const int64_t volo = (int64_t)Do * Ho * Wo;
  float acc = 0.f;
  for (int co = 0; co < Co; ++co) {
    const float* gp = dy + (n * Co + co) * volo + ((int64_t)(2 * di) * Ho + 2 * hi) * Wo + 2 * wi;
    const float* wp = wt + ((int64_t)ci * Co + co) * 8;
#pragma unroll
    for (int t = 0; t < 8; ++t)
      acc = fmaf(wp[t], gp[((int64_t)(t >> 2) * Ho + ((t >> 1) & 1)) * Wo + (t & 1)], acc);
  }
  dx[e] = acc;
}

// partial[n S + s][Ci Co 8 + Co]: dW over input-voxel chunk s of sample n (flattened input
// voxels [s Q, (s+1) Q), their 2 x 2 x 2 output taps) and db over output-voxel chunk s
// (flattened output voxels, output_padding included); S chunks per sample.
constexpr int kConvt3Chunk = 64;
__global__ __launch_bounds__(kBlock) void convt3d_wgrad_kernel(
    const float* __restrict__ dy, const float* __restrict__ x, float* __restrict__ partial,
    int Ci, int Di, int Hi, int Wi, int Co, int Do, int Ho, int Wo, int S) {
  const int s = blockIdx.x, n = blockIdx.y;
  const int EW = Ci * Co * 8, E = EW + Co;
  const int voli = Di * Hi * Wi;
  const int64_t volo = (int64_t)Do * Ho * Wo;
  const int q0 = s * kConvt3Chunk, q1 = min(voli, q0 + kConvt3Chunk);
  const int64_t o0 = (int64_t)s * volo / S, o1 = (int64_t)(s + 1) * volo / S;
  const float* xs = x + (int64_t)n * Ci * voli;
  const float* gs = dy + (int64_t)n * Co * volo;
  float* out = partial + ((int64_t)n * S + s) * E;
  for (int e = blockIdx.z * blockDim.x + threadIdx.x; e < E; e += gridDim.z * blockDim.x) {
    float acc = 0.f;
    if (e < EW) {
      const int t = e & 7, co = (e >> 3) % Co, ci = (e >> 3) / Co;
      const float* xp = xs + (int64_t)ci * voli;
      const float* gp = gs + (int64_t)co * volo + ((int64_t)(t >> 2) * Ho + ((t >> 1) & 1)) * Wo + (t & 1);
      for (int q = q0; q < q1; ++q) {
        const int wi = q % Wi, hi = (q / Wi) % Hi, di = q / (Wi * Hi);
        acc = fmaf(xp[q], gp[((int64_t)(2 * di) * Ho + 2 * hi) * Wo + 2 * wi], acc);
      }
    } else {
      const float* gp = gs + (int64_t)(e - EW) * volo;
      for (int64_t o = o0; o < o1; ++o) acc += gp[o];
    }
    out[e] = acc;
  }
}

inline int blocks_for(int64_t n) { return (int)((n + kBlock - 1) / kBlock); }

inline bool odd_le7(int k) { return k == 1 || k == 3 || k == 5 || k == 7; }

inline bool vol_ok(int N, int C, int D, int H, int W) {
  if (N < 1 || C < 1 || D < 1 || H < 1 || W < 1) return false;
  if ((int64_t)D * H * W >= INT32_MAX) return false;
  return (int64_t)N * C * D * H * W / kBlock < INT32_MAX;      // one thread per voxel fits a grid
}

inline bool dw_ok(int N, int C, int D, int H, int W, int KD, int KH, int KW) {
  if (!vol_ok(N, C, D, H, W) || !odd_le7(KD) || !odd_le7(KH) || !odd_le7(KW)) return false;
  const DwTiles nt = dw_tiles(D, H, W);
  const int64_t ntile = (int64_t)nt.ntd * nt.nth * nt.ntw;
  return ntile < INT32_MAX && (int64_t)N * C * ntile < INT32_MAX && C <= 65535;
}

template <bool FLIP>
int dw_launch(const float* x, const float* w, const float* b, float* y, int N, int C, int D, int H,
              int W, int KD, int KH, int KW, hipStream_t st) {
  const DwTiles nt = dw_tiles(D, H, W);
  const unsigned grid = (unsigned)((int64_t)N * C * nt.count());
  switch (KW) {
    case 1: dwconv3d_kernel<1, FLIP><<<grid, kBlock, 0, st>>>(x, w, b, y, C, D, H, W, KD, KH, nt); break;
    case 3: dwconv3d_kernel<3, FLIP><<<grid, kBlock, 0, st>>>(x, w, b, y, C, D, H, W, KD, KH, nt); break;
    case 5: dwconv3d_kernel<5, FLIP><<<grid, kBlock, 0, st>>>(x, w, b, y, C, D, H, W, KD, KH, nt); break;
    default: dwconv3d_kernel<7, FLIP><<<grid, kBlock, 0, st>>>(x, w, b, y, C, D, H, W, KD, KH, nt); break;
  }
  return (int)hipGetLastError();
}

inline bool pool_ok(int NC, int D, int H, int W, int KD, int KH, int KW) {
  return vol_ok(NC, 1, D, H, W) && KD >= 1 && KD <= 2 && KH >= 1 && KH <= 2 && KW >= 1 && KW <= 2 &&
         D >= KD && H >= KH && W >= KW;
}

inline bool convt_ok(int N, int Ci, int Di, int Hi, int Wi, int Co, int Do, int Ho, int Wo) {
  if (!vol_ok(N, Ci, Di, Hi, Wi) || Co < 1) return false;
  if (Do < 2 * Di || Do >= 2 * Di + 2 || Ho < 2 * Hi || Ho >= 2 * Hi + 2 || Wo < 2 * Wi || Wo >= 2 * Wi + 2)
    return false;
  return vol_ok(N, Co, Do, Ho, Wo) && (int64_t)Ci * Co * 8 + Co < INT32_MAX;
}

}  // namespace

// ============================================================================== C ABI

BLINDNO_API int blindno_dwconv3d_fwd(const float* x, const float* w, const float* b, float* y, int N,
                                     int C, int D, int H, int W, int KD, int KH, int KW,
                                     void* stream) {
  if (!x || !w || !y || !dw_ok(N, C, D, H, W, KD, KH, KW)) return (int)hipErrorInvalidValue;
  return dw_launch<false>(x, w, b, y, N, C, D, H, W, KD, KH, KW, (hipStream_t)stream);
}

BLINDNO_API int blindno_dwconv3d_bwd_data(const float* dy, const float* w, float* dx, int N, int C,
                                          int D, int H, int W, int KD, int KH, int KW,
                                          void* stream) {
  if (!dy || !w || !dx || !dw_ok(N, C, D, H, W, KD, KH, KW)) return (int)hipErrorInvalidValue;
  return dw_launch<true>(dy, w, nullptr, dx, N, C, D, H, W, KD, KH, KW, (hipStream_t)stream);
}

BLINDNO_API int blindno_dwconv3d_wgrad_nsplit(int N, int C, int D, int H, int W, int KD, int KH,
                                              int KW) {
  if (!dw_ok(N, C, D, H, W, KD, KH, KW)) return -1;
  // C KD workgroups per split; ~4 workgroups on each of the 256 CUs
  const int64_t items = (int64_t)N * dw_tiles(D, H, W).count();
  int64_t s = (1024 + (int64_t)C * KD - 1) / ((int64_t)C * KD);
  if (s > items) s = items;
  return (int)(s < 1 ? 1 : s);
}

BLINDNO_API int blindno_dwconv3d_bwd_weight(const float* dy, const float* x, float* dwb,
                                            float* partial, int nsplit, int N, int C, int D, int H,
                                            int W, int KD, int KH, int KW, void* stream) {
  if (!dy || !x || !dwb || !dw_ok(N, C, D, H, W, KD, KH, KW) || nsplit < 1 || nsplit > 65535 * 32 ||
      (nsplit > 1 && !partial))
    return (int)hipErrorInvalidValue;
  hipStream_t st = (hipStream_t)stream;
  float* dst = nsplit > 1 ? partial : dwb;
  const DwTiles nt = dw_tiles(D, H, W);
  const dim3 grid(nsplit, C, KD);
  switch (KW) {
    case 1: dwconv3d_wgrad_kernel<1><<<grid, kBlock, 0, st>>>(dy, x, dst, N, C, D, H, W, KD, KH, nt, nsplit); break;
    case 3: dwconv3d_wgrad_kernel<3><<<grid, kBlock, 0, st>>>(dy, x, dst, N, C, D, H, W, KD, KH, nt, nsplit); break;
    case 5: dwconv3d_wgrad_kernel<5><<<grid, kBlock, 0, st>>>(dy, x, dst, N, C, D, H, W, KD, KH, nt, nsplit); break;
    default: dwconv3d_wgrad_kernel<7><<<grid, kBlock, 0, st>>>(dy, x, dst, N, C, D, H, W, KD, KH, nt, nsplit); break;
  }
  const int err = (int)hipGetLastError();
  if (err || nsplit == 1) return err;
  return blindno_reduce_partials(partial, dwb, nsplit, C * (KD * KH * KW + 1), stream);
}

BLINDNO_API int blindno_maxpool3d_fwd(const float* x, float* y, uint8_t* arg, int NC, int D, int H,
                                      int W, int KD, int KH, int KW, void* stream) {
  if (!x || !y || !arg || !pool_ok(NC, D, H, W, KD, KH, KW)) return (int)hipErrorInvalidValue;
  const int Do = D / KD, Ho = H / KH, Wo = W / KW;
  const int64_t total = (int64_t)NC * Do * Ho * Wo;
  maxpool3d_fwd_kernel<<<blocks_for(total), kBlock, 0, (hipStream_t)stream>>>(x, y, arg, D, H, W, Do, Ho,
                                                                            Wo, KD, KH, KW, total);
  return (int)hipGetLastError();
}

BLINDNO_API int blindno_maxpool3d_bwd(const float* dy, const uint8_t* arg, float* dx, int NC, int D,
                                      int H, int W, int KD, int KH, int KW, void* stream) {
  if (!dy || !arg || !dx || !pool_ok(NC, D, H, W, KD, KH, KW)) return (int)hipErrorInvalidValue;
  const int Do = D / KD, Ho = H / KH, Wo = W / KW;
  const int64_t total = (int64_t)NC * D * H * W;
  maxpool3d_bwd_kernel<<<blocks_for(total), kBlock, 0, (hipStream_t)stream>>>(dy, arg, dx, D, H, W, Do,
                                                                            Ho, Wo, KD, KH, KW, total);
  return (int)hipGetLastError();
}

BLINDNO_API int blindno_convt3d_fwd(const float* x, const float* w, const float* b, float* y, int N,
                                    int Ci, int Di, int Hi, int Wi, int Co, int Do, int Ho, int Wo,
                                    void* stream) {
  if (!x || !w || !y || !convt_ok(N, Ci, Di, Hi, Wi, Co, Do, Ho, Wo)) return (int)hipErrorInvalidValue;
  const int64_t total = (int64_t)N * Co * Do * Ho * Wo;
  convt3d_fwd_kernel<<<blocks_for(total), kBlock, 0, (hipStream_t)stream>>>(x, w, b, y, Ci, Di, Hi, Wi, Co,
                                                                          Do, Ho, Wo, total);
  return (int)hipGetLastError();
}

BLINDNO_API int blindno_convt3d_bwd_data(const float* dy, const float* w, float* dx, int N, int Ci,
                                         int Di, int Hi, int Wi, int Co, int Do, int Ho, int Wo,
                                         void* stream) {
  if (!dy || !w || !dx || !convt_ok(N, Ci, Di, Hi, Wi, Co, Do, Ho, Wo)) return (int)hipErrorInvalidValue;
  const int64_t total = (int64_t)N * Ci * Di * Hi * Wi;
  convt3d_bwd_data_kernel<<<blocks_for(total), kBlock, 0, (hipStream_t)stream>>>(dy, w, dx, Ci, Di, Hi, Wi,
                                                                               Co, Do, Ho, Wo, total);
  return (int)hipGetLastError();
}

BLINDNO_API int blindno_convt3d_wgrad_nparts(int N, int Di, int Hi, int Wi) {
  if (!vol_ok(N, 1, Di, Hi, Wi)) return -1;
  return N * ((Di * Hi * Wi + kConvt3Chunk - 1) / kConvt3Chunk);
}

BLINDNO_API int blindno_convt3d_bwd_weight(const float* dy, const float* x, float* dwb,
                                           float* partial, int N, int Ci, int Di, int Hi, int Wi,
                                           int Co, int Do, int Ho, int Wo, void* stream) {
  if (!dy || !x || !dwb || !partial || !convt_ok(N, Ci, Di, Hi, Wi, Co, Do, Ho, Wo))
    return (int)hipErrorInvalidValue;
  const int E = Ci * Co * 8 + Co;
  const int S = (Di * Hi * Wi + kConvt3Chunk - 1) / kConvt3Chunk;
  if (N > 65535 || (int64_t)N * S >= INT32_MAX) return (int)hipErrorInvalidValue;
  int gz = (E + kBlock - 1) / kBlock;
  if (gz > 16) gz = 16;
  hipStream_t st = (hipStream_t)stream;
  convt3d_wgrad_kernel<<<dim3(S, N, gz), kBlock, 0, st>>>(dy, x, partial, Ci, Di, Hi, Wi, Co, Do, Ho, Wo, S);
  const int err = (int)hipGetLastError();
  if (err) return err;
  return blindno_reduce_partials(partial, dwb, N * S, E, stream);
}
