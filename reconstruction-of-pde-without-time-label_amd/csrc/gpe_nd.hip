// Grid-resident Gross-Pitaevskii split-step solver in two and three dimensions, the trapezoid
// density residuals (include/blindno_gpe2d.h, include/blindno_gpe3d.h), and the solver without its
// record, with the density-error integrals reduced on the device (include/blindno_gpe2d_err.h,
// include/blindno_gpe3d_err.h).  One core: the 2D and 3D entries at the end differ only in the
// list of passes they hand to it.
//
//   i psi_t = -1/2 lap psi + (V + g |psi|^2 + kappa |psi|^4) psi
// on a periodic nx x ny (x nz) grid (row-major, last axis contiguous, complex128 interleaved), the
// reference's 1D scheme (1d_GPE/datagen_GPE.py:29-115, csrc/evaluators.hip gpe_solve_kernel) with
// more axes:
//   N(h): psi <- exp(-i h (V + g|psi|^2 + kappa|psi|^4)) psi                     pointwise
//   L(h): psi <- ifftn(exp(-i h/2 |k|^2) fftn psi)                  k = 2 pi fftfreq(n, d) per axis
// Strang N(dt/2) L(dt) N(dt/2) or the nine-stage Yoshida sequence per step.
//
// gpe_solve_kernel keeps a trajectory in one workgroup's LDS (N <= 2048); a 256^2 complex128
// field is 1 MiB.  Here the field lives in global memory (the caller's scratch) and the kinetic
// phase is factorised, so L is one factor per axis and each factor is a batch of independent 1D
// transforms (FFT, multiply, inverse FFT, 1/n) along that axis.  All are one kernel template with
// two layouts:
//   ROW  a workgroup owns `tile` whole lines along the contiguous axis, a contiguous chunk of the
//        field: the 2D row pass (nx lines of ny) and the 3D z pass (nx ny lines of nz);
//   COL  a plane is n rows of `width` contiguous points and a workgroup owns `tile` >= 4 adjacent
//        columns of one plane over all n rows, each row of the tile a contiguous segment of
//        >= 64 B: the 2D column pass (one plane, nx rows of ny), the 3D y pass (nx planes, ny rows
//        of nz; a plane with nz < 1024/ny is taken whole) and the 3D x pass (one plane, nx rows of
//        ny nz).
// The tile sits in LDS exactly as it lies in global memory ([line][i] / [i][column]); the radix-2
// Stockham passes of gpe_solve_kernel run on all of the tile's transforms at once, lanes walking
// the contiguous index fastest, so every LDS and global access of a wave is a run of contiguous
// 16-B elements -- there is no transposed copy and hence no power-of-two stride between lanes
// that a padded stride would have to break.
//
// All pointwise work is fused into the first and the last pass of an L: what precedes the
// transforms (record 0 and the very first N, on the first ROW pass only) runs on the way into LDS,
// what follows them (the 1/n scale, N, the record, the next step's first N, the final field) on
// the last pass's way out.  One L is one launch per axis, so a Strang step is 2 (2D) or 3 (3D)
// launches and a Yoshida step 8 or 12; a call with no steps is one launch; the solver has no other
// kernel (the record-free error entries further down add two reduction kernels of their own).
// A pass updates the field in place: a workgroup reads its whole tile before it writes it, and
// tiles are disjoint.  The only ordering between passes is the launch boundary on the stream:
// no cooperative launch, no grid barrier, no flag another workgroup waits on, no float
// accumulation across workgroups and no memory location that two workgroups of a launch both
// touch.  A tile never spans two trajectories and the arithmetic of a point does not depend on
// the thread that runs it, so results are bit-deterministic and independent of B.
//
// LDS: two ping-pong buffers of n * tile points plus n/2 twiddles and n phase factors, 16 B
// each.  tile * n = 1024 points where the geometry allows, one butterfly per thread of a
// 512-thread workgroup: 32.8 KiB at n = 32, 33.5 KiB at n = 64, 38 KiB at n = 256 (four
// workgroups per CU), 56 KiB at n = 1024.  A COL tile keeps at least 4 columns, so it holds 2048
// points (76 KiB) at n = 512 and 4096 points (152 KiB of the CU's 160 KiB) at n = 1024, which is
// what bounds BLINDNO_GPE2D_MAX_N and BLINDNO_GPE3D_MAX_N.
// Every offset is 64-bit.  fp64 throughout; contraction is off so a complex product rounds like
// numpy's.
#include "common.h"
#include "blindno.h"

#pragma clang fp contract(off)

namespace {

struct __attribute__((aligned(16))) cd {
  double re, im;
};

__device__ __forceinline__ cd cmul(cd a, cd b) {
  return {a.re * b.re - a.im * b.im, a.re * b.im + a.im * b.re};
}

constexpr int kMinN = BLINDNO_GPE3D_MIN_N, kMaxN = BLINDNO_GPE3D_MAX_N;
static_assert(BLINDNO_GPE2D_MIN_N == kMinN && BLINDNO_GPE2D_MAX_N == kMaxN, "one range for every axis");
constexpr int64_t kMaxCells = BLINDNO_GPE3D_MAX_CELLS;
constexpr int kTilePoints = 1024;        // points of a workgroup's tile (per ping-pong buffer)
constexpr int kMinCols = 4;              // COL tile: 4 x 16 B = 64-B row segments at least
constexpr int kMaxThreads = 512;

struct PassArgs {
  const double* src;      // field read: psi0 on the first launch, the scratch field afterwards
  int64_t src_bstride;    // doubles per trajectory of src (0: one psi0 shared by the batch)
  double* field;          // (B, cells, 2) scratch field written
  const double* V;        // (B, cells)
  const double* g;        // (B)
  const double* kappa;    // (B)
  double* rec_abs64;      // (B, nrec, cells) or NULL
  float* rec_abs32;       // the same in fp32 or NULL
  double* rec_psi;        // (B, nrec, cells, 2) or NULL
  double* psi_out;        // (B, cells, 2), written when write_out
  int64_t cells;          // points of a trajectory
  int64_t plane_stride;   // COL: points between two planes
  int64_t row_stride;     // COL: points between two rows of a tile (the plane's width)
  int lg_tiles_pp;        // log2 of the tiles per plane (ROW: one plane)
  int tiles, lg_tiles;    // tiles per trajectory = planes * tiles per plane, a power of two
  int nrec;
  int tile, lg_tile;      // lines / columns per workgroup
  int lg_n;               // log2 of the transform length
  int do_lin;             // 0: no transform (nsteps = 0: record and copy only)
  double lin_h;           // L(lin_h) along this axis
  double d;               // grid spacing along this axis
  int rec_pre;            // record index written before anything else, or -1
  int has_pre;            // N(h_pre) before the transform
  double h_pre;
  int has_post1;          // after the transform: N(h_post1), record rec_post, N(h_post2)
  double h_post1;
  int rec_post;
  int has_post2;
  double h_post2;
  int write_out;
};

// psi <- exp(-i h (V + g|psi|^2 + kappa|psi|^4)) psi   (step_nonlinear, datagen_GPE.py:37-42)
__device__ __forceinline__ cd nonlinear(cd p, double V, double g, double kappa, double h) {
  const double a2 = p.re * p.re + p.im * p.im;
  const double A = V + g * a2 + kappa * (a2 * a2);
  double s, c;
  sincos(-h * A, &s, &c);
  return cmul({c, s}, p);
}

// One radix-2 Stockham pass (fft_pass of evaluators.hip) over the tile's `cnt` transforms of
// length n at once.  Point i of transform q sits at q*n + i (ROW layout) or i*cnt + q (COL
// layout); butterfly t takes the contiguous index from its low bits.  With `lin` the inputs are
// multiplied by the phase table first (the kinetic factor, folded into the first inverse pass).
template <bool COL, bool INV>
__device__ __forceinline__ void fft_pass(const cd* __restrict__ src, cd* __restrict__ dst,
                                         const cd* __restrict__ tw, const cd* __restrict__ lin,
                                         int lg_n, int lg_cnt, int Ns) {
  const int n = 1 << lg_n, half = n >> 1, cnt = 1 << lg_cnt;
  const int tstride = half / Ns;
  const int total = half << lg_cnt;
  for (int t = threadIdx.x; t < total; t += blockDim.x) {
    int j, q;
    if (COL) {
      q = t & (cnt - 1);
      j = t >> lg_cnt;
    } else {
      j = t & (half - 1);
      q = t >> (lg_n - 1);
    }
    const int base = COL ? q : q << lg_n;
    const int es = COL ? cnt : 1;
    const int k = j & (Ns - 1);
    cd w = tw[k * tstride];
    if (INV) w.im = -w.im;
    cd a0 = src[base + j * es];
    cd a1 = src[base + (j + half) * es];
    if (lin) {
      a0 = cmul(a0, lin[j]);
      a1 = cmul(a1, lin[j + half]);
    }
    a1 = cmul(a1, w);
    const int d = ((j - k) << 1) + k;
    dst[base + d * es] = {a0.re + a1.re, a0.im + a1.im};
    dst[base + (d + Ns) * es] = {a0.re - a1.re, a0.im - a1.im};
  }
}

template <bool COL>
__global__ __launch_bounds__(kMaxThreads) void gpe_pass_kernel(const PassArgs a) {
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  const int n = 1 << a.lg_n, cnt = a.tile;
  const int points = n << a.lg_tile;
  cd* buf0 = reinterpret_cast<cd*>(smem_raw);
  cd* buf1 = buf0 + points;
  cd* tw = buf1 + points;     // n/2
  cd* lin = tw + (n >> 1);    // n
  // every count is a power of two: the set-up of a workgroup has no division
  const int b = (int)blockIdx.x >> a.lg_tiles;
  const int r = (int)blockIdx.x & (a.tiles - 1);        // tile of the trajectory
  const int plane = r >> a.lg_tiles_pp;
  const int t0 = (r & ((1 << a.lg_tiles_pp) - 1)) << a.lg_tile;   // first line / column of the tile
  const int64_t N = a.cells;
  const double g = a.g[b], kappa = a.kappa[b];
  const double* Vb = a.V + (int64_t)b * N;
  // first point of the tile inside the trajectory (ROW: plane = 0 and t0 counts lines)
  const int64_t origin = COL ? (int64_t)plane * a.plane_stride + t0 : (int64_t)t0 << a.lg_n;
  // global point of LDS point e, inside the trajectory
  auto gidx = [&](int e) -> int64_t {
    return COL ? origin + (int64_t)(e >> a.lg_tile) * a.row_stride + (e & (cnt - 1)) : origin + e;
  };
  auto record = [&](cd p, int rec, int64_t gi) {
    const int64_t o = ((int64_t)b * a.nrec + rec) * N + gi;
    if (a.rec_abs64) a.rec_abs64[o] = hypot(p.re, p.im);
    if (a.rec_abs32) a.rec_abs32[o] = (float)hypot(p.re, p.im);
    if (a.rec_psi) *reinterpret_cast<cd*>(a.rec_psi + 2 * o) = p;
  };

  if (a.do_lin) {
    for (int i = threadIdx.x; i < (n >> 1); i += blockDim.x) {
      double s, c;
      sincospi(2.0 * (double)i / (double)n, &s, &c);
      tw[i] = {c, -s};
    }
    // k = 2 pi fftfreq(n, d): j / (n d) for j < (n+1)/2, else (j - n) / (n d)
    const double val = 1.0 / ((double)n * a.d);
    for (int i = threadIdx.x; i < n; i += blockDim.x) {
      const int f = i < (n + 1) / 2 ? i : i - n;
      const double k = 6.283185307179586 * ((double)f * val);
      double s, c;
      sincos((-a.lin_h * 0.5) * (k * k), &s, &c);
      lin[i] = {c, s};
    }
  }
  const double* src = a.src + (int64_t)b * a.src_bstride;
  for (int e = threadIdx.x; e < points; e += blockDim.x) {
    const int64_t gi = gidx(e);
    cd p = *reinterpret_cast<const cd*>(src + 2 * gi);
    if (a.rec_pre >= 0) record(p, a.rec_pre, gi);
    if (a.has_pre) p = nonlinear(p, Vb[gi], g, kappa, a.h_pre);
    buf0[e] = p;
  }
  __syncthreads();

  cd* bufs[2] = {buf0, buf1};
  int cur = 0;
  double scale = 1.0;
  if (a.do_lin) {
    for (int Ns = 1; Ns < n; Ns <<= 1) {
      fft_pass<COL, false>(bufs[cur], bufs[cur ^ 1], tw, nullptr, a.lg_n, a.lg_tile, Ns);
      cur ^= 1;
      __syncthreads();
    }
    for (int Ns = 1; Ns < n; Ns <<= 1) {
      fft_pass<COL, true>(bufs[cur], bufs[cur ^ 1], tw, Ns == 1 ? lin : nullptr, a.lg_n,
                          a.lg_tile, Ns);
      cur ^= 1;
      __syncthreads();
    }
    scale = 1.0 / (double)n;   // numpy.fft.ifft's normalisation; a power of two, so exact
  }
  const cd* res = bufs[cur];
  double* fb = a.field + 2 * (int64_t)b * N;
  double* ob = a.write_out ? a.psi_out + 2 * (int64_t)b * N : nullptr;
  for (int e = threadIdx.x; e < points; e += blockDim.x) {
    const int64_t gi = gidx(e);
    cd p = res[e];
    p.re = p.re * scale;
    p.im = p.im * scale;
    if (a.has_post1 || a.has_post2) {
      const double v = Vb[gi];
      if (a.has_post1) p = nonlinear(p, v, g, kappa, a.h_post1);
      if (a.rec_post >= 0) record(p, a.rec_post, gi);
      if (a.has_post2) p = nonlinear(p, v, g, kappa, a.h_post2);
    } else if (a.rec_post >= 0) {
      record(p, a.rec_post, gi);
    }
    *reinterpret_cast<cd*>(fb + 2 * gi) = p;
    if (a.write_out) *reinterpret_cast<cd*>(ob + 2 * gi) = p;
  }
}

// trapezoid weight of point i of a grid: half the sum of the two adjacent spacings (one at an end)
__device__ __forceinline__ double trapz_w(const double* __restrict__ x, int i, int n) {
  return 0.5 * ((i > 0 ? x[i] - x[i - 1] : 0.0) + (i < n - 1 ? x[i + 1] - x[i] : 0.0));
}

// out[2f] = trapz over every axis of (a_f - b_f)^2, out[2f+1] the same of b_f^2, as the weighted
// sum over the frame's points with the weights wx(ix) wy(iy) [wz(iz)]; w = wx wy in 2D and
// (wx wy) wz in 3D, which is what the bits depend on.  The entries have no scratch argument and
// allocate nothing, so a frame is one workgroup and the reduction has two stages inside it, both
// in a fixed order: each thread sums its points e = tid, tid + BLOCK, ... in ascending order, then
// a binary tree over the BLOCK partial sums in LDS.  BLOCK fixes the order of the sum (256 in 2D,
// 512 in 3D).  The grids need not be powers of two: indices by division.  DIM == 2: z unused.
template <int DIM, int BLOCK>
__global__ __launch_bounds__(BLOCK) void trapz_frames_kernel(
    const double* __restrict__ a, const double* __restrict__ b, const double* __restrict__ x,
    const double* __restrict__ y, const double* __restrict__ z, double* __restrict__ out, int nx,
    int ny, int nz) {
  __shared__ double ra[BLOCK], rb[BLOCK];
  const int64_t plane = DIM == 3 ? (int64_t)ny * nz : ny;
  const int64_t N = (int64_t)nx * plane;
  const double* ap = a + (int64_t)blockIdx.x * N;
  const double* bp = b + (int64_t)blockIdx.x * N;
  double sa = 0.0, sb = 0.0;
  for (int64_t e = threadIdx.x; e < N; e += BLOCK) {
    const int ix = (int)(e / plane);
    const int64_t r = e - (int64_t)ix * plane;
    double w;
    if constexpr (DIM == 3) {
      const int iy = (int)(r / nz), iz = (int)(r - (int64_t)iy * nz);
      w = (trapz_w(x, ix, nx) * trapz_w(y, iy, ny)) * trapz_w(z, iz, nz);
    } else {
      w = trapz_w(x, ix, nx) * trapz_w(y, (int)r, ny);
    }
    const double bv = bp[e], d = ap[e] - bv;
    sa += w * (d * d);
    sb += w * (bv * bv);
  }
  ra[threadIdx.x] = sa;
  rb[threadIdx.x] = sb;
  __syncthreads();
  for (int s = BLOCK / 2; s > 0; s >>= 1) {
    if (threadIdx.x < s) {
      ra[threadIdx.x] += ra[threadIdx.x + s];
      rb[threadIdx.x] += rb[threadIdx.x + s];
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    out[2 * (int64_t)blockIdx.x] = ra[0];
    out[2 * (int64_t)blockIdx.x + 1] = rb[0];
  }
}

// ---- blindno_gpe2d_error / blindno_gpe3d_error: the solver with its record reduced away.
//
// An error evaluation wants two numbers per trajectory and recorded step, the trapezoid integrals
// of (|psi| - |psi_ref|)^2 and |psi_ref|^2, not the frames.  The pass kernel above is driven by the
// same launch sequence as the solve entries (enqueue below); its |psi| record is pointed at one
// frame per trajectory in scratch (nrec = 1, record index 0), and after each launch that wrote the
// frame two small launches reduce it:
//   stage one  one workgroup of 256 threads per (trajectory, tile of TILE consecutive cells):
//              thread t adds the terms of cells t, t + 256, ... of the tile in ascending order (a
//              wave's loads are one contiguous 512-B run each), the wave sums by a fixed shuffle
//              tree (offsets 32, 16 .. 1), lane 0 of the four waves meet in LDS and thread 0 adds
//              them in wave order -> partial (B, tiles, 2)
//   stage two  one workgroup per trajectory: thread t adds tiles t, t + 256, ... in ascending
//              order, then the same tree -> err[b, r, :]
// The per-cell terms are trapz_frames_kernel's to the bit (the same w, d = a - b, w (d d) and
// w (b b); contraction is off for the whole file); only the order of the sum differs.  Every
// addition has a fixed place, so a second call repeats the bits; a workgroup reads only its own
// trajectory's frame and its reference's and writes only its own two partials, so the rest of the
// batch cannot change a group's numbers.  The frame cannot be replaced by reading the field after
// the last pass: that pass has already applied the next step's first N (has_post2).
constexpr int kErrBlock = 256;
template <int DIM>
constexpr int kErrTile = DIM == 2 ? BLINDNO_GPE2D_ERR_TILE : BLINDNO_GPE3D_ERR_TILE;
template <int TILE>
constexpr bool kErrTileOk = TILE >= 256 && TILE <= 4096 && (TILE & (TILE - 1)) == 0 && TILE % kErrBlock == 0;
static_assert(kErrTileOk<kErrTile<2>>, "BLINDNO_GPE2D_ERR_TILE: a power of two in [256, 4096]");
static_assert(kErrTileOk<kErrTile<3>>, "BLINDNO_GPE3D_ERR_TILE: a power of two in [256, 4096]");

// sum over the workgroup of (a, b), valid in thread 0; `red` is 2 x 4 doubles of LDS
__device__ __forceinline__ void err_block_sum2(double& a, double& b, double (*red)[kErrBlock / 64]) {
  for (int off = 32; off > 0; off >>= 1) {
    a += __shfl_down(a, off, 64);
    b += __shfl_down(b, off, 64);
  }
  const int wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) {
    red[0][wave] = a;
    red[1][wave] = b;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    a = red[0][0];
    b = red[1][0];
    for (int w = 1; w < kErrBlock / 64; ++w) {
      a += red[0][w];
      b += red[1][w];
    }
  }
}

// frame (B, N): |psi| of every trajectory at one recorded step; ny and nz are powers of two
// (DIM == 2: z unused, nz = 1 and lg_nz = 0)
template <int DIM, int TILE>
__global__ __launch_bounds__(kErrBlock) void gpe_err_tile_kernel(
    const double* __restrict__ frame, const double* __restrict__ x, const double* __restrict__ y,
    const double* __restrict__ z, double* __restrict__ partial, int64_t N, int tiles, int group,
    int nx, int ny, int nz, int lg_ny, int lg_nz) {
  __shared__ double red[2][kErrBlock / 64];
  const int b = (int)blockIdx.x / tiles;
  const int tile = (int)blockIdx.x - b * tiles;
  const double* ap = frame + (int64_t)b * N;
  const double* bp = frame + (int64_t)(b / group * group) * N;
  double sa = 0.0, sb = 0.0;
  for (int k = 0; k < TILE / kErrBlock; ++k) {
    const int64_t e = (int64_t)tile * TILE + k * kErrBlock + (int)threadIdx.x;
    if (e < N) {                                 // N may be smaller than one tile
      const int iy = (int)((e >> lg_nz) & (ny - 1));
      const int ix = (int)(e >> (lg_nz + lg_ny));
      double w = trapz_w(x, ix, nx) * trapz_w(y, iy, ny);
      if constexpr (DIM == 3) w = w * trapz_w(z, (int)(e & (nz - 1)), nz);
      const double bv = bp[e], d = ap[e] - bv;
      sa += w * (d * d);
      sb += w * (bv * bv);
    }
  }
  err_block_sum2(sa, sb, red);
  if (threadIdx.x == 0) {
    partial[2 * (int64_t)blockIdx.x] = sa;
    partial[2 * (int64_t)blockIdx.x + 1] = sb;
  }
}

__global__ __launch_bounds__(kErrBlock) void gpe_err_sum_kernel(const double* __restrict__ partial,
                                                                double* __restrict__ err, int tiles,
                                                                int nrec, int r) {
  __shared__ double red[2][kErrBlock / 64];
  const int b = blockIdx.x;
  const double* pt = partial + 2 * (int64_t)b * tiles;
  double sa = 0.0, sb = 0.0;
  for (int t = threadIdx.x; t < tiles; t += kErrBlock) {
    sa += pt[2 * (int64_t)t];
    sb += pt[2 * (int64_t)t + 1];
  }
  err_block_sum2(sa, sb, red);
  if (threadIdx.x == 0) {
    double* e = err + 2 * ((int64_t)b * nrec + r);
    e[0] = sa;
    e[1] = sb;
  }
}

int ilog2(int64_t v) {
  int l = 0;
  while (((int64_t)1 << l) < v) ++l;
  return l;
}

bool pow2_in_range(int v) { return v >= kMinN && v <= kMaxN && (v & (v - 1)) == 0; }

int64_t min_i64(int64_t a, int64_t b) { return a < b ? a : b; }
int64_t max_i64(int64_t a, int64_t b) { return a > b ? a : b; }

bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

// The geometry of a pass; everything else in PassArgs is zero.  One tile rule per layout (all
// sizes powers of two):
//   ROW  tile = max(1, min(lines, 1024 / n))
//   COL  tile = max(4, min(width, 1024 / n))
//   pass            layout  lines / planes, n, width   tile
//   2D row          ROW     nx lines of ny             max(1, min(nx, 1024 / ny))
//   2D column       COL     1 plane, nx, ny            max(4, min(ny, 1024 / nx))
//   3D z            ROW     nx ny lines of nz          max(1, min(nx ny, 1024 / nz))
//   3D y            COL     nx planes, ny, nz          max(4, min(nz, 1024 / ny))
//   3D x            COL     1 plane, nx, ny nz         max(4, min(ny nz, 1024 / nx))
PassArgs row_pass(int64_t lines, int n) {
  PassArgs p = {};
  p.tile = (int)max_i64(1, min_i64(lines, kTilePoints / n));
  p.lg_tile = ilog2(p.tile);
  p.lg_n = ilog2(n);
  p.tiles = (int)(lines / p.tile);
  p.lg_tiles_pp = p.lg_tiles = ilog2(p.tiles);
  return p;
}

PassArgs col_pass(int planes, int n, int64_t width) {
  PassArgs p = {};
  p.tile = (int)max_i64(kMinCols, min_i64(width, kTilePoints / n));
  p.lg_tile = ilog2(p.tile);
  p.lg_n = ilog2(n);
  p.plane_stride = n * width;
  p.row_stride = width;
  p.tiles = planes * (int)(width / p.tile);
  p.lg_tiles_pp = ilog2(width / p.tile);
  p.lg_tiles = ilog2(p.tiles);
  return p;
}

// A grid and its passes in launch order: the first is ROW and reads psi0, the last carries the
// post work; the transform axes are (y, x) in 2D and (z, y, x) in 3D.
struct Geometry {
  int dim, nx, ny, nz;          // nz = 1 in 2D
  int64_t cells;
  PassArgs pass[3];
};

// false for a grid the entries refuse.  BLINDNO_GPE3D_MAX_CELLS bounds the 3D grid only: the 2D
// header sets no such limit (1024^2 is its largest grid).
bool geometry(int dim, int B, int nx, int ny, int nz, Geometry* G) {
  if (B <= 0 || !pow2_in_range(nx) || !pow2_in_range(ny) || (dim == 3 && !pow2_in_range(nz))) return false;
  if (dim == 2) nz = 1;
  *G = {dim, nx, ny, nz, (int64_t)nx * ny * nz, {}};
  if (dim == 3 && G->cells > kMaxCells) return false;
  if (dim == 2) {
    G->pass[0] = row_pass(nx, ny);
    G->pass[1] = col_pass(1, nx, ny);
  } else {
    G->pass[0] = row_pass((int64_t)nx * ny, nz);
    G->pass[1] = col_pass(nx, ny, nz);
    G->pass[2] = col_pass(1, nx, (int64_t)ny * nz);
  }
  // a launch's workgroup count must fit the grid's x dimension
  for (int i = 0; i < dim; ++i)
    if ((int64_t)B * G->pass[i].tiles > 0x7fffffff) return false;
  return true;
}

template <bool COL>
hipError_t launch_pass(const PassArgs& a, int B, hipStream_t st) {
  const int n = 1 << a.lg_n;
  const int points = n << a.lg_tile;
  const size_t sh = sizeof(cd) * (2 * (size_t)points + n / 2 + n);
  if (sh > 64 * 1024) {
    // more dynamic LDS than the default cap; a refusal surfaces as the launch's own error
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&gpe_pass_kernel<COL>),
                              hipFuncAttributeMaxDynamicSharedMemorySize, (int)sh);
    (void)hipGetLastError();
  }
  const int threads = (int)max_i64(64, min_i64(kMaxThreads, points / 2));
  gpe_pass_kernel<COL><<<(unsigned)((int64_t)B * a.tiles), threads, sh, st>>>(a);
  return hipGetLastError();
}

// The arguments that the solve and error entries of both dimensions share.
struct Solve {
  const double *psi0, *V, *g, *kappa;
  double dt;
  int nsteps, order, rec_every;
  void* rec_abs;
  int rec_abs_f32;
  double *rec_psi, *psi_out, *scratch;
  int B, psi0_batched;
  void* stream;
};

// What the error entries add to the launch sequence: the frame that takes the record's place and
// the reduction enqueued after every launch that wrote it.
struct ErrPlan {
  const double *x, *y, *z;
  double* frame;      // (B, N) |psi| of the step being reduced
  double* partial;    // (B, tiles, 2)
  double* err;        // (B, nrec, 2)
  int tiles, group;
};

int64_t err_tiles(const Geometry& G) {
  const int tile = G.dim == 2 ? kErrTile<2> : kErrTile<3>;
  return (G.cells + tile - 1) / tile;
}

// The launch sequence of the solve entries on the passes of G (their spacings `d` set by the
// caller).  With `E` (the error entries) the only differences are where the pass kernel records
// -- E->frame as a one-frame fp64 record, index 0 at every record step -- and the two reduction
// launches after each launch that recorded.
int enqueue(const Solve& s, Geometry& G, const ErrPlan* E) {
  if (s.nsteps < 0 || s.rec_every < 1 || (s.order != 2 && s.order != 4) || !s.psi0 || !s.V || !s.g ||
      !s.kappa || !s.scratch || (s.rec_abs_f32 != 0 && s.rec_abs_f32 != 1) || !aligned16(s.psi0) ||
      !aligned16(s.scratch) || !aligned16(s.rec_psi) || !aligned16(s.psi_out))
    return (int)hipErrorInvalidValue;
  hipStream_t st = (hipStream_t)s.stream;
  const int B = s.B, nsteps = s.nsteps, np = G.dim;
  const int64_t N = G.cells;
  const int nrec = nsteps / s.rec_every + 1;
  for (int i = 0; i < np; ++i) {
    PassArgs& p = G.pass[i];
    p.src = s.scratch;
    p.src_bstride = 2 * N;
    p.field = s.scratch;
    p.V = s.V;
    p.g = s.g;
    p.kappa = s.kappa;
    p.rec_abs64 = E ? E->frame : s.rec_abs_f32 ? nullptr : (double*)s.rec_abs;
    p.rec_abs32 = !E && s.rec_abs_f32 ? (float*)s.rec_abs : nullptr;
    p.rec_psi = s.rec_psi;
    p.psi_out = s.psi_out;
    p.cells = N;
    p.nrec = E ? 1 : nrec;
    p.rec_pre = p.rec_post = -1;
  }
  // record r has just been written to E->frame by the launch before: reduce it into err[:, r, :]
  auto reduce = [&](int r) -> hipError_t {
    const unsigned wgs = (unsigned)((int64_t)B * E->tiles);
    const int lg_ny = ilog2(G.ny), lg_nz = ilog2(G.nz);
    if (G.dim == 2)
      gpe_err_tile_kernel<2, kErrTile<2>><<<wgs, kErrBlock, 0, st>>>(
          E->frame, E->x, E->y, E->z, E->partial, N, E->tiles, E->group, G.nx, G.ny, G.nz, lg_ny, lg_nz);
    else
      gpe_err_tile_kernel<3, kErrTile<3>><<<wgs, kErrBlock, 0, st>>>(
          E->frame, E->x, E->y, E->z, E->partial, N, E->tiles, E->group, G.nx, G.ny, G.nz, lg_ny, lg_nz);
    gpe_err_sum_kernel<<<B, kErrBlock, 0, st>>>(E->partial, E->err, E->tiles, nrec, r);
    return hipGetLastError();
  };
  PassArgs& first = G.pass[0];
  PassArgs& last = G.pass[np - 1];
  first.src = s.psi0;                    // the first launch reads psi0 and records step 0
  first.src_bstride = s.psi0_batched ? 2 * N : 0;
  first.rec_pre = 0;

  if (nsteps == 0) {
    first.do_lin = 0;
    first.write_out = s.psi_out != nullptr;
    hipError_t e = launch_pass<false>(first, B, st);
    if (e == hipSuccess && E) e = reduce(0);
    return (int)e;
  }
  // Yoshida coefficients as the reference forms them (2**(1/3) = pow(2, 1/3))
  const double dt = s.dt;
  const double cr = pow(2.0, 1.0 / 3.0);
  const double c2 = 2.0 - cr;
  const double a1 = 1.0 / c2, a2 = -cr / c2;
  // per step: N(hn[0]) L(hl[0]) N(hn[1]) ... L(hl[nl-1]) N(hn[nl])
  const int nl = s.order == 2 ? 1 : 4;
  const double hn2[2] = {dt / 2, dt / 2}, hl2[1] = {dt};
  const double hn4[5] = {a1 * dt, a2 * dt, a1 * dt, a2 * dt, a1 * dt};
  const double hl4[4] = {a1 * dt, a2 * dt, a2 * dt, a1 * dt};
  const double* hn = s.order == 2 ? hn2 : hn4;
  const double* hl = s.order == 2 ? hl2 : hl4;
  first.has_pre = 1;                     // the first step's first N; later ones ride on the
  first.h_pre = hn[0];                   // previous step's last pass (has_post2)
  for (int i = 0; i < np; ++i) G.pass[i].do_lin = 1;
  for (int n = 1; n <= nsteps; ++n) {
    for (int l = 0; l < nl; ++l) {
      for (int i = 0; i < np; ++i) G.pass[i].lin_h = hl[l];
      hipError_t e = launch_pass<false>(first, B, st);
      if (e != hipSuccess) return (int)e;
      if (E && first.rec_pre >= 0 && (e = reduce(0)) != hipSuccess) return (int)e;
      first.src = s.scratch;
      first.src_bstride = 2 * N;
      first.rec_pre = -1;
      first.has_pre = 0;
      for (int i = 1; i < np - 1; ++i)
        if ((e = launch_pass<true>(G.pass[i], B, st)) != hipSuccess) return (int)e;
      const bool final_l = l == nl - 1;
      last.has_post1 = 1;
      last.h_post1 = hn[l + 1];
      const int rec = final_l && n % s.rec_every == 0 ? n / s.rec_every : -1;
      last.rec_post = rec >= 0 && E ? 0 : rec;
      last.has_post2 = final_l && n < nsteps;
      last.h_post2 = hn[0];
      last.write_out = final_l && n == nsteps && s.psi_out != nullptr;
      e = launch_pass<true>(last, B, st);
      if (e != hipSuccess) return (int)e;
      if (E && rec >= 0 && (e = reduce(rec)) != hipSuccess) return (int)e;
    }
  }
  return (int)hipSuccess;
}

// blindno_gpe2d_solve / blindno_gpe3d_solve (E = NULL) and the integrator of the error entries.
// dz and nz are ignored in 2D.
int solve(int dim, const Solve& s, double dx, double dy, double dz, int nx, int ny, int nz, const ErrPlan* E) {
  Geometry G;
  if (!geometry(dim, s.B, nx, ny, nz, &G) || !(dx > 0.0) || !(dy > 0.0) || (dim == 3 && !(dz > 0.0)))
    return (int)hipErrorInvalidValue;
  // 3D only, kept as it is: the largest byte offset formed is 16 B nrec N (the psi record), and it
  // must fit 63 bits.  The 2D entry has no such check.
  if (dim == 3 && s.nsteps >= 0 && s.rec_every >= 1 && (s.rec_abs || s.rec_psi) &&
      (double)s.B * (double)(s.nsteps / s.rec_every + 1) * (double)G.cells * 16.0 >= 9.0e18)
    return (int)hipErrorInvalidValue;
  const double d[3] = {dx, dy, dz};
  for (int i = 0; i < dim; ++i) G.pass[i].d = d[dim - 1 - i];
  return enqueue(s, G, E);
}

int64_t scratch_doubles(int dim, int B, int nx, int ny, int nz, bool error) {
  Geometry G;
  if (!geometry(dim, B, nx, ny, nz, &G)) return -1;
  if (!error) return 2 * (int64_t)B * G.cells;
  return 3 * (int64_t)B * G.cells + 2 * (int64_t)B * err_tiles(G);   // field, frame, tile partials
}

int64_t launches(int dim, int nsteps, int order) {
  if (nsteps < 0 || (order != 2 && order != 4)) return -1;
  return nsteps == 0 ? 1 : (int64_t)nsteps * (order == 2 ? dim : 4 * dim);
}

int64_t error_launches(int dim, int nsteps, int order, int rec_every) {
  const int64_t n = launches(dim, nsteps, order);
  if (n < 0 || rec_every < 1) return -1;
  return n + 2 * ((int64_t)(nsteps / rec_every) + 1);
}

// blindno_gpe2d_error / blindno_gpe3d_error; `s` comes without record and output.  z is ignored in
// 2D.  The alignment of scratch, which the 2D entry used to test here as well, is refused by
// enqueue for both dimensions.
int solve_error(int dim, const Solve& s, const double* x, const double* y, const double* z, double dx, double dy,
          double dz, int group, double* err, int nx, int ny, int nz) {
  Geometry G;
  if (!geometry(dim, s.B, nx, ny, nz, &G) || group < 1 || s.B % group != 0 || !x || !y || (dim == 3 && !z) ||
      !err || !s.scratch)
    return (int)hipErrorInvalidValue;
  const int64_t BN = (int64_t)s.B * G.cells;
  ErrPlan E;
  E.x = x;
  E.y = y;
  E.z = z;
  E.frame = s.scratch + 2 * BN;                // after the working field
  E.partial = s.scratch + 3 * BN;
  E.err = err;
  // tiles <= the first pass's workgroups per trajectory, so B * tiles fits the grid as its launch does
  E.tiles = (int)err_tiles(G);
  E.group = group;
  return solve(dim, s, dx, dy, dz, nx, ny, nz, &E);
}

}  // namespace

BLINDNO_API int64_t blindno_gpe2d_scratch_doubles(int B, int nx, int ny) {
  return scratch_doubles(2, B, nx, ny, 1, false);
}

BLINDNO_API int64_t blindno_gpe3d_scratch_doubles(int B, int nx, int ny, int nz) {
  return scratch_doubles(3, B, nx, ny, nz, false);
}

BLINDNO_API int64_t blindno_gpe2d_error_scratch_doubles(int B, int nx, int ny) {
  return scratch_doubles(2, B, nx, ny, 1, true);
}

BLINDNO_API int64_t blindno_gpe3d_error_scratch_doubles(int B, int nx, int ny, int nz) {
  return scratch_doubles(3, B, nx, ny, nz, true);
}

BLINDNO_API int64_t blindno_gpe2d_launches(int nsteps, int order) { return launches(2, nsteps, order); }

BLINDNO_API int64_t blindno_gpe3d_launches(int nsteps, int order) { return launches(3, nsteps, order); }

BLINDNO_API int64_t blindno_gpe2d_error_launches(int nsteps, int order, int rec_every) {
  return error_launches(2, nsteps, order, rec_every);
}

BLINDNO_API int64_t blindno_gpe3d_error_launches(int nsteps, int order, int rec_every) {
  return error_launches(3, nsteps, order, rec_every);
}

BLINDNO_API int blindno_gpe2d_solve(const double* psi0, const double* V, const double* g,
                                    const double* kappa, double dx, double dy, double dt, int nsteps,
                                    int order, int rec_every, void* rec_abs, int rec_abs_f32,
                                    double* rec_psi, double* psi_out, double* scratch, int B, int nx,
                                    int ny, int psi0_batched, void* stream) {
  const Solve s = {psi0, V, g, kappa, dt, nsteps, order, rec_every, rec_abs, rec_abs_f32, rec_psi,
                   psi_out, scratch, B, psi0_batched, stream};
  return solve(2, s, dx, dy, 0.0, nx, ny, 1, nullptr);
}

BLINDNO_API int blindno_gpe3d_solve(const double* psi0, const double* V, const double* g,
                                    const double* kappa, double dx, double dy, double dz, double dt,
                                    int nsteps, int order, int rec_every, void* rec_abs,
                                    int rec_abs_f32, double* rec_psi, double* psi_out, double* scratch,
                                    int B, int nx, int ny, int nz, int psi0_batched, void* stream) {
  const Solve s = {psi0, V, g, kappa, dt, nsteps, order, rec_every, rec_abs, rec_abs_f32, rec_psi,
                   psi_out, scratch, B, psi0_batched, stream};
  return solve(3, s, dx, dy, dz, nx, ny, nz, nullptr);
}

BLINDNO_API int blindno_gpe2d_error(const double* psi0, const double* V, const double* g,
                                    const double* kappa, const double* x, const double* y, double dx,
                                    double dy, double dt, int nsteps, int order, int rec_every,
                                    int group, double* err, double* scratch, int B, int nx, int ny,
                                    int psi0_batched, void* stream) {
  const Solve s = {psi0, V, g, kappa, dt, nsteps, order, rec_every, nullptr, 0, nullptr,
                   nullptr, scratch, B, psi0_batched, stream};
  return solve_error(2, s, x, y, nullptr, dx, dy, 0.0, group, err, nx, ny, 1);
}

BLINDNO_API int blindno_gpe3d_error(const double* psi0, const double* V, const double* g,
                                    const double* kappa, const double* x, const double* y,
                                    const double* z, double dx, double dy, double dz, double dt,
                                    int nsteps, int order, int rec_every, int group, double* err,
                                    double* scratch, int B, int nx, int ny, int nz, int psi0_batched,
                                    void* stream) {
  const Solve s = {psi0, V, g, kappa, dt, nsteps, order, rec_every, nullptr, 0, nullptr,
                   nullptr, scratch, B, psi0_batched, stream};
  return solve_error(3, s, x, y, z, dx, dy, dz, group, err, nx, ny, nz);
}

BLINDNO_API int blindno_trapz2_frames(const double* a, const double* b, const double* x,
                                      const double* y, double* out, int frames, int nx, int ny,
                                      void* stream) {
  if (frames <= 0 || nx < 1 || ny < 1 || !a || !b || !x || !y || !out)
    return (int)hipErrorInvalidValue;
  trapz_frames_kernel<2, 256><<<frames, 256, 0, (hipStream_t)stream>>>(a, b, x, y, nullptr, out, nx, ny, 1);
  return (int)hipGetLastError();
}

BLINDNO_API int blindno_trapz3_frames(const double* a, const double* b, const double* x,
                                      const double* y, const double* z, double* out, int frames,
                                      int nx, int ny, int nz, void* stream) {
  if (frames <= 0 || nx < 1 || ny < 1 || nz < 1 || !a || !b || !x || !y || !z || !out)
    return (int)hipErrorInvalidValue;
  trapz_frames_kernel<3, 512><<<frames, 512, 0, (hipStream_t)stream>>>(a, b, x, y, z, out, nx, ny, nz);
  return (int)hipGetLastError();
}
