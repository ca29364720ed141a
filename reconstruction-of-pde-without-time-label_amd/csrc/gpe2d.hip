// Grid-resident 2D Gross-Pitaevskii split-step solver and the 2D trapezoid density residual
// (include/blindno_gpe2d.h), and the solver without its record, with the density-error sums
// reduced on the device (include/blindno_gpe2d_err.h).
//
//   i psi_t = -1/2 (psi_xx + psi_yy) + (V + g |psi|^2 + kappa |psi|^4) psi
// on a periodic nx x ny grid (row-major, y contiguous, complex128 interleaved), the reference's 1D
// scheme (1d_GPE/datagen_GPE.py:29-115, csrc/evaluators.hip gpe_solve_kernel) with one more axis:
//   N(h): psi <- exp(-i h (V + g|psi|^2 + kappa|psi|^4)) psi            pointwise
//   L(h): psi <- ifft2(exp(-i h/2 (kx^2 + ky^2)) fft2 psi)               kx = 2 pi fftfreq(nx, dx)
// Strang N(dt/2) L(dt) N(dt/2) or the nine-stage Yoshida sequence per step.
//
// gpe_solve_kernel keeps a trajectory in one workgroup's LDS (N <= 2048); a 256^2 complex128
// field is 1 MiB.  Here the field lives in global memory (the caller's scratch) and the kinetic
// phase is factorised, exp(-i h/2 kx^2) exp(-i h/2 ky^2), so L = L_x L_y and each factor is a
// batch of independent 1D transforms (FFT, multiply, inverse FFT, 1/n) along one axis:
//   row pass     a workgroup owns `tile` whole rows (a contiguous chunk of the field) and
//                transforms along y;
//   column pass  a workgroup owns `tile` >= 4 adjacent columns over all nx rows (each row of the
//                tile a contiguous segment of >= 64 B) and transforms along x.
// Both are one kernel template.  The tile sits in LDS exactly as it lies in global memory
// ([row][iy] / [ix][column]); the radix-2 Stockham passes of gpe_solve_kernel run on all of the
// tile's transforms at once, lanes walking the contiguous index fastest, so every LDS access of
// a wave is a run of contiguous 16-B elements -- there is no transposed copy and hence no
// power-of-two stride between lanes that a padded stride would have to break.
//
// All pointwise work is fused into the two passes: what precedes the transform (record 0 and
// the very first N, on the first row pass only) runs on the way into LDS, what follows it (the
// 1/n scale, N, the record, the next step's first N, the final field) on the way out.  One L is
// two launches, so a Strang step is 2 launches and a Yoshida step 8; there is no other kernel.
// A pass updates the field in place: a workgroup reads its whole tile before it writes it, and
// tiles are disjoint.  The only ordering between passes is the launch boundary on the stream:
// no cooperative launch, no grid barrier, no flag another workgroup waits on, and no memory
// location that two workgroups of a launch both touch.  A
// tile never spans two trajectories and the arithmetic of a point does not depend on the thread
// that runs it, so results are bit-deterministic and independent of B.
//
// LDS: two ping-pong buffers of n * tile points plus n/2 twiddles and n phase factors, 16 B
// each.  tile * n = 1024 points, one butterfly per thread of a 512-thread workgroup: 38 KiB at
// n = 256 (four workgroups per CU), 56 KiB at n = 1024.  The column pass keeps at least 4
// columns, so it holds 2048 points (76 KiB) at nx = 512 and 4096 points (152 KiB of the CU's
// 160 KiB) at nx = 1024.
// fp64 throughout; contraction is off so a complex product rounds like numpy's.
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

constexpr int kMinN = 4, kMaxN = 1024;   // BLINDNO_GPE2D_MIN_N / BLINDNO_GPE2D_MAX_N
constexpr int kTilePoints = 1024;        // points of a workgroup's tile (per ping-pong buffer)
constexpr int kMinCols = 4;              // column tile: 4 x 16 B = 64-B row segments at least
constexpr int kMaxThreads = 512;
constexpr int kTrapzBlock = 256;

struct PassArgs {
  const double* src;      // field read: psi0 on the first launch, the scratch field afterwards
  int64_t src_bstride;    // doubles per trajectory of src (0: one psi0 shared by the batch)
  double* field;          // (B, nx, ny, 2) scratch field written
  const double* V;        // (B, nx, ny)
  const double* g;        // (B)
  const double* kappa;    // (B)
  double* rec_abs64;      // (B, nrec, nx, ny) or NULL
  float* rec_abs32;       // the same in fp32 or NULL
  double* rec_psi;        // (B, nrec, nx, ny, 2) or NULL
  double* psi_out;        // (B, nx, ny, 2), written when write_out
  int nx, ny, nrec;
  int tile, lg_tile;      // rows / columns per workgroup
  int lg_n;               // log2 of the transform length (ny for the row pass, nx for the column pass)
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
// length n at once.  Point i of transform q sits at q*n + i (row pass) or i*cnt + q (column
// pass); butterfly t takes the contiguous index from its low bits.  With `lin` the inputs are
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
__global__ __launch_bounds__(kMaxThreads) void gpe2d_pass_kernel(const PassArgs a) {
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  const int n = 1 << a.lg_n, cnt = a.tile;
  const int points = n << a.lg_tile;
  cd* buf0 = reinterpret_cast<cd*>(smem_raw);
  cd* buf1 = buf0 + points;
  cd* tw = buf1 + points;     // n/2
  cd* lin = tw + (n >> 1);    // n
  const int tiles = (COL ? a.ny : a.nx) >> a.lg_tile;   // per trajectory
  const int b = blockIdx.x / tiles;
  const int t0 = (blockIdx.x - b * tiles) << a.lg_tile; // first row / column of the tile
  const int64_t N = (int64_t)a.nx * a.ny;
  const double g = a.g[b], kappa = a.kappa[b];
  const double* Vb = a.V + (int64_t)b * N;
  // global point of LDS point e, inside the trajectory
  auto gidx = [&](int e) -> int64_t {
    return COL ? (int64_t)(e >> a.lg_tile) * a.ny + t0 + (e & (cnt - 1)) : (int64_t)t0 * a.ny + e;
  };
  auto record = [&](cd p, int r, int64_t gi) {
    const int64_t o = ((int64_t)b * a.nrec + r) * N + gi;
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

// out[2f] = trapz_y(trapz_x((a_f - b_f)^2)), out[2f+1] = trapz_y(trapz_x(b_f^2)) as the weighted
// sum over the frame's points with the trapezoid weights wx(ix) wy(iy), w(i) = half the sum of
// the two adjacent spacings (one at an end).  One workgroup per frame, fixed-order reduction.
__global__ __launch_bounds__(kTrapzBlock) void trapz2_frames_kernel(
    const double* __restrict__ a, const double* __restrict__ b, const double* __restrict__ x,
    const double* __restrict__ y, double* __restrict__ out, int nx, int ny) {
  __shared__ double ra[kTrapzBlock], rb[kTrapzBlock];
  const int64_t N = (int64_t)nx * ny;
  const double* ap = a + (int64_t)blockIdx.x * N;
  const double* bp = b + (int64_t)blockIdx.x * N;
  double sa = 0.0, sb = 0.0;
  for (int64_t e = threadIdx.x; e < N; e += kTrapzBlock) {
    const int ix = (int)(e / ny), iy = (int)(e - (int64_t)ix * ny);
    const double wx = 0.5 * ((ix > 0 ? x[ix] - x[ix - 1] : 0.0) + (ix < nx - 1 ? x[ix + 1] - x[ix] : 0.0));
    const double wy = 0.5 * ((iy > 0 ? y[iy] - y[iy - 1] : 0.0) + (iy < ny - 1 ? y[iy + 1] - y[iy] : 0.0));
    const double w = wx * wy;
    const double bv = bp[e], d = ap[e] - bv;
    sa += w * (d * d);
    sb += w * (bv * bv);
  }
  ra[threadIdx.x] = sa;
  rb[threadIdx.x] = sb;
  __syncthreads();
  for (int s = kTrapzBlock / 2; s > 0; s >>= 1) {
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

// ---- blindno_gpe2d_error (include/blindno_gpe2d_err.h): the solver with its record reduced away.
//
// An error evaluation wants two numbers per trajectory and recorded step, the trapezoid integrals
// of (|psi| - |psi_ref|)^2 and |psi_ref|^2, not the frames.  The pass kernel above is driven by the
// same launch sequence as blindno_gpe2d_solve (gpe2d_enqueue below); its |psi| record is pointed at
// one frame per trajectory in scratch (nrec = 1, record index 0), and after each launch that wrote
// the frame two small launches reduce it:
//   stage one  one workgroup of 256 threads per (trajectory, tile of kErrTile consecutive cells):
//              thread t adds the terms of cells t, t + 256, ... of the tile in ascending order (a
//              wave's loads are one contiguous 512-B run each), the wave sums by a fixed shuffle
//              tree (offsets 32, 16 .. 1), lane 0 of the four waves meet in LDS and thread 0 adds
//              them in wave order -> partial (B, tiles, 2)
//   stage two  one workgroup per trajectory: thread t adds tiles t, t + 256, ... in ascending
//              order, then the same tree -> err[b, r, :]
// The per-cell terms are trapz2_frames_kernel's to the bit (w = wx wy, d = a - b, w (d d) and
// w (b b); contraction is off for the whole file); only the order of the sum differs.  Every
// addition has a fixed place, so a second call repeats the bits; a workgroup reads only its own
// trajectory's frame and its reference's and writes only its own two partials, so the rest of the
// batch cannot change a group's numbers.  The frame cannot be replaced by reading the field after
// the column pass: that pass has already applied the next step's first N (has_post2).
constexpr int kErrTile = BLINDNO_GPE2D_ERR_TILE;
constexpr int kErrBlock = 256;
static_assert(kErrTile >= 256 && kErrTile <= 4096 && (kErrTile & (kErrTile - 1)) == 0 &&
                  kErrTile % kErrBlock == 0,
              "BLINDNO_GPE2D_ERR_TILE: a power of two in [256, 4096]");

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

// frame (B, N): |psi| of every trajectory at one recorded step; ny is a power of two
__global__ __launch_bounds__(kErrBlock) void gpe2d_err_tile_kernel(
    const double* __restrict__ frame, const double* __restrict__ x, const double* __restrict__ y,
    double* __restrict__ partial, int64_t N, int tiles, int group, int nx, int ny, int lg_ny) {
  __shared__ double red[2][kErrBlock / 64];
  const int b = (int)blockIdx.x / tiles;
  const int tile = (int)blockIdx.x - b * tiles;
  const double* ap = frame + (int64_t)b * N;
  const double* bp = frame + (int64_t)(b / group * group) * N;
  double sa = 0.0, sb = 0.0;
  for (int k = 0; k < kErrTile / kErrBlock; ++k) {
    const int64_t e = (int64_t)tile * kErrTile + k * kErrBlock + (int)threadIdx.x;
    if (e < N) {                                 // N may be smaller than one tile
      const int iy = (int)(e & (ny - 1));
      const int ix = (int)(e >> lg_ny);
      const double wx = 0.5 * ((ix > 0 ? x[ix] - x[ix - 1] : 0.0) + (ix < nx - 1 ? x[ix + 1] - x[ix] : 0.0));
      const double wy = 0.5 * ((iy > 0 ? y[iy] - y[iy - 1] : 0.0) + (iy < ny - 1 ? y[iy + 1] - y[iy] : 0.0));
      const double w = wx * wy;
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

__global__ __launch_bounds__(kErrBlock) void gpe2d_err_sum_kernel(const double* __restrict__ partial,
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

int ilog2(int v) {
  int l = 0;
  while ((1 << l) < v) ++l;
  return l;
}

bool pow2_in_range(int v) { return v >= kMinN && v <= kMaxN && (v & (v - 1)) == 0; }

int min_int(int a, int b) { return a < b ? a : b; }
int max_int(int a, int b) { return a > b ? a : b; }

// rows per workgroup of the row pass / columns per workgroup of the column pass
int row_tile(int nx, int ny) { return max_int(1, min_int(nx, kTilePoints / ny)); }
int col_tile(int nx, int ny) { return max_int(kMinCols, min_int(ny, kTilePoints / nx)); }

bool gpe2d_grid(int B, int nx, int ny, int64_t* row_blocks, int64_t* col_blocks) {
  if (B <= 0 || !pow2_in_range(nx) || !pow2_in_range(ny)) return false;
  *row_blocks = (int64_t)B * (nx / row_tile(nx, ny));
  *col_blocks = (int64_t)B * (ny / col_tile(nx, ny));
  return *row_blocks <= 0x7fffffff && *col_blocks <= 0x7fffffff;
}

bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

template <bool COL>
hipError_t launch_pass(const PassArgs& a, int B, hipStream_t st) {
  const int n = 1 << a.lg_n;
  const int points = n << a.lg_tile;
  const size_t sh = sizeof(cd) * (2 * (size_t)points + n / 2 + n);
  if (sh > 64 * 1024) {
    // more dynamic LDS than the default cap; a refusal surfaces as the launch's own error
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&gpe2d_pass_kernel<COL>),
                              hipFuncAttributeMaxDynamicSharedMemorySize, (int)sh);
    (void)hipGetLastError();
  }
  const int threads = max_int(64, min_int(kMaxThreads, points / 2));
  const int tiles = (COL ? a.ny : a.nx) >> a.lg_tile;
  gpe2d_pass_kernel<COL><<<B * tiles, threads, sh, st>>>(a);
  return hipGetLastError();
}

}  // namespace

BLINDNO_API int64_t blindno_gpe2d_scratch_doubles(int B, int nx, int ny) {
  int64_t rb, cb;
  if (!gpe2d_grid(B, nx, ny, &rb, &cb)) return -1;
  return 2 * (int64_t)B * nx * ny;
}

BLINDNO_API int64_t blindno_gpe2d_launches(int nsteps, int order) {
  if (nsteps < 0 || (order != 2 && order != 4)) return -1;
  return nsteps == 0 ? 1 : (int64_t)nsteps * (order == 2 ? 2 : 8);
}

namespace {

// What blindno_gpe2d_error adds to the launch sequence: the frame that takes the record's place and
// the reduction enqueued after every launch that wrote it.
struct ErrPlan {
  const double *x, *y;
  double* frame;      // (B, N) |psi| of the step being reduced
  double* partial;    // (B, tiles, 2)
  double* err;        // (B, nrec, 2)
  int tiles, group;
};

// The launch sequence of blindno_gpe2d_solve.  With `E` (blindno_gpe2d_error) the only differences
// are where the pass kernel records -- E->frame as a one-frame fp64 record, index 0 at every record
// step -- and the two reduction launches after each launch that recorded.
int gpe2d_enqueue(const double* psi0, const double* V, const double* g, const double* kappa,
                  double dx, double dy, double dt, int nsteps, int order, int rec_every, void* rec_abs,
                  int rec_abs_f32, double* rec_psi, double* psi_out, double* scratch, int B, int nx,
                  int ny, int psi0_batched, const ErrPlan* E, void* stream) {
  int64_t rb, cb;
  if (!gpe2d_grid(B, nx, ny, &rb, &cb) || nsteps < 0 || rec_every < 1 ||
      (order != 2 && order != 4) || !psi0 || !V || !g || !kappa || !scratch ||
      (rec_abs_f32 != 0 && rec_abs_f32 != 1) || !(dx > 0.0) || !(dy > 0.0) || !aligned16(psi0) ||
      !aligned16(scratch) || !aligned16(rec_psi) || !aligned16(psi_out))
    return (int)hipErrorInvalidValue;
  hipStream_t st = (hipStream_t)stream;
  const int64_t N = (int64_t)nx * ny;
  PassArgs base = {};
  base.field = scratch;
  base.V = V;
  base.g = g;
  base.kappa = kappa;
  base.rec_abs64 = E ? E->frame : rec_abs_f32 ? nullptr : (double*)rec_abs;
  base.rec_abs32 = !E && rec_abs_f32 ? (float*)rec_abs : nullptr;
  base.rec_psi = rec_psi;
  base.psi_out = psi_out;
  base.nx = nx;
  base.ny = ny;
  const int nrec = nsteps / rec_every + 1;
  base.nrec = E ? 1 : nrec;
  // record r has just been written to E->frame by the launch before: reduce it into err[:, r, :]
  auto reduce = [&](int r) -> hipError_t {
    gpe2d_err_tile_kernel<<<(unsigned)((int64_t)B * E->tiles), kErrBlock, 0, st>>>(
        E->frame, E->x, E->y, E->partial, N, E->tiles, E->group, nx, ny, ilog2(ny));
    gpe2d_err_sum_kernel<<<B, kErrBlock, 0, st>>>(E->partial, E->err, E->tiles, nrec, r);
    return hipGetLastError();
  };
  base.rec_pre = base.rec_post = -1;

  PassArgs row = base, col = base;
  row.tile = row_tile(nx, ny);
  row.lg_tile = ilog2(row.tile);
  row.lg_n = ilog2(ny);
  row.d = dy;
  col.tile = col_tile(nx, ny);
  col.lg_tile = ilog2(col.tile);
  col.lg_n = ilog2(nx);
  col.d = dx;
  row.src = psi0;                        // the first launch reads psi0 and records step 0
  row.src_bstride = psi0_batched ? 2 * N : 0;
  row.rec_pre = 0;
  col.src = scratch;
  col.src_bstride = 2 * N;

  if (nsteps == 0) {
    row.do_lin = 0;
    row.write_out = psi_out != nullptr;
    hipError_t e = launch_pass<false>(row, B, st);
    if (e == hipSuccess && E) e = reduce(0);
    return (int)e;
  }
  // Yoshida coefficients as the reference forms them (2**(1/3) = pow(2, 1/3))
  const double cr = pow(2.0, 1.0 / 3.0);
  const double c2 = 2.0 - cr;
  const double a1 = 1.0 / c2, a2 = -cr / c2;
  // per step: N(hn[0]) L(hl[0]) N(hn[1]) ... L(hl[nl-1]) N(hn[nl])
  const int nl = order == 2 ? 1 : 4;
  const double hn2[2] = {dt / 2, dt / 2}, hl2[1] = {dt};
  const double hn4[5] = {a1 * dt, a2 * dt, a1 * dt, a2 * dt, a1 * dt};
  const double hl4[4] = {a1 * dt, a2 * dt, a2 * dt, a1 * dt};
  const double* hn = order == 2 ? hn2 : hn4;
  const double* hl = order == 2 ? hl2 : hl4;
  row.do_lin = col.do_lin = 1;
  row.has_pre = 1;                       // the first step's first N; later ones ride on the
  row.h_pre = hn[0];                     // previous step's column pass (has_post2)
  for (int n = 1; n <= nsteps; ++n) {
    for (int l = 0; l < nl; ++l) {
      row.lin_h = col.lin_h = hl[l];
      hipError_t e = launch_pass<false>(row, B, st);
      if (e != hipSuccess) return (int)e;
      if (E && row.rec_pre >= 0 && (e = reduce(0)) != hipSuccess) return (int)e;
      row.src = scratch;
      row.src_bstride = 2 * N;
      row.rec_pre = -1;
      row.has_pre = 0;
      const bool last = l == nl - 1;
      col.has_post1 = 1;
      col.h_post1 = hn[l + 1];
      const int rec = last && n % rec_every == 0 ? n / rec_every : -1;
      col.rec_post = rec >= 0 && E ? 0 : rec;
      col.has_post2 = last && n < nsteps;
      col.h_post2 = hn[0];
      col.write_out = last && n == nsteps && psi_out != nullptr;
      e = launch_pass<true>(col, B, st);
      if (e != hipSuccess) return (int)e;
      if (E && rec >= 0 && (e = reduce(rec)) != hipSuccess) return (int)e;
    }
  }
  return (int)hipSuccess;
}

}  // namespace

BLINDNO_API int blindno_gpe2d_solve(const double* psi0, const double* V, const double* g,
                                    const double* kappa, double dx, double dy, double dt, int nsteps,
                                    int order, int rec_every, void* rec_abs, int rec_abs_f32,
                                    double* rec_psi, double* psi_out, double* scratch, int B, int nx,
                                    int ny, int psi0_batched, void* stream) {
  return gpe2d_enqueue(psi0, V, g, kappa, dx, dy, dt, nsteps, order, rec_every, rec_abs, rec_abs_f32,
                       rec_psi, psi_out, scratch, B, nx, ny, psi0_batched, nullptr, stream);
}

BLINDNO_API int64_t blindno_gpe2d_error_scratch_doubles(int B, int nx, int ny) {
  int64_t rb, cb;
  if (!gpe2d_grid(B, nx, ny, &rb, &cb)) return -1;
  const int64_t N = (int64_t)nx * ny;
  const int64_t tiles = (N + kErrTile - 1) / kErrTile;
  return 3 * (int64_t)B * N + 2 * (int64_t)B * tiles;   // field, frame, tile partials
}

BLINDNO_API int64_t blindno_gpe2d_error_launches(int nsteps, int order, int rec_every) {
  const int64_t solve = blindno_gpe2d_launches(nsteps, order);
  if (solve < 0 || rec_every < 1) return -1;
  return solve + 2 * ((int64_t)(nsteps / rec_every) + 1);
}

BLINDNO_API int blindno_gpe2d_error(const double* psi0, const double* V, const double* g,
                                    const double* kappa, const double* x, const double* y, double dx,
                                    double dy, double dt, int nsteps, int order, int rec_every,
                                    int group, double* err, double* scratch, int B, int nx, int ny,
                                    int psi0_batched, void* stream) {
  int64_t rb, cb;
  if (!gpe2d_grid(B, nx, ny, &rb, &cb) || group < 1 || B % group != 0 || !x || !y || !err ||
      !scratch || !aligned16(scratch))
    return (int)hipErrorInvalidValue;
  const int64_t N = (int64_t)nx * ny;
  const int64_t BN = (int64_t)B * N;
  ErrPlan E;
  E.x = x;
  E.y = y;
  E.frame = scratch + 2 * BN;                  // after the working field
  E.partial = scratch + 3 * BN;
  E.err = err;
  // tiles <= the row pass's workgroups per trajectory, so B * tiles fits the grid as its launch does
  E.tiles = (int)((N + kErrTile - 1) / kErrTile);
  E.group = group;
  return gpe2d_enqueue(psi0, V, g, kappa, dx, dy, dt, nsteps, order, rec_every, nullptr, 0, nullptr,
                       nullptr, scratch, B, nx, ny, psi0_batched, &E, stream);
}

BLINDNO_API int blindno_trapz2_frames(const double* a, const double* b, const double* x,
                                      const double* y, double* out, int frames, int nx, int ny,
                                      void* stream) {
  if (frames <= 0 || nx < 1 || ny < 1 || !a || !b || !x || !y || !out)
    return (int)hipErrorInvalidValue;
  trapz2_frames_kernel<<<frames, kTrapzBlock, 0, (hipStream_t)stream>>>(a, b, x, y, out, nx, ny);
  return (int)hipGetLastError();
}
