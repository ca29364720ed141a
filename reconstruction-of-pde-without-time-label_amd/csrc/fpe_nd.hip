// Grid-resident Fokker-Planck propagation on 1D / 2D / 3D grids of any size (include/blindno_fpe.h).
//
// dp/dt = M p, the finite-volume master equation of csrc/evaluators.hip (fp_propagate_kernel) with
// one more axis: N = nx*ny*nz cells, cell i = (ix*ny + iy)*nz + iz,
//   (M p)_i = cxm_i p_{i-ex} + cxp_i p_{i+ex} + cym_i p_{i-ey} + cyp_i p_{i+ey}
//           + czm_i p_{i-ez} + czp_i p_{i+ez} - diag_i p_i
// coef (B, 7, N) = [diag, cxm, cxp, cym, cyp, czm, czp] (in-rates from the neighbours, zero across a
// reflecting wall; neighbour indices wrap per axis, which is the periodic case).
//
// fp_propagate_kernel keeps a trajectory in one workgroup's LDS (N <= 8192).  Here the density p
// and the two Horner iterates live in global memory and ONE launch is ONE Horner pass
//   w_out = p + (h/k) M w_in
// over every cell of every trajectory: workgroups of 256 consecutive cells tile the (B, N) cells,
// and the only ordering between passes is the launch boundary on the stream (no cooperative
// launch, no grid-wide barrier, no flag or counter that another workgroup waits on).
//
// Why no LDS tile: per cell a pass streams 7 coefficients, p and the result (9 doubles, no reuse)
// and reads 7 values of w_in, each of which 7 cells want.  With z fastest the z neighbours share
// the cell's own cache line, the y neighbours lie nz doubles away (inside the workgroup's own
// 2 KiB span for nz <= 128) and the x neighbours ny*nz away (L2: at 40^3 a whole trajectory's w
// is 512 KB of the XCD's 4 MiB).  Staging w_in in LDS would only move those already-cached reads;
// the 9 streamed doubles set the time.  At 256 threads and no LDS the kernel runs at full
// occupancy, which is what a latency-bound stream of fp64 loads wants.
//
// The per-cell operation order is fp_propagate_kernel's with the two z terms appended before the
// final fma; with nz = 1 the z neighbours are the cell itself and their coefficients are zero, so
// the result is bit-identical to blindno_fp_propagate.  Contraction is off as it is there.
#include "common.h"
#include "blindno.h"

#pragma clang fp contract(off)

namespace {

constexpr int kTile = 256;                       // cells per workgroup
constexpr int64_t kMaxCells = (int64_t)1 << 26;  // BLINDNO_FP_ND_MAX_CELLS

// One Horner pass.  p and w_out may be the same buffer (each cell reads its own p before writing
// its own w_out); w_in is never w_out.  Strides are per trajectory, in doubles.
__global__ __launch_bounds__(kTile) void fp_nd_pass_kernel(
    const double* __restrict__ coef, const double* p, int64_t p_stride,
    const double* w_in, int64_t win_stride, double* w_out, int64_t wout_stride, int N, int nx,
    int ny, int nz, int tiles, double h, int k) {
  const int b = blockIdx.x / tiles;
  const int i = (blockIdx.x - b * tiles) * kTile + threadIdx.x;
  if (i >= N) return;
  const int ixy = i / nz, iz = i - ixy * nz;
  const int ix = ixy / ny, iy = ixy - ix * ny;
  const int xm = ((ix == 0 ? nx - 1 : ix - 1) * ny + iy) * nz + iz;
  const int xp = ((ix == nx - 1 ? 0 : ix + 1) * ny + iy) * nz + iz;
  const int ym = (ix * ny + (iy == 0 ? ny - 1 : iy - 1)) * nz + iz;
  const int yp = (ix * ny + (iy == ny - 1 ? 0 : iy + 1)) * nz + iz;
  const int zm = ixy * nz + (iz == 0 ? nz - 1 : iz - 1);
  const int zp = ixy * nz + (iz == nz - 1 ? 0 : iz + 1);
  const double* cf = coef + (int64_t)b * 7 * N;
  const double* w = w_in + (int64_t)b * win_stride;
  const double hk = h / (double)k;
  double mw = -cf[i] * w[i];
  mw = fma(cf[(int64_t)N + i], w[xm], mw);
  mw = fma(cf[2 * (int64_t)N + i], w[xp], mw);
  mw = fma(cf[3 * (int64_t)N + i], w[ym], mw);
  mw = fma(cf[4 * (int64_t)N + i], w[yp], mw);
  mw = fma(cf[5 * (int64_t)N + i], w[zm], mw);
  mw = fma(cf[6 * (int64_t)N + i], w[zp], mw);
  w_out[(int64_t)b * wout_stride + i] = fma(hk, mw, p[(int64_t)b * p_stride + i]);
}

__global__ __launch_bounds__(kTile) void fp_nd_copy_kernel(const double* __restrict__ src,
                                                           double* __restrict__ dst,
                                                           int64_t dst_stride, int N, int tiles) {
  const int b = blockIdx.x / tiles;
  const int i = (blockIdx.x - b * tiles) * kTile + threadIdx.x;
  if (i < N) dst[(int64_t)b * dst_stride + i] = src[(int64_t)b * N + i];
}

bool fp_nd_cells(int B, int nx, int ny, int nz, int64_t* N, int64_t* blocks) {
  if (B <= 0 || nx < 1 || ny < 1 || nz < 1) return false;
  const int64_t n = (int64_t)nx * ny;          // < 2^62
  if (n > kMaxCells || n * nz > kMaxCells) return false;
  *N = n * nz;
  *blocks = (int64_t)B * ((*N + kTile - 1) / kTile);
  return *blocks <= 0x7fffffff;                // one workgroup index per (trajectory, tile)
}

}  // namespace

BLINDNO_API int64_t blindno_fp_propagate_nd_scratch_doubles(int B, int nx, int ny, int nz) {
  int64_t N, blocks;
  if (!fp_nd_cells(B, nx, ny, nz, &N, &blocks)) return -1;
  return 2 * (int64_t)B * N;
}

BLINDNO_API int blindno_fp_propagate_nd(const double* p0, const double* coef, double* out,
                                        double* scratch, int B, int nx, int ny, int nz, int nout,
                                        int substeps, int degree, double dt_out, void* stream) {
  int64_t N, blocks;
  if (!fp_nd_cells(B, nx, ny, nz, &N, &blocks) || nout < 1 || substeps < 1 || degree < 1 ||
      !p0 || !coef || !out || !scratch)
    return (int)hipErrorInvalidValue;
  hipStream_t st = (hipStream_t)stream;
  const int tiles = (int)((N + kTile - 1) / kTile);
  const int grid = (int)blocks;
  const double h = dt_out / substeps;
  const int64_t os = (int64_t)nout * N;        // trajectory stride of out
  double* wa = scratch;
  double* wb = scratch + (int64_t)B * N;
  fp_nd_copy_kernel<<<grid, kTile, 0, st>>>(p0, out, os, (int)N, tiles);
#define PASS(P_, PS_, WI_, WIS_, WO_, WOS_, K_)                                                  \
  fp_nd_pass_kernel<<<grid, kTile, 0, st>>>(coef, P_, PS_, WI_, WIS_, WO_, WOS_, (int)N, nx, ny, \
                                            nz, tiles, h, K_)
  for (int o = 1; o < nout; ++o) {
    const double* prev = out + (int64_t)(o - 1) * N;   // record o-1, stride os
    double* rec = out + (int64_t)o * N;                // record o, stride os: holds p from substep 1 on
    for (int sub = 0; sub < substeps; ++sub) {
      if (degree == 1) {
        // the single pass reads its neighbours from p itself, so p may not be overwritten in
        // place: it moves prev -> wa -> wb -> wa ... and lands in the record on the last substep
        const double* src = sub == 0 ? prev : ((sub - 1) & 1 ? wb : wa);
        const int64_t ss = sub == 0 ? os : N;
        double* dst = sub == substeps - 1 ? rec : (sub & 1 ? wb : wa);
        const int64_t ds = sub == substeps - 1 ? os : N;
        PASS(src, ss, src, ss, dst, ds, 1);
        continue;
      }
      const double* p = sub == 0 ? prev : rec;
      const double* wi = p;
      int64_t wis = os;
      double* wo = wa;
      for (int k = degree; k >= 2; --k) {
        PASS(p, os, wi, wis, wo, N, k);
        wi = wo;
        wis = N;
        wo = wo == wa ? wb : wa;
      }
      // last pass: each cell reads its own p and writes its own cell of the record
      PASS(p, os, wi, wis, rec, os, 1);
    }
  }
#undef PASS
  return (int)hipGetLastError();
}

// ---- blindno_fp_error_nd (include/blindno_fpe_err.h): the same propagation with no record.
//
// A density-error evaluation wants two numbers per trajectory and frame, |p - p_ref|^2 and
// |p_ref|^2, not the frames: at 40^3 x 400 frames the record is 204.8 MB per trajectory against
// 1.5 MB of state.  Here the density lives in scratch beside the two iterates, the passes are
// fp_nd_pass_kernel's in blindno_fp_propagate_nd's order (so every iterate has the record's bits),
// and after the initial state and after every output interval two small launches reduce the sums:
//   stage one  one workgroup per (trajectory, tile of 256 cells): each lane squares its cell, the
//              wave sums by a fixed shuffle tree (offsets 32, 16 .. 1), lane 0 of the four waves
//              meet in LDS and thread 0 adds them in wave order -> partial (B, tiles, 2)
//   stage two  one workgroup per trajectory: thread t adds tiles t, t + 256, .. in index order,
//              then the same tree -> err (B, nout, 2)
// Every addition has a fixed place, so a second call repeats the bits, and a trajectory reads only
// its own group's cells, so the rest of the batch cannot change them.  Trajectory b's reference is
// trajectory (b / group) * group; for the reference itself p - p_ref is 0.0 in every cell.
namespace {

// sum over the workgroup of (a, b), valid in thread 0; `red` is 2 x 4 doubles of LDS
__device__ __forceinline__ void fp_nd_block_sum2(double& a, double& b, double (*red)[kTile / 64]) {
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
    for (int w = 1; w < kTile / 64; ++w) {
      a += red[0][w];
      b += red[1][w];
    }
  }
}

__global__ __launch_bounds__(kTile) void fp_nd_err_tile_kernel(const double* __restrict__ p,
                                                               double* __restrict__ partial, int N,
                                                               int tiles, int group) {
  __shared__ double red[2][kTile / 64];
  const int b = blockIdx.x / tiles;
  const int i = (blockIdx.x - b * tiles) * kTile + threadIdx.x;
  double num = 0.0, den = 0.0;
  if (i < N) {
    const double r = p[(int64_t)(b / group * group) * N + i];
    const double d = p[(int64_t)b * N + i] - r;
    num = d * d;
    den = r * r;
  }
  fp_nd_block_sum2(num, den, red);
  if (threadIdx.x == 0) {
    partial[2 * (int64_t)blockIdx.x] = num;
    partial[2 * (int64_t)blockIdx.x + 1] = den;
  }
}

__global__ __launch_bounds__(kTile) void fp_nd_err_sum_kernel(const double* __restrict__ partial,
                                                              double* __restrict__ err, int tiles,
                                                              int nout, int o) {
  __shared__ double red[2][kTile / 64];
  const int b = blockIdx.x;
  const double* pt = partial + 2 * (int64_t)b * tiles;
  double num = 0.0, den = 0.0;
  for (int t = threadIdx.x; t < tiles; t += kTile) {
    num += pt[2 * (int64_t)t];
    den += pt[2 * (int64_t)t + 1];
  }
  fp_nd_block_sum2(num, den, red);
  if (threadIdx.x == 0) {
    double* e = err + 2 * ((int64_t)b * nout + o);
    e[0] = num;
    e[1] = den;
  }
}

}  // namespace

BLINDNO_API int64_t blindno_fp_error_nd_scratch_doubles(int B, int nx, int ny, int nz) {
  int64_t N, blocks;
  if (!fp_nd_cells(B, nx, ny, nz, &N, &blocks)) return -1;
  return 3 * (int64_t)B * N + 2 * blocks;      // p, the two iterates, the tile partials
}

BLINDNO_API int blindno_fp_error_nd(const double* p0, const double* coef, double* err,
                                    double* scratch, int B, int group, int nx, int ny, int nz,
                                    int nout, int substeps, int degree, double dt_out,
                                    void* stream) {
  int64_t N, blocks;
  if (!fp_nd_cells(B, nx, ny, nz, &N, &blocks) || group < 1 || B % group != 0 || nout < 1 ||
      substeps < 1 || degree < 1 || !p0 || !coef || !err || !scratch)
    return (int)hipErrorInvalidValue;
  hipStream_t st = (hipStream_t)stream;
  const int tiles = (int)((N + kTile - 1) / kTile);
  const int grid = (int)blocks;
  const double h = dt_out / substeps;
  const int64_t BN = (int64_t)B * N;
  double* p = scratch;                         // the density; with degree 1 it rotates through all three
  double* wa = scratch + BN;
  double* wb = scratch + 2 * BN;
  double* partial = scratch + 3 * BN;          // (B, tiles, 2)
  fp_nd_copy_kernel<<<grid, kTile, 0, st>>>(p0, p, N, (int)N, tiles);
#define PASS(P_, WI_, WO_, K_)                                                                  \
  fp_nd_pass_kernel<<<grid, kTile, 0, st>>>(coef, P_, N, WI_, N, WO_, N, (int)N, nx, ny, nz, tiles, \
                                            h, K_)
  for (int o = 0; o < nout; ++o) {
    for (int sub = 0; o > 0 && sub < substeps; ++sub) {
      if (degree == 1) {
        // the single pass reads its neighbours from p itself: write the next density elsewhere
        PASS(p, p, wa, 1);
        double* t = p;
        p = wa;
        wa = t;
        continue;
      }
      const double* wi = p;
      double* wo = wa;
      for (int k = degree; k >= 2; --k) {
        PASS(p, wi, wo, k);
        wi = wo;
        wo = wo == wa ? wb : wa;
      }
      // last pass: each cell reads its own p and writes its own cell of p
      PASS(p, wi, p, 1);
    }
    fp_nd_err_tile_kernel<<<grid, kTile, 0, st>>>(p, partial, (int)N, tiles, group);
    fp_nd_err_sum_kernel<<<B, kTile, 0, st>>>(partial, err, tiles, nout, o);
  }
#undef PASS
  return (int)hipGetLastError();
}
