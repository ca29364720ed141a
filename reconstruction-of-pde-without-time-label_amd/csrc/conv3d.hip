// 3D convolution (nn.Conv3d with bias, any kernel / stride / zero padding per axis, groups 1) of
// the NIOFP3D snapshot encoders' ConvBlock3D layers (2d_FPE/Baselines.py:26-38, Encoder3D /
// Encoder3D_down :322-429), forward and both adjoints, as implicit GEMMs on the fp32 matrix
// cores (v_mfma_f32_16x16x4f32: exact fp32 products, fixed accumulation order -- deterministic).
// The decomposition is csrc/conv.hip's with one more axis (a = 0, 1, 2 for depth, height, width):
//
//   FWD   y[n][co][o]  = b[co] + sum_{ci,k} W[co][ci][k] x[n][ci][o s - p + k]
//         GEMM  M = Co, N = output voxels (n, do, ho, wo), K = Ci KD KH KW
//   BWD_D dx[n][ci][i] = sum_{co,k} W[co][ci][k] dy[n][co][(i + p - k) / s]
//         split into stride-phase classes: input voxels with (i_a + p_a) % s_a = r_a on every
//         axis only meet taps k_a = r_a + s_a j_a, so each class (up to 8 with strides <= 2) is
//         its own GEMM  M = Ci, N = class voxels, K = Co x (its taps).  The taps off the stride
//         lattice are never visited; voxels of a class without taps (a stride above the kernel
//         extent) receive exactly 0.
//   BWD_W dW[co][ci][k] = sum_{n,o} dy[n][co][o] x[n][ci][o s - p + k],  db[co] = sum dy
//         GEMM  M = Co, N = Ci KD KH KW + 1 (the extra column is the bias: B = 1), K = output
//         voxels, cut over blockIdx.z into fixed K ranges; the partials are reduced in a fixed
//         order afterwards (blindno_reduce_partials).
//
// Tiling for CDNA4 wave64 as in conv.hip: a 256-thread workgroup computes a BM x BN tile (128 x
// 128 where the GEMM has the rows and the tiles to fill the chip, 64 x 64 otherwise) as 2 x 2
// waves, K in steps of 16 staged through double-buffered LDS.  The LDS tiles are k-contiguous per
// row (A[m][k], B[n][k], rows padded to 20 floats) and the MFMA K order is permuted (step s takes
// k = 4 (lane >> 4) + s), so one ds_read_b128 brings a lane's operands of four MFMA steps; the
// next step's global loads are issued before the current step's MFMAs.  There is no im2col
// buffer: each loader lane decodes its (channel, tap) / voxel indices with multiply-high
// divisions by the launch's constants (FastDiv).  GEMM indices are 32-bit (checked on the host),
// every flat tensor offset is 64-bit.
//
// The deep encoder layers (7_1, 7_2, 7_3: 1-3 output voxels per volume, K = 512 x 27) leave the
// chip short of workgroups, so the forward and the input gradient take nsplit: K is cut into
// nsplit ranges whose partial output slabs are summed in split order.
#include "common.h"
#include "blindno.h"

using namespace blindno;

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int MF = 16;                            // MFMA block (16 x 16 x 4)
constexpr int NR = 4;                             // accumulator registers per block
constexpr int BK = 16;                            // K per step
constexpr int SK = BK + 4;                        // LDS row stride (floats)

enum { FWD = 0, BWD_D = 1, BWD_W = 2 };

// one stride-phase class of BWD_D, per axis a: input voxels i = i0 + s t (t < c), taps
// k = r + s j (j < nk), output voxel o = o0 + t - j
constexpr int kMaxPhases = 8;    // sd sh sw <= 8 (strides <= 2 per axis, or e.g. (2, 3, 1))
struct Phase3 {
  int i0[3], c[3], r[3], nk[3], o0[3];
  int Ncol, K;
  FastDiv dC, dC12, dC2, dT, dT12, dT2;   // by c0 c1 c2, c1 c2, c2; nk0 nk1 nk2, nk1 nk2, nk2
};

struct Conv3Args {
  int N, Ci, Co;
  int I[3], O[3], Kk[3], s[3], p[3];   // input / output / kernel extents, stride, padding
  int ivol, ovol, kvol;                // I0 I1 I2, O0 O1 O2, KD KH KW
  int M, Ncol, K;                      // GEMM sizes of this mode
  int kchunk;                          // K per split (multiple of BK)
  int nph;                             // BWD_D: stride-phase classes (blockIdx.z = class + nph split)
  int64_t slab;                        // FWD / BWD_D: floats per partial output slab
  FastDiv dKvol, dK12, dK2, dOvol, dO12, dO2;
  Phase3 phase[kMaxPhases];            // BWD_D
};

// (d, h, w) of a flat index by the divisors of (e1 e2, e2)
__device__ __forceinline__ void split3(int v, const FastDiv& d12, const FastDiv& d2, int e12, int e2,
                                       int& a, int& b, int& c) {
  a = (int)d12.div((unsigned)v);
  const int r = v - a * e12;
  b = (int)d2.div((unsigned)r);
  c = r - b * e2;
}

// ---- A operand (BM x BK tile), element (m, k) of global (mg, kg)
template <int MODE>
__device__ __forceinline__ float load_a(const float* __restrict__ pa, const Conv3Args& g,
                                        const Phase3& ph, int mg, int kg, int kend) {
  if (mg >= g.M || kg >= kend) return 0.f;
  if (MODE == FWD) return pa[(int64_t)mg * g.K + kg];                       // W[co][k]
  if (MODE == BWD_D) {                                    // W[co][ci][r + s j] per axis
    const int nt = ph.nk[0] * ph.nk[1] * ph.nk[2];
    const int co = (int)ph.dT.div((unsigned)kg), j = kg - co * nt;
    int jd, jh, jw;
    split3(j, ph.dT12, ph.dT2, ph.nk[1] * ph.nk[2], ph.nk[2], jd, jh, jw);
    const int kd = ph.r[0] + g.s[0] * jd, kh = ph.r[1] + g.s[1] * jh, kw = ph.r[2] + g.s[2] * jw;
    return pa[((int64_t)co * g.Ci + mg) * g.kvol + (kd * g.Kk[1] + kh) * g.Kk[2] + kw];
  }
  // BWD_W: dy[n][co][q], k = output voxel
  const int n = (int)g.dOvol.div((unsigned)kg), q = kg - n * g.ovol;
  return pa[((int64_t)n * g.Co + mg) * g.ovol + q];
}

// voxel decomposition of the B operand's N index (FWD: output voxel, BWD_D: input voxel)
struct Vox {
  int64_t base;   // FWD: x offset of (n, 0, ...); BWD_D: dy offset of (n, 0, ...)
  int d, h, w;    // FWD: o s - p per axis; BWD_D: o0 + t per axis
  bool ok;
};

template <int MODE>
__device__ __forceinline__ Vox decode_vox(const Conv3Args& g, const Phase3& ph, int ng) {
  Vox p;
  p.ok = ng < (MODE == BWD_D ? ph.Ncol : g.Ncol);
  const int v = p.ok ? ng : 0;
  if (MODE == FWD) {
    const int n = (int)g.dOvol.div((unsigned)v), q = v - n * g.ovol;
    int od, oh, ow;
    split3(q, g.dO12, g.dO2, g.O[1] * g.O[2], g.O[2], od, oh, ow);
    p.base = (int64_t)n * g.Ci * g.ivol;
    p.d = od * g.s[0] - g.p[0];
    p.h = oh * g.s[1] - g.p[1];
    p.w = ow * g.s[2] - g.p[2];
  } else {
    const int cv = ph.c[0] * ph.c[1] * ph.c[2];
    const int n = (int)ph.dC.div((unsigned)v), q = v - n * cv;
    int td, th, tw;
    split3(q, ph.dC12, ph.dC2, ph.c[1] * ph.c[2], ph.c[2], td, th, tw);
    p.base = (int64_t)n * g.Co * g.ovol;
    p.d = ph.o0[0] + td;
    p.h = ph.o0[1] + th;
    p.w = ph.o0[2] + tw;
  }
  return p;
}

// dx offset of BWD_D's class-local voxel (channel 0)
__device__ __forceinline__ int64_t dx_offset(const Conv3Args& g, const Phase3& ph, int ng) {
  const int cv = ph.c[0] * ph.c[1] * ph.c[2];
  const int n = (int)ph.dC.div((unsigned)ng), q = ng - n * cv;
  int td, th, tw;
  split3(q, ph.dC12, ph.dC2, ph.c[1] * ph.c[2], ph.c[2], td, th, tw);
  const int d = ph.i0[0] + g.s[0] * td, h = ph.i0[1] + g.s[1] * th, w = ph.i0[2] + g.s[2] * tw;
  return (int64_t)n * g.Ci * g.ivol + ((int64_t)d * g.I[1] + h) * g.I[2] + w;
}

// B element (k, voxel) for FWD / BWD_D
template <int MODE>
__device__ __forceinline__ float load_b_vox(const float* __restrict__ pb, const Conv3Args& g,
                                            const Phase3& ph, const Vox& p, int kg, int kend) {
  if (!p.ok || kg >= kend) return 0.f;
  if (MODE == FWD) {
    const int ch = (int)g.dKvol.div((unsigned)kg), t = kg - ch * g.kvol;
    int kd, kh, kw;
    split3(t, g.dK12, g.dK2, g.Kk[1] * g.Kk[2], g.Kk[2], kd, kh, kw);
    const int d = p.d + kd, h = p.h + kh, w = p.w + kw;
    if ((unsigned)d >= (unsigned)g.I[0] || (unsigned)h >= (unsigned)g.I[1] ||
        (unsigned)w >= (unsigned)g.I[2])
      return 0.f;
    return pb[p.base + (int64_t)ch * g.ivol + ((int64_t)d * g.I[1] + h) * g.I[2] + w];
  }
  const int nt = ph.nk[0] * ph.nk[1] * ph.nk[2];
  const int co = (int)ph.dT.div((unsigned)kg), j = kg - co * nt;
  int jd, jh, jw;
  split3(j, ph.dT12, ph.dT2, ph.nk[1] * ph.nk[2], ph.nk[2], jd, jh, jw);
  const int d = p.d - jd, h = p.h - jh, w = p.w - jw;
  if ((unsigned)d >= (unsigned)g.O[0] || (unsigned)h >= (unsigned)g.O[1] ||
      (unsigned)w >= (unsigned)g.O[2])
    return 0.f;
  return pb[p.base + (int64_t)co * g.ovol + ((int64_t)d * g.O[1] + h) * g.O[2] + w];
}

// BWD_W B operand: column n = (ci, kd, kh, kw) (or the bias column) fixed per thread and tile
struct Tap3 {
  int64_t coff;   // ci ivol
  int kd, kh, kw;
  int kind;       // 0 out of range, 1 tap, 2 bias column
};

__device__ __forceinline__ Tap3 decode_tap(const Conv3Args& g, int ng) {
  Tap3 t{0, 0, 0, 0, 0};
  const int nw = g.Ci * g.kvol;
  if (ng < nw) {
    const int ci = (int)g.dKvol.div((unsigned)ng), r = ng - ci * g.kvol;
    split3(r, g.dK12, g.dK2, g.Kk[1] * g.Kk[2], g.Kk[2], t.kd, t.kh, t.kw);
    t.coff = (int64_t)ci * g.ivol;
    t.kind = 1;
  } else if (ng == nw) {
    t.kind = 2;
  }
  return t;
}

template <int MODE, int BM, int BN>
__global__ __launch_bounds__(256) void conv3d_igemm_kernel(const float* __restrict__ pa,
                                                           const float* __restrict__ pb,
                                                           const float* __restrict__ bias,
                                                           float* __restrict__ out, Conv3Args g) {
  constexpr int EA = BM * BK / 256, EB = BN * BK / 256;  // loads per thread per K step (A, B)
  constexpr int AR = 256 / BK;                     // A rows (BWD_W: B columns) per load round
  constexpr int MI = BM / 2 / MF, NJ = BN / 2 / MF;  // MFMA blocks per wave
  constexpr int KS = 256 / BN;                     // k stride of a thread's B loads
  __shared__ float As[2][BM * SK];
  __shared__ float Bs[2][BN * SK];
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = uniform_int(tid >> 6);
  const int wm = wave >> 1, wn = wave & 1;
  const int cm = lane % MF, gm = lane / MF;         // block row / column, k group
  const int m0 = blockIdx.y * BM, n0 = blockIdx.x * BN;
  // blockIdx.z: the K split (FWD, BWD_W), or class + nph x split (BWD_D).  Split FWD / BWD_D
  // launches write partial output slabs (out + split x slab), reduced afterwards in split order;
  // a split past a class's K writes its zeros (every slab covers every voxel of the class)
  const int split = MODE == BWD_D ? (int)blockIdx.z / g.nph : (int)blockIdx.z;
  const Phase3& ph = g.phase[MODE == BWD_D ? (int)blockIdx.z - split * g.nph : 0];
  if (MODE == BWD_D && n0 >= ph.Ncol) return;        // this class has fewer voxels (whole block)
  const int kbeg = split * g.kchunk;
  const int kend = min(MODE == BWD_D ? ph.K : g.K, kbeg + g.kchunk);
  if (MODE != BWD_W) out += (int64_t)split * g.slab;
  const int nk = kend > kbeg ? (kend - kbeg + BK - 1) / BK : 0;

  // loader roles.  A: k = tid % 16 (contiguous in memory for all modes), m = tid / 16 + 16 e.
  // B (FWD / BWD_D): voxel n = tid % BN fixed for the tile, k = tid / BN + (256 / BN) e.
  // B (BWD_W): voxel k = tid % 16, column n = tid / 16 + 16 e (fixed taps for the tile).
  const int ak = tid % BK, am = tid / BK;
  const int bn = tid % BN, bk = tid / BN;
  Vox vox{};
  Tap3 taps[EB];
  if (MODE != BWD_W) {
    vox = decode_vox<MODE>(g, ph, n0 + bn);
  } else {
#pragma unroll
    for (int e = 0; e < EB; ++e) taps[e] = decode_tap(g, n0 + am + AR * e);
  }

  // register staging: loads run one K-step ahead of the MFMAs
  float ra[EA], rb[EB];
  auto gload = [&](int kt) {
    const int k0 = kbeg + kt * BK;
#pragma unroll
    for (int e = 0; e < EA; ++e) ra[e] = load_a<MODE>(pa, g, ph, m0 + am + AR * e, k0 + ak, kend);
    if (MODE != BWD_W) {
#pragma unroll
      for (int e = 0; e < EB; ++e) rb[e] = load_b_vox<MODE>(pb, g, ph, vox, k0 + bk + KS * e, kend);
    } else {
      const int kg = k0 + ak;                          // this thread's output voxel
      const bool kok = kg < kend;
      const int v = kok ? kg : 0;
      const int n = (int)g.dOvol.div((unsigned)v), q = v - n * g.ovol;
      int od, oh, ow;
      split3(q, g.dO12, g.dO2, g.O[1] * g.O[2], g.O[2], od, oh, ow);
      const int64_t xb = (int64_t)n * g.Ci * g.ivol;
      const int d0 = od * g.s[0] - g.p[0], h0 = oh * g.s[1] - g.p[1], w0 = ow * g.s[2] - g.p[2];
#pragma unroll
      for (int e = 0; e < EB; ++e) {
        float v2 = 0.f;
        if (kok && taps[e].kind == 1) {
          const int d = d0 + taps[e].kd, h = h0 + taps[e].kh, w = w0 + taps[e].kw;
          if ((unsigned)d < (unsigned)g.I[0] && (unsigned)h < (unsigned)g.I[1] &&
              (unsigned)w < (unsigned)g.I[2])
            v2 = pb[xb + taps[e].coff + ((int64_t)d * g.I[1] + h) * g.I[2] + w];
        } else if (kok && taps[e].kind == 2) {
          v2 = 1.f;
        }
        rb[e] = v2;
      }
    }
  };
  auto sstore = [&](int buf) {
#pragma unroll
    for (int e = 0; e < EA; ++e) As[buf][(am + AR * e) * SK + ak] = ra[e];
    if (MODE != BWD_W) {
#pragma unroll
      for (int e = 0; e < EB; ++e) Bs[buf][bn * SK + bk + KS * e] = rb[e];
    } else {
#pragma unroll
      for (int e = 0; e < EB; ++e) Bs[buf][(am + AR * e) * SK + ak] = rb[e];
    }
  };

  f32x4 acc[MI][NJ];
#pragma unroll
  for (int i = 0; i < MI; ++i)
#pragma unroll
    for (int j = 0; j < NJ; ++j)
#pragma unroll
      for (int r = 0; r < NR; ++r) acc[i][j][r] = 0.f;

  if (nk > 0) {
    gload(0);
    sstore(0);
    __syncthreads();
    for (int kt = 0; kt < nk; ++kt) {
      const int cur = kt & 1;
      if (kt + 1 < nk) gload(kt + 1);
      const float* as = As[cur];
      const float* bs = Bs[cur];
      // lane (cm, gm) supplies k = 4 gm + s in MFMA step s: one 16-B read per block (the MFMA K
      // order is permuted consistently for A and B)
      f32x4 av[MI], bv[NJ];
#pragma unroll
      for (int i = 0; i < MI; ++i)
        av[i] = *reinterpret_cast<const f32x4*>(as + (wm * (BM / 2) + i * MF + cm) * SK + 4 * gm);
#pragma unroll
      for (int j = 0; j < NJ; ++j)
        bv[j] = *reinterpret_cast<const f32x4*>(bs + (wn * (BN / 2) + j * MF + cm) * SK + 4 * gm);
#pragma unroll
      for (int st = 0; st < 4; ++st)
#pragma unroll
        for (int i = 0; i < MI; ++i)
#pragma unroll
          for (int j = 0; j < NJ; ++j)
            acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[i][st], bv[j][st], acc[i][j], 0, 0, 0);
      if (kt + 1 < nk) sstore(cur ^ 1);
      __syncthreads();
    }
  }

  // epilogue: lane holds rows 4 gm + r of column cm of each MF x MF block
#pragma unroll
  for (int j = 0; j < NJ; ++j) {
    const int ng = n0 + wn * (BN / 2) + j * MF + cm;
    if (ng >= (MODE == BWD_D ? ph.Ncol : g.Ncol)) continue;
    if (MODE == BWD_W) {
#pragma unroll
      for (int i = 0; i < MI; ++i)
#pragma unroll
        for (int r = 0; r < NR; ++r) {
          const int mg = m0 + wm * (BM / 2) + i * MF + 4 * gm + r;
          if (mg < g.M) out[((int64_t)blockIdx.z * g.M + mg) * g.Ncol + ng] = acc[i][j][r];
        }
    } else if (MODE == FWD) {
      const int n = (int)g.dOvol.div((unsigned)ng), q = ng - n * g.ovol;
#pragma unroll
      for (int i = 0; i < MI; ++i)
#pragma unroll
        for (int r = 0; r < NR; ++r) {
          const int mg = m0 + wm * (BM / 2) + i * MF + 4 * gm + r;
          if (mg < g.M)
            out[((int64_t)n * g.M + mg) * g.ovol + q] = acc[i][j][r] + (bias && split == 0 ? bias[mg] : 0.f);
        }
    } else {
      const int64_t o0 = dx_offset(g, ph, ng);
#pragma unroll
      for (int i = 0; i < MI; ++i)
#pragma unroll
        for (int r = 0; r < NR; ++r) {
          const int mg = m0 + wm * (BM / 2) + i * MF + 4 * gm + r;
          if (mg < g.M) out[o0 + (int64_t)mg * g.ivol] = acc[i][j][r];
        }
    }
  }
}

struct Geom3 {
  int N, Ci, Di, Hi, Wi, Co, KD, KH, KW, sd, sh, sw, pd, ph, pw;
};

bool make_args(Conv3Args& g, const Geom3& q) {
  const int I[3] = {q.Di, q.Hi, q.Wi}, Kk[3] = {q.KD, q.KH, q.KW}, s[3] = {q.sd, q.sh, q.sw},
            p[3] = {q.pd, q.ph, q.pw};
  if (q.N < 1 || q.Ci < 1 || q.Co < 1) return false;
  int64_t ivol = 1, ovol = 1, kvol = 1;
  for (int a = 0; a < 3; ++a) {
    if (I[a] < 1 || Kk[a] < 1 || s[a] < 1 || p[a] < 0) return false;
    const int64_t num = (int64_t)I[a] + 2 * (int64_t)p[a] - Kk[a];
    if (num < 0) return false;                       // output extent < 1
    const int64_t O = num / s[a] + 1;
    if (O >= INT32_MAX || (int64_t)I[a] + p[a] >= INT32_MAX) return false;
    g.I[a] = I[a]; g.O[a] = (int)O; g.Kk[a] = Kk[a]; g.s[a] = s[a]; g.p[a] = p[a];
    ivol *= I[a];
    ovol *= O;
    kvol *= Kk[a];
    if (ivol >= INT32_MAX || ovol >= INT32_MAX || kvol >= INT32_MAX) return false;
  }
  // every GEMM extent and tensor size below 2^31 (32-bit voxel / k indices, FastDiv range)
  const int64_t lim = INT32_MAX;
  if (q.N * ivol >= lim || q.Ci * ivol >= lim || q.N * q.Ci * ivol >= lim) return false;
  if (q.N * ovol >= lim || q.Co * ovol >= lim || q.N * q.Co * ovol >= lim) return false;
  if (q.Ci * kvol >= lim - 1 || q.Co * kvol >= lim || (int64_t)q.Co * q.Ci * kvol >= lim) return false;
  g.N = q.N; g.Ci = q.Ci; g.Co = q.Co;
  g.ivol = (int)ivol; g.ovol = (int)ovol; g.kvol = (int)kvol;
  g.kchunk = 0;
  g.nph = 1;
  g.slab = 0;
  g.dKvol = FastDiv::make((unsigned)kvol);
  g.dK12 = FastDiv::make((unsigned)(Kk[1] * Kk[2]));
  g.dK2 = FastDiv::make((unsigned)Kk[2]);
  g.dOvol = FastDiv::make((unsigned)ovol);
  g.dO12 = FastDiv::make((unsigned)(g.O[1] * g.O[2]));
  g.dO2 = FastDiv::make((unsigned)g.O[2]);
  return true;
}

// 128 x 128 tiles where the GEMM has the rows and enough column tiles (over all stride-phase
// classes) to fill the chip; 64 x 64 otherwise (conv.hip's rule)
bool big_tiles(int mode, int M, int Ncol, int classes) {
  if (M < 128 || Ncol < 128) return false;
  if (mode == BWD_W || (mode == FWD && Ncol >= 512)) return true;
  return (int64_t)cdiv(M, 128) * cdiv(Ncol, 128) * classes >= 512;
}

template <int MODE>
void launch_igemm(int nz, int M, int Ncol, const float* pa, const float* pb, const float* bias,
                  float* out, const Conv3Args& g, hipStream_t st) {
  if (big_tiles(MODE, M, Ncol, MODE == BWD_D ? g.nph : 1)) {
    const dim3 g3(cdiv(Ncol, 128), cdiv(M, 128), nz);
    conv3d_igemm_kernel<MODE, 128, 128><<<g3, 256, 0, st>>>(pa, pb, bias, out, g);
  } else {
    const dim3 g3(cdiv(Ncol, 64), cdiv(M, 64), nz);
    conv3d_igemm_kernel<MODE, 64, 64><<<g3, 256, 0, st>>>(pa, pb, bias, out, g);
  }
}

// grid limits of a launch (x is unbounded in practice; y, z <= 65535)
bool grid_ok(int M, int nz) { return cdiv(M, 64) <= 65535 && nz >= 1 && nz <= 65535; }

// FWD / BWD_D: split K when the output tiles leave the chip short of workgroups (the encoder's
// last layers).  Aim at >= 1024 workgroups with >= 16 K-steps per split.
int dk_splits(int mode, int M, int Ncol, int K, int classes) {
  const int T = big_tiles(mode, M, Ncol, classes) ? 128 : 64;
  const int64_t tiles = (int64_t)cdiv(M, T) * cdiv(Ncol, T) * classes;
  if (tiles >= 512) return 1;
  int64_t s = cdiv(1024, tiles);
  const int64_t maxs = cdiv(K, 16 * BK);
  if (s > maxs) s = maxs;
  if (s > 16) s = 16;
  return (int)(s < 1 ? 1 : s);
}

// BWD_W: aim at >= 4096 workgroups with >= 8 K-steps per split (conv.hip's measured rule)
int wgrad_splits(const Conv3Args& g) {
  const int T = big_tiles(BWD_W, g.M, g.Ncol, 1) ? 128 : 64;
  const int64_t tiles = (int64_t)cdiv(g.M, T) * cdiv(g.Ncol, T);
  int64_t s = cdiv(4096, tiles);
  const int64_t maxs = cdiv(cdiv(g.K, BK), 8);
  if (s > maxs) s = maxs;
  if (s > 1024) s = 1024;
  return (int)(s < 1 ? 1 : s);
}

bool fwd_args(Conv3Args& g, const Geom3& q) {
  if (!make_args(g, q)) return false;
  g.M = g.Co;
  g.Ncol = g.N * g.ovol;
  g.K = g.Ci * g.kvol;
  g.kchunk = cdiv(g.K, BK) * BK;
  g.slab = (int64_t)g.N * g.Co * g.ovol;
  return true;
}

// stride-phase classes of BWD_D; returns the largest class's voxel count (-1: invalid), and
// *uncovered when some voxels' classes have no taps (they receive no gradient: only when a
// stride exceeds its kernel extent)
int bwd_data_args(Conv3Args& g, const Geom3& q, bool* uncovered) {
  if (q.sd < 1 || q.sh < 1 || q.sw < 1 || (int64_t)q.sd * q.sh * q.sw > kMaxPhases) return -1;
  if (!make_args(g, q)) return -1;
  g.M = g.Ci;
  g.Ncol = g.N * g.ivol;
  g.K = g.Co * g.kvol;
  g.nph = g.s[0] * g.s[1] * g.s[2];
  g.slab = (int64_t)g.N * g.Ci * g.ivol;
  int maxcol = 1, maxk = BK;
  *uncovered = false;
  for (int c = 0; c < g.nph; ++c) {
    Phase3& p = g.phase[c];
    const int r[3] = {c / (g.s[1] * g.s[2]), (c / g.s[2]) % g.s[1], c % g.s[2]};
    int cv = 1, nt = 1;
    for (int a = 0; a < 3; ++a) {
      const int s = g.s[a];
      p.r[a] = r[a];
      p.i0[a] = ((r[a] - g.p[a]) % s + s) % s;
      p.c[a] = p.i0[a] < g.I[a] ? (g.I[a] - p.i0[a] + s - 1) / s : 0;
      p.nk[a] = r[a] < g.Kk[a] ? (g.Kk[a] - r[a] + s - 1) / s : 0;
      p.o0[a] = (p.i0[a] + g.p[a] - r[a]) / s;
      cv *= p.c[a];
      nt *= p.nk[a];
    }
    p.Ncol = g.N * cv;
    p.K = g.Co * nt;
    if (p.K == 0 && p.Ncol > 0) *uncovered = true;
    if (p.K == 0) p.Ncol = 0;
    auto fd = [](int v) { return FastDiv::make((unsigned)(v > 0 ? v : 1)); };
    p.dC = fd(cv);
    p.dC12 = fd(p.c[1] * p.c[2]);
    p.dC2 = fd(p.c[2]);
    p.dT = fd(nt);
    p.dT12 = fd(p.nk[1] * p.nk[2]);
    p.dT2 = fd(p.nk[2]);
    if (p.Ncol > maxcol) maxcol = p.Ncol;
    if (p.K > maxk) maxk = p.K;
  }
  g.kchunk = cdiv(maxk, BK) * BK;
  return maxcol;
}

// the K range of each of nsplit splits (multiple of BK); the number of splits that remain
int set_split(Conv3Args& g, int nsplit) {
  const int kmax = g.kchunk;
  g.kchunk = cdiv(cdiv(kmax, nsplit), BK) * BK;
  return cdiv(kmax, g.kchunk);
}

bool wgrad_args(Conv3Args& g, const Geom3& q) {
  if (!make_args(g, q)) return false;
  g.M = g.Co;
  g.Ncol = g.Ci * g.kvol + 1;
  g.K = g.N * g.ovol;
  return true;
}

}  // namespace

#define GEOM3_PARAMS                                                                            \
  int N, int Ci, int Di, int Hi, int Wi, int Co, int KD, int KH, int KW, int sd, int sh, int sw, \
      int pd, int ph, int pw
#define GEOM3_VALUES \
  Geom3 { N, Ci, Di, Hi, Wi, Co, KD, KH, KW, sd, sh, sw, pd, ph, pw }

BLINDNO_API int blindno_conv3d_fwd_nsplit(GEOM3_PARAMS) {
  Conv3Args g;
  if (!fwd_args(g, GEOM3_VALUES)) return -1;
  return dk_splits(FWD, g.M, g.Ncol, g.K, 1);
}

BLINDNO_API int blindno_conv3d_fwd(const float* x, const float* w, const float* b, float* y,
                                   float* partial, int nsplit, GEOM3_PARAMS, void* stream) {
  Conv3Args g;
  if (!x || !w || !y || nsplit < 1 || (nsplit > 1 && !partial) || !fwd_args(g, GEOM3_VALUES))
    return (int)hipErrorInvalidValue;
  const int nz = set_split(g, nsplit);
  if (!grid_ok(g.M, nz) || (nz > 1 && g.slab >= INT32_MAX / nz)) return (int)hipErrorInvalidValue;
  hipStream_t st = (hipStream_t)stream;
  launch_igemm<FWD>(nz, g.M, g.Ncol, w, x, b, nz > 1 ? partial : y, g, st);
  const int e = (int)hipGetLastError();
  if (e || nz == 1) return e;
  return blindno_reduce_partials(partial, y, nz, (int)g.slab, stream);
}

BLINDNO_API int blindno_conv3d_bwd_data_nsplit(GEOM3_PARAMS) {
  Conv3Args g;
  bool unc;
  const int maxcol = bwd_data_args(g, GEOM3_VALUES, &unc);
  if (maxcol < 0) return -1;
  return dk_splits(BWD_D, g.M, maxcol, g.kchunk, g.nph);
}

BLINDNO_API int blindno_conv3d_bwd_data(const float* dy, const float* w, float* dx, float* partial,
                                        int nsplit, GEOM3_PARAMS, void* stream) {
  Conv3Args g;
  bool uncovered;
  if (!dy || !w || !dx || nsplit < 1 || (nsplit > 1 && !partial)) return (int)hipErrorInvalidValue;
  const int maxcol = bwd_data_args(g, GEOM3_VALUES, &uncovered);
  if (maxcol < 0) return (int)hipErrorInvalidValue;
  const int nz = set_split(g, nsplit);
  if (!grid_ok(g.M, g.nph * nz) || (nz > 1 && g.slab >= INT32_MAX / nz))
    return (int)hipErrorInvalidValue;
  float* out = nz > 1 ? partial : dx;
  hipStream_t st = (hipStream_t)stream;
  if (uncovered) {
    const hipError_t e = hipMemsetAsync(out, 0, sizeof(float) * (size_t)g.slab * nz, st);
    if (e != hipSuccess) return (int)e;
  }
  launch_igemm<BWD_D>(g.nph * nz, g.M, maxcol, w, dy, nullptr, out, g, st);
  const int e = (int)hipGetLastError();
  if (e || nz == 1) return e;
  return blindno_reduce_partials(partial, dx, nz, (int)g.slab, stream);
}

BLINDNO_API int blindno_conv3d_wgrad_nsplit(GEOM3_PARAMS) {
  Conv3Args g;
  if (!wgrad_args(g, GEOM3_VALUES)) return -1;
  return wgrad_splits(g);
}

BLINDNO_API int blindno_conv3d_bwd_weight(const float* dy, const float* x, float* dwb,
                                          float* partial, int nsplit, GEOM3_PARAMS, void* stream) {
  Conv3Args g;
  if (!dy || !x || !dwb || nsplit < 1 || (nsplit > 1 && !partial) || !wgrad_args(g, GEOM3_VALUES))
    return (int)hipErrorInvalidValue;
  g.kchunk = cdiv(cdiv(g.K, nsplit), BK) * BK;
  const int nz = cdiv(g.K, g.kchunk);
  if (!grid_ok(g.M, nz) || (int64_t)g.M * g.Ncol >= INT32_MAX / nz) return (int)hipErrorInvalidValue;
  hipStream_t st = (hipStream_t)stream;
  launch_igemm<BWD_W>(nz, g.M, g.Ncol, dy, x, nullptr, nz > 1 ? partial : dwb, g, st);
  const int e = (int)hipGetLastError();
  if (e || nz == 1) return e;
  return blindno_reduce_partials(partial, dwb, nz, g.M * g.Ncol, stream);
}
