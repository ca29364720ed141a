// Bag-level projection of the 3D snapshot encoder (NIOFP3D_FNO's FNO_input): the FNO3d
// projection (crop -> fc1 -> GELU -> fc2, 2d_FPE/FNOModules.py:360-364) of every snapshot of a
// bag fused with the fixed-weight bag mean that consumes it (the expression of
// 2d_FPE/NIOModules.py:565-575 with one more grid channel).  The kernels are the geometry
// templates of csrc/bagproj.h (16-point tiles over the flattened (bag, crop point) space, the
// hidden units split over the waves, the bag walked in LDS-staged chunks; fixed summation
// order, no read-modify-write on global memory: a second call is bit-identical); this file
// holds the 3D crop N1 x N2 x N3 out of P1 x P2 x P3 -- which is not a prefix of any 2D view of
// the field -- and its entry points (include/blindno_bag3d.h).
#include "bagproj.h"

#include "blindno_bag3d.h"

namespace {

// point f of the flattened (bag, crop point) space -> offset of (bag b, snapshot 0, channel 0,
// i, j, k) in z (B U, C, P1, P2, P3); 32-bit (the launchers bound the field below 2^31).  HW is
// the channel-volume stride P1 P2 P3 (the name the kernels use for it).
struct BagGeom3 {
  unsigned npts, S, N23, N3, P23, P3, HW, C, U;
  FastDiv dS, dN23, dN3;
  __device__ __forceinline__ unsigned base(unsigned f) const {
    const unsigned b = dS.div(f), s = f - b * S;
    const unsigned i = dN23.div(s), r = s - i * N23;
    const unsigned j = dN3.div(r), k = r - j * N3;
    return b * U * C * HW + i * P23 + j * P3 + k;
  }
};

bool bag_geom3(int B, int U, int C, int P1, int P2, int P3, int N1, int N2, int N3, int Hd,
               BagGeom3& g) {
  if (B < 1 || U < 1 || U > kMaxU || C < 1 || C > 4 || Hd != kHd || N1 < 1 || N2 < 1 || N3 < 1 ||
      N1 > P1 || N2 > P2 || N3 > P3)
    return false;
  const int64_t lim = (int64_t)1 << 31;
  if ((int64_t)B * U * C * P1 * P2 * P3 >= lim) return false;   // => B N1 N2 N3 < 2^31 as well
  g.S = (unsigned)(N1 * N2 * N3);
  g.npts = (unsigned)B * g.S;
  g.N23 = (unsigned)(N2 * N3);
  g.N3 = (unsigned)N3;
  g.P23 = (unsigned)(P2 * P3);
  g.P3 = (unsigned)P3;
  g.HW = (unsigned)(P1 * P2 * P3);
  g.C = (unsigned)C;
  g.U = (unsigned)U;
  g.dS = FastDiv::make(g.S);
  g.dN23 = FastDiv::make(g.N23);
  g.dN3 = FastDiv::make(g.N3);
  return true;
}

int64_t tiles3(int B, int N1, int N2, int N3) {
  return ((int64_t)B * N1 * N2 * N3 + 15) / 16;
}

}  // namespace

BLINDNO_API int64_t blindno_project_bag3d_stats_floats(int B, int N1, int N2, int N3) {
  return tiles3(B, N1, N2, N3) * (int64_t)kTileF4 * 4;
}

BLINDNO_API int blindno_project_bag3d_bwd_nchunk(int B, int N1, int N2, int N3) {
  const int64_t tiles = tiles3(B, N1, N2, N3);
  return (int)(tiles < 1 ? 1 : (tiles > 1024 ? 1024 : tiles));
}

BLINDNO_API int blindno_project_bag3d_fwd(const float* z, const float* w1, const float* b1,
                                          const float* w2, const float* b2, const float* lw,
                                          float* ubar, float* stats, float* v, int B, int U, int C,
                                          int P1, int P2, int P3, int N1, int N2, int N3, int Hd,
                                          void* stream) {
  BagGeom3 g;
  if (!bag_geom3(B, U, C, P1, P2, P3, N1, N2, N3, Hd, g) || !z || !w1 || !b1 || !w2 || !b2 ||
      !ubar || !stats || !v)
    return (int)hipErrorInvalidValue;
  const unsigned ntiles = (g.npts + 15) / 16;
  bagproj_fwd_kernel<BagGeom3><<<ntiles, 256, 0, (hipStream_t)stream>>>(z, w1, b1, w2, b2, lw, ubar,
                                                                        stats, v, g);
  return (int)hipGetLastError();
}

BLINDNO_API int blindno_project_bag3d_bwd(const float* stats, const float* gs, const float* w2,
                                          const float* lw, const float* v, float* dz,
                                          float* partial, int nchunk, int B, int U, int C, int P1,
                                          int P2, int P3, int N1, int N2, int N3, int Hd,
                                          void* stream) {
  BagGeom3 g;
  if (!bag_geom3(B, U, C, P1, P2, P3, N1, N2, N3, Hd, g) || !stats || !gs || !w2 || !v || !dz ||
      !partial || nchunk < 1)
    return (int)hipErrorInvalidValue;
  hipStream_t st = (hipStream_t)stream;
  // dz is zero on the padding (the 3D layer adjoints read the whole field): the field is
  // cleared, the kernel writes the crop
  const int e = (int)hipMemsetAsync(dz, 0, sizeof(float) * (size_t)B * U * C * g.HW, st);
  if (e) return e;
  bagproj_bwd_kernel<BagGeom3><<<nchunk, 256, 0, st>>>(stats, gs, w2, lw, v, dz, partial, g);
  return (int)hipGetLastError();
}
