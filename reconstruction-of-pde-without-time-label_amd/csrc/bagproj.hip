// Bag-level projection of the snapshot encoder: the FNO_input projection (crop -> fc1 -> GELU
// -> fc2, 2d_FPE/FNOModules.py:234-239) of every snapshot of a bag fused with the fixed-weight
// bag mean that consumes it (2d_FPE/NIOModules.py:569-575), with the backward reduced to
// bag-level sufficient statistics.
//
// The bag mean hands every snapshot l of bag b the same upstream gradient up to its weight:
// dy[l, p] = lw_l ghat[b, p] (ghat = W'[:, 2] . dL/dh[b, p], lw_l = multiplicity / L).  With
// h = W1 z + b1 per snapshot point, a = GELU(h) and g = GELU'(h), every parameter gradient is
// therefore a ghat-weighted sum of per-(bag, point) statistics that the forward forms while h
// is in registers:
//     A[k] = sum_l lw_l a_k,   S[k] = sum_l lw_l g_k,   Q[k][c] = sum_l lw_l g_k z_c,
//     dW2 = sum_bp ghat A,  db1 = w2 * sum_bp ghat S,  dW1 = w2 * sum_bp ghat Q,
//     db2 = sum_bp ghat * sum_l lw_l,
// and the input gradient is dz[l, p, c] = lw_l ghat[b, p] v[l, p, c] with v = W1^T (w2 * g).
// The forward's output is the bag mean of the projections itself,
//     ubar[b, p] = sum_l lw_l (w2 . a_l + b2) = w2 . A + b2 sum_l lw_l,
// so no per-snapshot output is written, and the backward reads 3 KB of statistics per (bag,
// point) instead of recomputing fc1, GELU and GELU' for every snapshot point.
//
// Forward layout ("hidden x points", one v_mfma_f32_16x16x4f32 per 16 x 16 tile, K = C <= 4):
//     H (16 hid x 16 pts) = W1 (16 hid x C) . Z (C x 16 pts)
// lane l holds h for hidden units 4 (l >> 4) + r (r < 4) and point l & 15, so the lane's Q
// update needs only its own point's C channels and v reduces over the 4 lane groups (a
// reduce-scatter of 3 lane swaps) instead of over 16 lanes.  A workgroup owns a 16-point tile;
// its 4 waves split the 128 hidden units (2 tiles each, weights in registers) and walk the
// bag's snapshots in double-buffered chunks staged through LDS, where the waves' v partials are
// also summed.
// The kernels are the geometry templates of csrc/bagproj.h; this file holds the 2D crop and its
// entry points.
#include "bagproj.h"

namespace {

// point f of the flattened (bag, crop point) space -> offset of (bag b, snapshot 0, channel 0,
// row h, column w) in z (B U, C, P1, P2); 32-bit (the launchers bound the field below 2^31)
struct BagGeom {
  unsigned npts, S, Wo, P2, HW, C, U;
  FastDiv dS, dWo;
  __device__ __forceinline__ unsigned base(unsigned f) const {
    const unsigned b = dS.div(f), s = f - b * S;
    const unsigned h = dWo.div(s), w = s - h * Wo;
    return b * U * C * HW + h * P2 + w;
  }
};

bool bag_geom(int B, int U, int C, int P1, int P2, int Ho, int Wo, int Hd, BagGeom& g) {
  if (B < 1 || U < 1 || U > kMaxU || C < 1 || C > 4 || Hd != kHd || Ho < 1 || Wo < 1 || Ho > P1 ||
      Wo > P2)
    return false;
  if ((int64_t)B * U * C * P1 * P2 >= INT32_MAX || (int64_t)B * Ho * Wo >= INT32_MAX) return false;
  g.npts = (unsigned)(B * Ho * Wo);
  g.S = (unsigned)(Ho * Wo);
  g.Wo = (unsigned)Wo;
  g.P2 = (unsigned)P2;
  g.HW = (unsigned)(P1 * P2);
  g.C = (unsigned)C;
  g.U = (unsigned)U;
  g.dS = FastDiv::make(g.S);
  g.dWo = FastDiv::make(g.Wo);
  return true;
}

}  // namespace

#if BAGPROJ_PROBE
BLINDNO_API int blindno_bagproj_probe_read(unsigned long long* dst, int n) {
  return (int)hipMemcpyFromSymbol(dst, HIP_SYMBOL(g_bagproj_probe),
                                  sizeof(unsigned long long) * (size_t)n, 0, hipMemcpyDeviceToHost);
}
#endif

BLINDNO_API int64_t blindno_project_bag_stats_floats(int B, int Ho, int Wo) {
  return ((int64_t)B * Ho * Wo + 15) / 16 * (int64_t)kTileF4 * 4;
}

#ifndef BAGPROJ_BWD_BLOCKS
#define BAGPROJ_BWD_BLOCKS 1024
#endif
BLINDNO_API int blindno_project_bag_bwd_nchunk(int B, int Ho, int Wo) {
  const int64_t tiles = ((int64_t)B * Ho * Wo + 15) / 16;
  return (int)(tiles < 1 ? 1 : (tiles > BAGPROJ_BWD_BLOCKS ? BAGPROJ_BWD_BLOCKS : tiles));
}

BLINDNO_API int blindno_project_bag_fwd(const float* z, const float* w1, const float* b1,
                                        const float* w2, const float* b2, const float* lw,
                                        float* ubar, float* stats, float* v, int B, int U, int C,
                                        int P1, int P2, int Ho, int Wo, int Hd, void* stream) {
  BagGeom g;
  if (!bag_geom(B, U, C, P1, P2, Ho, Wo, Hd, g) || !z || !ubar || !stats || !v)
    return (int)hipErrorInvalidValue;
  const unsigned ntiles = (g.npts + 15) / 16;
  bagproj_fwd_kernel<BagGeom><<<ntiles, 256, 0, (hipStream_t)stream>>>(z, w1, b1, w2, b2, lw, ubar, stats,
                                                               v, g);
  return (int)hipGetLastError();
}

BLINDNO_API int blindno_project_bag_bwd(const float* stats, const float* gs, const float* w2,
                                        const float* lw, const float* v, float* dz,
                                        float* partial, int nchunk, int B, int U, int C, int P1,
                                        int P2, int Ho, int Wo, int Hd, void* stream) {
  BagGeom g;
  if (!bag_geom(B, U, C, P1, P2, Ho, Wo, Hd, g) || !stats || !gs || (dz && !v) || !partial ||
      nchunk < 1)
    return (int)hipErrorInvalidValue;
  bagproj_bwd_kernel<BagGeom><<<nchunk, 256, 0, (hipStream_t)stream>>>(stats, gs, w2, lw, v, dz, partial, g);
  return (int)hipGetLastError();
}
