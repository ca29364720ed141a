/* libblindno C ABI: the bag-level projection of the 3D snapshot encoder (NIOFP3D_FNO).
 *
 * Included by blindno.h (include that one); same conventions: every entry returns a hipError_t
 * code as int (0 = success) unless it is a size query, pointers are device pointers, the last
 * argument is the stream.  The Python binding keeps these entries in
 * blindno._lib.ABI["blindno_bag3d.h"].
 */
#ifndef BLINDNO_BAG3D_H
#define BLINDNO_BAG3D_H

#include "blindno.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The 3D counterpart of blindno_project_bag_fwd / _bwd: FNO3d's projection (crop + fc1 + GELU +
 * fc2, 2d_FPE/FNOModules.py:360-364) of the U snapshots of each of B bags fused with the
 * fixed-weight bag mean that consumes it (2d_FPE/NIOModules.py:565-575 with a third grid
 * channel).  z (B U, C, P1, P2, P3): the last encoder layer (snapshot n = b U + l), cropped to
 * N1 x N2 x N3 (any P >= N per axis); lw (U) the snapshot weights (multiplicity / L; NULL:
 * 1 / U).  C <= 4, Hd = 128, one output channel, U <= 1024.  Offsets are 32-bit: with
 * B U C P1 P2 P3 >= 2^31 (or any other invalid argument) the entries return
 * hipErrorInvalidValue and launch nothing.  Forward writes
 *   ubar (B, N1 N2 N3) = sum_l lw_l fc2(GELU(fc1(z_l)))   (the bag mean of the projections),
 *   stats (blindno_project_bag3d_stats_floats(B, N1, N2, N3) floats): per 16-point tile of the
 *         flattened (bag, crop point) space the bag-level sums A = sum lw GELU(h),
 *         S = sum lw GELU'(h), Q = sum lw GELU'(h) z^T  (3 KiB per point),
 *   v (B U, C, P1, P2, P3) on the crop: W1^T (w2 * GELU'(h)) per snapshot point (the padding is
 *         left unwritten).
 * Backward: gs (B, N1 N2 N3) = the gradient of ubar; writes dz (B U, C, P1, P2, P3) =
 * lw_l gs v on the crop and 0 on the padding, and per-workgroup partials
 * [dW1 (Hd*C) | db1 (Hd) | dW2 (Hd) | db2] into partial[nchunk][...] for
 * blindno_reduce_partials, nchunk = blindno_project_bag3d_bwd_nchunk(B, N1, N2, N3) (any
 * value >= 1).  Fixed summation order: a second call gives the same bits. */
int64_t blindno_project_bag3d_stats_floats(int B, int N1, int N2, int N3);
int blindno_project_bag3d_bwd_nchunk(int B, int N1, int N2, int N3);
int blindno_project_bag3d_fwd(const float* z, const float* w1, const float* b1, const float* w2,
                              const float* b2, const float* lw, float* ubar, float* stats,
                              float* v, int B, int U, int C, int P1, int P2, int P3, int N1, int N2,
                              int N3, int Hd, blindno_stream_t stream);
int blindno_project_bag3d_bwd(const float* stats, const float* gs, const float* w2, const float* lw,
                              const float* v, float* dz, float* partial, int nchunk, int B, int U,
                              int C, int P1, int P2, int P3, int N1, int N2, int N3, int Hd,
                              blindno_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* BLINDNO_BAG3D_H */
