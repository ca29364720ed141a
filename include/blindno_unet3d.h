/* libblindno C ABI: the 3D kernels of the attention UNet, PermInvUNet_attn3D (csrc/unet3d.hip).
 *
 * Included by blindno.h (include that one); same conventions: every entry returns a hipError_t
 * code as int (0 = success) unless it is a size query, pointers are device pointers, tensors are
 * NCDHW fp32, the last argument is the stream.  NULL tensors (a bias excepted), sizes < 1 and
 * unsupported kernel extents return hipErrorInvalidValue and launch nothing.  Every reduction is
 * a fixed-order tree or per-chunk partials summed in chunk order by blindno_reduce_partials: no
 * float atomics, a second call is bit-identical.  Offsets are 64-bit; one (n, c) volume must
 * stay below 2^31 voxels.  The Python binding keeps these entries in
 * blindno._lib.ABI["blindno_unet3d.h"].
 *
 * The rest of the 3D UNet runs on entries that take a 3D field unchanged: blindno_conv3d_* (the
 * 3x3x3 and 1x1x1 convolutions), blindno_cnx_pw_* and blindno_bn_act_* with HW = D H W, and
 * blindno_tok_attn_* with D = C D H W.
 */
#ifndef BLINDNO_UNET3D_H
#define BLINDNO_UNET3D_H

#include "blindno.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- depthwise convolution (ConvNeXtBlock3D.dwconv: nn.Conv3d(C, C, K, padding K/2, groups C)):
 *   y[n][c][d][h][w] = b[c] + sum_{i,j,k} W[c][i][j][k] x[n][c][d+i-KD/2][h+j-KH/2][w+k-KW/2]
 * with zero padding; KD, KH, KW each odd and <= 7, not necessarily equal.  x, y (N, C, D, H, W),
 * w (C, KD, KH, KW), b (C) or NULL.
 *   bwd_data:   dx = the same kernel on the point-reflected taps (exact for odd extents with
 *               same padding), no bias
 *   bwd_weight: dwb (C, KD KH KW + 1): columns [0, KD KH KW) = dW, the last column = db.  The
 *               (n, tile) work items of a channel are cut into nsplit ranges; with nsplit > 1
 *               the range sums go to partial (nsplit x C x (KD KH KW + 1) floats) and are summed
 *               in range order.  Any nsplit >= 1 is valid; blindno_dwconv3d_wgrad_nsplit gives
 *               the count that fills the chip (-1 for an invalid geometry). */
int blindno_dwconv3d_fwd(const float* x, const float* w, const float* b, float* y, int N, int C,
                         int D, int H, int W, int KD, int KH, int KW, blindno_stream_t stream);
int blindno_dwconv3d_bwd_data(const float* dy, const float* w, float* dx, int N, int C, int D,
                              int H, int W, int KD, int KH, int KW, blindno_stream_t stream);
int blindno_dwconv3d_wgrad_nsplit(int N, int C, int D, int H, int W, int KD, int KH, int KW);
int blindno_dwconv3d_bwd_weight(const float* dy, const float* x, float* dwb, float* partial,
                                int nsplit, int N, int C, int D, int H, int W, int KD, int KH,
                                int KW, blindno_stream_t stream);

/* ---- max pool (nn.MaxPool3d(2)): window = stride = KD x KH x KW, each 1 or 2, floor:
 * x (NC, D, H, W) -> y, arg (NC, D/KD, H/KH, W/KW); arg (uint8) is the tap index
 * (i KH + j) KW + k of the maximum in (d, h, w) scan order -- the first maximum wins and a NaN
 * wins (torch's rules).  bwd writes every voxel of dx (NC, D, H, W) once: dy where the voxel is
 * its window's argmax, 0 elsewhere and on the planes the floor drops. */
int blindno_maxpool3d_fwd(const float* x, float* y, uint8_t* arg, int NC, int D, int H, int W,
                          int KD, int KH, int KW, blindno_stream_t stream);
int blindno_maxpool3d_bwd(const float* dy, const uint8_t* arg, float* dx, int NC, int D, int H,
                          int W, int KD, int KH, int KW, blindno_stream_t stream);

/* ---- transposed convolution (nn.ConvTranspose3d(Ci, Co, kernel = stride = 2, output_padding)):
 * x (N, Ci, Di, Hi, Wi), w (Ci, Co, 2, 2, 2), b (Co) or NULL -> y (N, Co, Do, Ho, Wo) with
 * 2 Di <= Do < 2 (Di + 1) and likewise Ho, Wo; the planes past 2 Di (output_padding) receive
 * the bias only and give no gradient to x or w.
 *   bwd_weight: dwb = [dW (Ci Co 8) | db (Co)]; partial: blindno_convt3d_wgrad_nparts(N, Di, Hi,
 *               Wi) x (Ci Co 8 + Co) floats, summed in part order. */
int blindno_convt3d_fwd(const float* x, const float* w, const float* b, float* y, int N, int Ci,
                        int Di, int Hi, int Wi, int Co, int Do, int Ho, int Wo,
                        blindno_stream_t stream);
int blindno_convt3d_bwd_data(const float* dy, const float* w, float* dx, int N, int Ci, int Di,
                             int Hi, int Wi, int Co, int Do, int Ho, int Wo,
                             blindno_stream_t stream);
int blindno_convt3d_wgrad_nparts(int N, int Di, int Hi, int Wi);
int blindno_convt3d_bwd_weight(const float* dy, const float* x, float* dwb, float* partial, int N,
                               int Ci, int Di, int Hi, int Wi, int Co, int Do, int Ho, int Wo,
                               blindno_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* BLINDNO_UNET3D_H */
