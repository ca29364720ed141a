/* libblindno C ABI, part 2: the 3D convolutions of the NIOFP3D snapshot encoders.
 *
 * Included by blindno.h (include that one); same conventions: every entry returns a hipError_t
 * code as int (0 = success) unless it is a size query, pointers are device pointers, the last
 * argument is the stream.  The Python binding keeps these entries in
 * blindno._lib.ABI["blindno_conv3d.h"].
 */
#ifndef BLINDNO_CONV3D_H
#define BLINDNO_CONV3D_H

#include "blindno.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- NIOFP3D snapshot encoder convolutions: nn.Conv3d (bias, groups 1, any kernel / stride /
 * zero padding per axis) of the ConvBlock3D layers (2d_FPE/Baselines.py:26-38; Encoder3D and
 * Encoder3D_down :322-429), replacing the MIOpen calls of torch.nn.Conv3d.  NCDHW fp32;
 * Do = (Di + 2 pd - KD) / sd + 1, Ho and Wo likewise.  Implicit GEMMs on the fp32 matrix cores
 * with a fixed accumulation order and no atomics (a second call is bit-identical); no im2col
 * buffer.  Every tensor and GEMM extent must stay below 2^31 elements; invalid arguments (NULL
 * tensors, sizes < 1, an output extent < 1, for bwd_data sd sh sw > 8) return
 * hipErrorInvalidValue (the *_nsplit queries: -1) and launch nothing.
 *   fwd:        y (N, Co, Do, Ho, Wo) = conv(x (N, Ci, Di, Hi, Wi), w (Co, Ci, KD, KH, KW)) + b
 *               (b may be NULL)
 *   bwd_data:   dx (N, Ci, Di, Hi, Wi) = conv^T(dy, w), one GEMM per stride-phase class; input
 *               voxels that no tap reaches (a stride above its kernel extent) get exactly 0
 *   bwd_weight: dwb (Co, Ci KD KH KW + 1): columns [0, Ci KD KH KW) = dW, last column = db
 * Each takes nsplit >= 1: K (fwd: Ci KD KH KW, bwd_data: Co x a class's taps, bwd_weight: the
 * N Do Ho Wo output voxels) is cut into nsplit ranges whose partial results (partial: nsplit *
 * |y|, nsplit * |dx| or nsplit * |dwb| floats; NULL allowed when nsplit is 1) are summed in split
 * order by blindno_reduce_partials.  The *_nsplit queries give the count that fills the chip
 * (the encoder's last blocks have 1-3 output voxels per volume and K = 13824); any nsplit >= 1
 * is valid. */
int blindno_conv3d_fwd_nsplit(int N, int Ci, int Di, int Hi, int Wi, int Co, int KD, int KH, int KW,
                              int sd, int sh, int sw, int pd, int ph, int pw);
int blindno_conv3d_fwd(const float* x, const float* w, const float* b, float* y, float* partial,
                       int nsplit, int N, int Ci, int Di, int Hi, int Wi, int Co, int KD, int KH,
                       int KW, int sd, int sh, int sw, int pd, int ph, int pw,
                       blindno_stream_t stream);
int blindno_conv3d_bwd_data_nsplit(int N, int Ci, int Di, int Hi, int Wi, int Co, int KD, int KH,
                                   int KW, int sd, int sh, int sw, int pd, int ph, int pw);
int blindno_conv3d_bwd_data(const float* dy, const float* w, float* dx, float* partial, int nsplit,
                            int N, int Ci, int Di, int Hi, int Wi, int Co, int KD, int KH, int KW,
                            int sd, int sh, int sw, int pd, int ph, int pw,
                            blindno_stream_t stream);
int blindno_conv3d_wgrad_nsplit(int N, int Ci, int Di, int Hi, int Wi, int Co, int KD, int KH,
                                int KW, int sd, int sh, int sw, int pd, int ph, int pw);
int blindno_conv3d_bwd_weight(const float* dy, const float* x, float* dwb, float* partial,
                              int nsplit, int N, int Ci, int Di, int Hi, int Wi, int Co, int KD,
                              int KH, int KW, int sd, int sh, int sw, int pd, int ph, int pw,
                              blindno_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* BLINDNO_CONV3D_H */
