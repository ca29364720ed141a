/* libblindno C ABI, part 12: physics attention of the structured-mesh Transolver and the LayerNorm
 * over channel planes (the snapshot encoder of NIOFP2D_Trans).
 *
 * Included by blindno.h (include that one); same conventions: every entry returns a hipError_t
 * code as int (0 = success) unless it is a size query, pointers are device pointers, the last
 * argument is the stream, nothing is allocated and nothing synchronises inside.  The Python
 * binding keeps these entries in blindno._lib.ABI["blindno_physattn.h"].
 */
#ifndef BLINDNO_PHYSATTN_H
#define BLINDNO_PHYSATTN_H

#include "blindno.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Physics_Attention_Structured_Mesh_2D.forward (model/Physics_Attention.py:88-116) after its two
 * 3x3 convolutions, as NIOFP2D_Trans builds it (2d_FPE/NIOModules.py:104-116): 4 heads h, D = 8
 * channels per head, G = 16 slices, 32 channels; fp32.  Activations are channel planes, the layout
 * of blindno_conv2d_*: xm, fm (S, 32, N) with N = H W and sstride floats between two snapshots
 * (32 N for separate tensors, 64 N for the two halves of one 64-channel convolution output); head h
 * owns channels 8 h .. 8 h + 7.  Per snapshot s and head h:
 *     w[n, g]   = softmax_g((Ws xm_h[n] + bs)[g] / clamp(temperature[h], 0.1, 5))
 *     norm[g]   = sum_n w[n, g]
 *     tok[g, :] = sum_n w[n, g] fm_h[n, :] / (norm[g] + 1e-5)
 *     q, k, v   = tok Wq^T, tok Wk^T, tok Wv^T;  A = softmax(q k^T / sqrt(8));  otok = A v
 *     ox[n, 8 h + c] = sum_g w[n, g] otok[g, c]
 *     y[n, :]   = Wo ox[n, :] + bo (+ res[n, :])
 * Ws (16, 8), bs (16), Wq / Wk / Wv (8, 8) are shared by the heads; Wo (32, 32), bo (32);
 * temperature (4).  y, res (S, 32, N) planes; res may be NULL.
 *
 * The kernels read N = H W points per snapshot and never the plane's shape, so the 3D structured
 * mesh (Physics_Attention_Structured_Mesh_3D, model/Physics_Attention.py:119-175, after its two
 * 3x3x3 convolutions) runs on the same entries: a grid (H, W, D) is passed as (H, W D).
 *
 * Three launches: a slice pass (a thread per point; w stored as (S, 4, 16, N) planes, partials of
 * norm and the unnormalised tokens per workgroup of 256 points), a token pass per (s, h) (partials
 * added in index order; writes tok (S, 4, 16, 8), norm (S, 4, 16), A (S, 4, 16, 16), otok
 * (S, 4, 16, 8), all kept for the backward) and a deslice pass (ox formed per point in registers
 * and never stored, to_out and the residual in the same thread).
 *
 * Backward from dy (S, 32, N): a first point pass (dox = dy Wo, kept in scratch for the second;
 * the partials of dotok[g, c] = sum_n w[n, g] dox[n, c], of dWo = dy^T ox and of dbo), the token
 * attention's backward per (s, h) (dtok and this (s, h)'s dWq, dWk, dWv), a second point pass
 *     dw[n, g] = sum_c otok[g, c] dox[n, c]
 *                + (sum_c fm[n, c] dtok[g, c] - sum_c tok[g, c] dtok[g, c]) / (norm[g] + 1e-5)
 * with the slice softmax backward, dfm, dxm and the partials of dWs, dbs, dtemperature (the clamp
 * passes the gradient where 0.1 <= temperature <= 5 and none outside, as torch.clamp), and one
 * launch that adds every partial table in index order.  dxm, dfm (S, 32, N) with dstride floats
 * between snapshots.  No atomics anywhere: two calls agree to the bit.
 *
 * Each entry returns hipErrorInvalidValue, with nothing launched, for S < 1, S > 65535, H < 1,
 * W < 1, H W > 2^24, a stride below 32 N or a NULL pointer (res excepted); the queries return -1
 * for such sizes (blindno_physattn_ok: 0). */

/* 1 where the kernels take the configuration (heads = 4, D = 8, G = 16 and a valid S, H, W). */
int blindno_physattn_ok(int S, int H, int W, int heads, int D, int G);
/* Workgroups per snapshot of the point passes (256 points each). */
int blindno_physattn_nblk(int H, int W);
/* Forward scratch: the token partials, S 4 nblk 144 floats. */
int64_t blindno_physattn_fwd_scratch_floats(int S, int H, int W);
int blindno_physattn_fwd(const float* xm, const float* fm, int64_t sstride,
                         const float* temperature, const float* Ws, const float* bs,
                         const float* Wq, const float* Wk, const float* Wv, const float* Wo,
                         const float* bo, const float* res, float* w, float* tok, float* norm,
                         float* A, float* otok, float* scratch, float* y, int S, int H, int W,
                         blindno_stream_t stream);
/* Backward scratch: dox (S 32 N), the dotok partials (S 4 nblk 144), the dWo / dbo partials
 * (S nblk 1056), dtok / (norm + 1e-5) (S 4 128), its tok term (S 4 16), the dWq / dWk / dWv
 * partials (S 4 192) and the dWs / dbs / dtemperature partials (S nblk 148) floats, in that
 * order; contents undefined afterwards. */
int64_t blindno_physattn_bwd_scratch_floats(int S, int H, int W);
int blindno_physattn_bwd(const float* dy, const float* xm, const float* fm, int64_t sstride,
                         const float* temperature, const float* Ws, const float* bs,
                         const float* Wq, const float* Wk, const float* Wv, const float* Wo,
                         const float* w, const float* tok, const float* norm, const float* A,
                         const float* otok, float* scratch, float* dxm, float* dfm,
                         int64_t dstride, float* dtemperature, float* dWs, float* dbs, float* dWq,
                         float* dWk, float* dWv, float* dWo, float* dbo, int S, int H, int W,
                         blindno_stream_t stream);

/* nn.LayerNorm(32) over the channel planes (model/Transolver_Structured_Mesh_2D.py:58,62,65):
 * x, y (S, C, HW) with C = 32, a thread per point; biased variance, eps inside the root.  mean,
 * rstd (S, HW) are written by the forward and read by the backward.  The backward's dgamma / dbeta
 * go through per-workgroup partials (S blindno_ln_planes_nblk(HW) 64 floats) added in index order.
 * hipErrorInvalidValue for C != 32, S < 1, S > 65535, HW < 1, HW > 2^24 or a NULL pointer. */
int blindno_ln_planes_nblk(int HW);
int blindno_ln_planes_fwd(const float* x, const float* gamma, const float* beta, float* y,
                          float* mean, float* rstd, int S, int C, int HW, float eps,
                          blindno_stream_t stream);
int blindno_ln_planes_bwd(const float* dy, const float* x, const float* gamma, const float* mean,
                          const float* rstd, float* dx, float* dgamma, float* dbeta,
                          float* partial, int S, int C, int HW, blindno_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* BLINDNO_PHYSATTN_H */
