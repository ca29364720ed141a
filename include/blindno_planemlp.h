/* libblindno C ABI, part 13: the fused per-point MLP over channel planes (the token MLPs of the
 * structured-mesh Transolver: ln_2 + mlp + residual of a block, and preprocess).
 *
 * Included by blindno.h (include that one); same conventions: every entry returns a hipError_t
 * code as int (0 = success) unless it is a size query, pointers are device pointers, the last
 * argument is the stream, nothing is allocated and nothing synchronises inside.  The Python
 * binding keeps these entries in blindno._lib.ABI["blindno_planemlp.h"].
 */
#ifndef BLINDNO_PLANEMLP_H
#define BLINDNO_PLANEMLP_H

#include "blindno.h"

#ifdef __cplusplus
extern "C" {
#endif

/* MLP(n_layers = 0).forward of model/Transolver_Structured_Mesh_{2D,3D}.py on the plane layout of
 * blindno_conv2d_* / blindno_conv3d_* / blindno_physattn_*: activations (S, C, N), N points per
 * snapshot, with an explicit number of floats between two snapshots (C N for a tensor of its own,
 * more for a channel slice of a wider one); fp32, a thread per point, 256 points per workgroup.
 *     u[n, :] = LayerNorm_C(x[n, :]) gamma + beta      with LayerNorm, else u[n, :] = x[n, :]
 *     y[n, :] = W2 gelu(W1 u[n, :] + b1) + b2 (+ res[n, :])
 * W1 (Chid, Cin), b1 (Chid), W2 (Cout, Chid), b2 (Cout): nn.Linear's layout.  LayerNorm: biased
 * variance, eps inside the root; GELU: the exact erf form.  Two configurations exist:
 *     (Cin, Chid, Cout) = (32, 32, 32) with LayerNorm     a block's ln_2 + mlp at mlp_ratio = 1
 *     (Cin, Chid, Cout) = (4, 64, 32) without LayerNorm   preprocess at space_dim + fun_dim = 4
 * res (S, Cout, N) may be NULL in both.  The hidden vector lives in registers and is never stored;
 * the forward keeps nothing but mean, rstd (S, N) when LayerNorm is on (NULL otherwise, as are
 * gamma and beta).
 *
 * Backward from dy (S, Cout, N): u and the hidden layer are recomputed from x (and mean, rstd);
 * dx (S, Cin, N) includes the LayerNorm's backward; the residual's gradient is dy itself and is
 * the caller's.  dW1, db1, dW2, db2 (and dgamma, dbeta with LayerNorm) go through per-workgroup
 * partials in scratch, S nblk rows of Chid Cin + Chid + Cout Chid + Cout + 2 Cin floats, which a
 * second launch adds in index order.  No atomics: two calls agree to the bit.
 *
 * Each entry returns hipErrorInvalidValue, with nothing launched, for a configuration other than
 * the two above (LayerNorm pointers given to the second or missing from the first included),
 * S < 1, S > 65535, N < 1, N > 2^24, a stride below C N or a NULL required pointer; the size
 * queries return -1 for such arguments (blindno_plane_mlp_ok: 0). */

/* 1 for (32, 32, 32, has_ln = 1) and (4, 64, 32, has_ln = 0), else 0. */
int blindno_plane_mlp_ok(int Cin, int Chid, int Cout, int has_ln);
/* Workgroups per snapshot (256 points each). */
int blindno_plane_mlp_nblk(int N);
int blindno_plane_mlp_fwd(const float* x, int64_t xstride, const float* gamma, const float* beta,
                          const float* W1, const float* b1, const float* W2, const float* b2,
                          const float* res, int64_t rstride, float* y, int64_t ystride,
                          float* mean, float* rstd, int S, int N, int Cin, int Chid, int Cout,
                          float eps, blindno_stream_t stream);
/* Backward scratch: the partial table; contents undefined afterwards. */
int64_t blindno_plane_mlp_bwd_scratch_floats(int S, int N, int Cin, int Chid, int Cout);
int blindno_plane_mlp_bwd(const float* dy, int64_t dystride, const float* x, int64_t xstride,
                          const float* gamma, const float* beta, const float* W1, const float* b1,
                          const float* W2, const float* mean, const float* rstd, float* scratch,
                          float* dx, int64_t dxstride, float* dW1, float* db1, float* dW2,
                          float* db2, float* dgamma, float* dbeta, int S, int N, int Cin, int Chid,
                          int Cout, blindno_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* BLINDNO_PLANEMLP_H */
