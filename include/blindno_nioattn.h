/* libblindno C ABI, part 10: the bag token attention of NIOFP2D_attn in coefficient space.
 *
 * Included by blindno.h (include that one); same conventions: every entry returns a hipError_t
 * code as int (0 = success) unless it is a size query, pointers are device pointers, the last
 * argument is the stream, nothing is allocated and nothing synchronises inside.  The Python
 * binding keeps these entries in blindno._lib.ABI["blindno_nioattn.h"].
 */
#ifndef BLINDNO_NIOATTN_H
#define BLINDNO_NIOATTN_H

#include "blindno.h"

#ifdef __cplusplus
extern "C" {
#endif

/* NIOFP2D_attn (2d_FPE/NIOModules.py:410-504; NC copy 2d_Non_conservative_FPE/NIOModules.py:406-)
 * feeds the DeepONet field u[b, l, p] = (w[b, l, :] . basis[p, :] + b0) / sqrt(P)
 * (DeepOnetNoBiasOrg.forward) to the bag token attention of :463-495: tokens X_b = [gx, gy, u_1 ..
 * u_L] (T = L + 2 rows of S = nx ny points), A = softmax(X X^T / sqrt(S)), fused = (A X)^T w0 / T +
 * bias with fc0 = Linear(1, width) read through .data.  Those tokens have rank <= Q = P + 3:
 *     X_b = C_b Phi^T,   Phi (S, Q) = [gx, gy, scale basis_0 .. scale basis_{P-1}, scale 1],
 *     C_b (T, Q): rows 0, 1 the unit vectors e_0, e_1, row 2 + l = [0, 0, w[b, l, :], b0],
 * scale = 1 / sqrt(P), so the attention runs on the coefficients (csrc/nioattn.hip), fp32:
 *     M = Phi^T Phi (Q, Q)                     the only reduction over S, shared by the batch
 *     A_b = softmax_rows(C M C^T / sqrt(S))    row maximum subtracted
 *     cs_b[s] = sum_t A_b[t, s],   v_b = C^T cs_b / T (Q)
 *     y[b, p, c] = fc0w[c] (Phi[p] . v_b) + fc0b[c]
 * and nothing of size B L S or T S exists.  Backward from dy (B, S, width):
 *     dm = dy . fc0w,  dv_b = sum_p dm[b, p] Phi[p],  dcs = C dv / T,
 *     dS = A o (dcs_row - A dcs),  E = dS C,  F = dS^T C,
 *     dC = cs dv^T / T + (E + F) M / sqrt(S),   dM = sum_b C^T E / sqrt(S),
 *     dPhi[p] = Phi[p] (dM + dM^T) + sum_b dm[b, p] v_b,
 *     dw[b, l, :] = dC[b, 2 + l, 2 : 2 + P],  db0 = sum_{b, l} dC[b, 2 + l, Q - 1],
 *     dbasis = scale dPhi[:, 2 : 2 + P];  no grid gradient.
 * Limits: 1 <= P <= 64, L >= 1, T = L + 2 <= 256; any B, S, width >= 1.
 * Every reduction runs in a fixed order (per-workgroup partials added in index order, bags in
 * index order, no atomics): a second call is bit-identical and a bag's A, cs, v do not depend on
 * the rest of the batch.  The per-bag kernels use up to 150 KB of LDS at T = 256, P = 64 (their
 * dynamic LDS limit is raised once per device, the first time a shape needs more than 64 KB).
 *
 *   grid (S, 2), basis (S, P), w (B, L, P), b0 (1), fc0w (width), fc0b (width)
 *   M (Q, Q), A (B, T, T), cs (B, T), v (B, Q), y (B, S, width)
 *   dw (B, L, P), dbasis (S, P), db0 (1)
 *
 * Each entry returns hipErrorInvalidValue, with nothing launched, for B <= 0 (fwd, bwd), L < 1,
 * T > 256 (fwd, bwd), P < 1, P > 64, S < 1, width < 1 (fwd, bwd), a NULL pointer, or a block count
 * that is not the query's; the queries return -1 for such sizes. */

/* Workgroups of the moments' first stage (128 points each) and its scratch, nblk Q Q floats. */
int blindno_nioattn_moments_nblk(int S);
int64_t blindno_nioattn_moments_scratch_floats(int S, int P);
/* M from grid and basis: per-workgroup partials, then one pass adding them in index order. */
int blindno_nioattn_moments(const float* grid, const float* basis, float* partial, float* M,
                            int nblk, int S, int P, blindno_stream_t stream);

/* A, cs, v (kept for the backward) and y.  One workgroup per bag, then one pass over basis. */
int blindno_nioattn_fwd(const float* w, const float* b0, const float* basis, const float* grid,
                        const float* M, const float* fc0w, const float* fc0b, float* A, float* cs,
                        float* v, float* y, int B, int L, int S, int P, int width,
                        blindno_stream_t stream);

/* Workgroups of the backward's two streaming passes (128 points each) and its scratch:
 * dm (B S), the dv partials (nblk B Q), the per-bag dM (B Q Q), dM + dM^T (Q Q) and the per-bag
 * db0 (B) floats, in that order; contents undefined afterwards. */
int blindno_nioattn_bwd_nblk(int S);
int64_t blindno_nioattn_bwd_scratch_floats(int B, int S, int P);
int blindno_nioattn_bwd(const float* dy, const float* w, const float* b0, const float* basis,
                        const float* grid, const float* M, const float* fc0w, const float* A,
                        const float* cs, const float* v, float* scratch, float* dw, float* dbasis,
                        float* db0, int nblk, int B, int L, int S, int P, int width,
                        blindno_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* BLINDNO_NIOATTN_H */
