/* libblindno C ABI, part 14: the multiplicity-weighted bag token attention of NIOFP2D_Trans_attn.
 *
 * Included by blindno.h (include that one); same conventions: every entry returns a hipError_t
 * code as int (0 = success) unless it is a query, pointers are device pointers, the last
 * argument is the stream, nothing is allocated and nothing synchronises inside.  The Python
 * binding keeps these entries in blindno._lib.ABI["blindno_bagattn_mix.h"].
 */
#ifndef BLINDNO_BAGATTN_MIX_H
#define BLINDNO_BAGATTN_MIX_H

#include "blindno.h"

#ifdef __cplusplus
extern "C" {
#endif

/* NIOFP2D_Trans_attn (2d_FPE/NIOModules.py:169-296; NC copy 2d_Non_conservative_FPE/
 * NIOModules.py:168-) runs softmax(X X^T / sqrt(S)) X over the tokens [gx, gy, u_1 .. u_L] of a
 * bag drawn with replacement and fuses the token outputs with fc0 = Linear(3, width) read through
 * .data: the two grid tokens' outputs get W[:, 0] and W[:, 1], every snapshot token's W[:, 2] / L.
 * A duplicate's row and column of the attention are copies of its original's, so the op runs on
 * the U distinct snapshots with counts nu_u (sum L), csrc/bagattn_mix.hip, fp32.  With V = U + 2,
 * X = [gx, gy, u_1 .. u_U] (V rows of S points) and masses nut = [1, 1, nu_1 .. nu_U]:
 *     G = X X^T / sqrt(S)                                         (does not depend on nu)
 *     P[t, v] = nut_v e^{G[t, v]} / sum_v' nut_v' e^{G[t, v']}     row maximum subtracted
 *     r_0 = P[0, :],  r_1 = P[1, :],  r_2 = sum_{t >= 2} lw_t P[t, :],   lw_t = nu_t / L
 *     m_k[p] = sum_v r_k[v] X[v, p],   y[b, p, c] = sum_k W[c, k] m_k[p] + bias[c]
 * Backward from dy (B, S, width):
 *     dm_k[p] = sum_c W[c, k] dy[p, c],   dr_k[v] = sum_p X[v, p] dm_k[p]
 *     dP[0, :] = dr_0,  dP[1, :] = dr_1,  dP[t, :] = lw_t dr_2 (t >= 2)
 *     dG = P o (dP - rowsum(P o dP)),   M = (dG + dG^T) / sqrt(S)
 *     dX[v, p] = sum_k r_k[v] dm_k[p] + sum_t M[v, t] X[t, p]
 * Rows 0, 1 of dX are the grid tokens' gradient dgt (B, 2, S), written when dgt is non-NULL; rows
 * >= 2 are du, the gradient with respect to a DISTINCT snapshot (the sum over its duplicates).
 * Nothing of size V S is written besides du, and no (B, L, S) array exists.
 *
 *   grid (S, 2), u (B, U, S), W (width, 3), bias (width), y (B, S, width)
 *   lw (U) = nu / L, or NULL: every nu = 1 and L = U (the argument L is then ignored).  The counts
 *   are recovered as rint(lw L), so they are exact integers.
 *   P (B, V, V) and r (B, 3, V) are written by the forward and read by the backward.
 *
 * Launches: forward Gram partials (the chunked kernel of blindno_bagattn_fwd, 512 points per
 * workgroup), one workgroup per bag for P and r, one pass over X for y; backward one pass over X
 * for dm and the dr partials (128 points per workgroup), one workgroup per bag for M, one pass
 * over X for dX.  Every reduction is a fixed-order sum over per-chunk partials, with no atomics: a
 * second call is bit-identical.
 *
 * Limits: B, U, S, width >= 1, V = U + 2 <= 256, B <= 65535; with lw, L >= U.
 * blindno_bagattn_mix_ok answers 1 for such a shape and 0 otherwise; fwd and bwd return
 * hipErrorInvalidValue, with nothing launched, where it answers 0, for a NULL pointer (lw and dgt
 * excepted) or for lw with L < U; the other queries return -1. */
int blindno_bagattn_mix_ok(int B, int U, int S, int width);

/* Workgroups per bag of the Gram pass and of the backward's first pass. */
int blindno_bagattn_mix_nchunk(int S);
int blindno_bagattn_mix_bwd_nchunk(int S);

/* Forward scratch: the Gram partials, B nchunk V V floats; contents undefined afterwards. */
int64_t blindno_bagattn_mix_fwd_scratch_floats(int B, int U, int S);
int blindno_bagattn_mix_fwd(const float* grid, const float* u, const float* W, const float* bias,
                            const float* lw, float* scratch, float* P, float* r, float* y, int B,
                            int U, int S, int width, int L, blindno_stream_t stream);

/* Backward scratch: dm (B 3 S), the dr partials (B bwd_nchunk 3 V) and M (B V V) floats, in that
 * order; contents undefined afterwards. */
int64_t blindno_bagattn_mix_bwd_scratch_floats(int B, int U, int S);
int blindno_bagattn_mix_bwd(const float* grid, const float* u, const float* dy, const float* W,
                            const float* lw, const float* P, const float* r, float* scratch,
                            float* du, float* dgt, int B, int U, int S, int width, int L,
                            blindno_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* BLINDNO_BAGATTN_MIX_H */
