/* libblindno C ABI, part 4: the grid-resident 2D Gross-Pitaevskii split-step solver and the 2D
 * trapezoid density residual.
 *
 * Included by blindno.h (include that one); same conventions: every entry returns a hipError_t
 * code as int (0 = success) unless it is a size query, pointers are device pointers, the last
 * argument is the stream, nothing is allocated and nothing synchronises inside.  The Python
 * binding keeps these entries in blindno._lib.ABI["blindno_gpe2d.h"].
 */
#ifndef BLINDNO_GPE2D_H
#define BLINDNO_GPE2D_H

#include "blindno.h"

#ifdef __cplusplus
extern "C" {
#endif

/* nx and ny of blindno_gpe2d_solve are each a power of two in this range (not necessarily equal). */
#define BLINDNO_GPE2D_MIN_N 4
#define BLINDNO_GPE2D_MAX_N 1024

/* ---- i psi_t = -1/2 (psi_xx + psi_yy) + (V + g|psi|^2 + kappa|psi|^4) psi on a periodic
 * nx x ny grid, B trajectories, fp64 (csrc/gpe2d.hip).  Point (ix, iy) of a field is element
 * ix*ny + iy (y contiguous); complex fields are interleaved (re, im) doubles, 16-byte aligned.
 *   psi0     (B, nx, ny, 2) if psi0_batched, else (nx, ny, 2) shared by every trajectory
 *   V        (B, nx, ny);  g, kappa (B)
 *   rec_abs  (B, nrec, nx, ny) |psi| of the recorded steps, doubles, or floats when rec_abs_f32
 *            (the fp64 value rounded once); may be NULL
 *   rec_psi  (B, nrec, nx, ny, 2) the recorded fields; may be NULL
 *   psi_out  (B, nx, ny, 2) the field after nsteps steps; may be NULL
 *   scratch  blindno_gpe2d_scratch_doubles(B, nx, ny) = 2 B nx ny doubles (the working field;
 *            contents undefined afterwards)
 * nrec = nsteps / rec_every + 1: steps 0, rec_every, 2 rec_every, ... are recorded.
 * The integrator is blindno_gpe_solve's split step with one more axis: N(h) multiplies by
 * exp(-i h (V + g|psi|^2 + kappa|psi|^4)) pointwise, L(h) = ifft2(exp(-i h/2 (kx^2 + ky^2)) fft2),
 * kx = 2 pi fftfreq(nx, dx), ky likewise; order 2 is Strang N(dt/2) L(dt) N(dt/2) per step (the
 * two half steps at a step boundary stay two applications), order 4 the nine-stage Yoshida
 * sequence.  L is applied as L_x L_y, one launch per axis with the pointwise work fused in:
 * blindno_gpe2d_launches(nsteps, order) = 2 nsteps (order 2) or 8 nsteps (order 4) kernels are
 * enqueued on `stream` (1 when nsteps = 0) -- the caller bounds that number.  The only ordering
 * between them is the stream's; nothing is accumulated across workgroups, so a second call is
 * bit-identical and a trajectory's result does not depend on the rest of the batch.
 * hipErrorInvalidValue, with nothing launched, for B <= 0, nx or ny not a power of two in
 * [BLINDNO_GPE2D_MIN_N, BLINDNO_GPE2D_MAX_N], an order other than 2 or 4, rec_every < 1,
 * nsteps < 0, dx or dy not positive, rec_abs_f32 not 0 or 1, a NULL psi0, V, g, kappa or scratch,
 * or a complex pointer that is not 16-byte aligned; the size queries return -1 for such
 * arguments. */
int64_t blindno_gpe2d_scratch_doubles(int B, int nx, int ny);
int64_t blindno_gpe2d_launches(int nsteps, int order);
int blindno_gpe2d_solve(const double* psi0, const double* V, const double* g, const double* kappa,
                        double dx, double dy, double dt, int nsteps, int order, int rec_every,
                        void* rec_abs, int rec_abs_f32, double* rec_psi, double* psi_out,
                        double* scratch, int B, int nx, int ny, int psi0_batched,
                        blindno_stream_t stream);

/* ---- the 2D density residual of time_averaged_L2_error_2d: per frame f of a, b (frames, nx, ny)
 *   out[2f]   = trapz_y(trapz_x((a_f - b_f)^2)),   out[2f+1] = trapz_y(trapz_x(b_f^2))
 * on the grids x (nx), y (ny) (numpy.trapz along each axis), fp64, one workgroup per frame with a
 * fixed-order reduction (deterministic). */
int blindno_trapz2_frames(const double* a, const double* b, const double* x, const double* y,
                          double* out, int frames, int nx, int ny, blindno_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* BLINDNO_GPE2D_H */
