/* libblindno C ABI, part 9: the 2D Gross-Pitaevskii solver without its record, with the density-error
 * sums reduced on the device.
 *
 * Included by blindno.h (include that one); same conventions: every entry returns a hipError_t
 * code as int (0 = success) unless it is a size query, pointers are device pointers, the last
 * argument is the stream, nothing is allocated and nothing synchronises inside.  The Python
 * binding keeps these entries in blindno._lib.ABI["blindno_gpe2d_err.h"].
 */
#ifndef BLINDNO_GPE2D_ERR_H
#define BLINDNO_GPE2D_ERR_H

#include "blindno.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Cells of one workgroup of the first reduction stage: 256 threads, four consecutive runs of 256
 * cells each.  A trajectory has ceil(nx ny / BLINDNO_GPE2D_ERR_TILE) tiles. */
#define BLINDNO_GPE2D_ERR_TILE 1024

/* ---- blindno_gpe2d_solve (blindno_gpe2d.h) without its record: the trapezoid integrals of the
 * squared |psi| error of every trajectory against a reference trajectory of the same batch, per
 * recorded step.  fp64 (csrc/gpe2d.hip).
 *   psi0, V, g, kappa, dx, dy, dt, nsteps, order, rec_every, psi0_batched
 *                      exactly as in blindno_gpe2d_solve
 *   x (nx), y (ny)     the grids; used only for the trapezoid weights, as in blindno_trapz2_frames
 *                      (numpy.trapz along each axis)
 *   group              trajectories come in consecutive groups of `group`; trajectory
 *                      (b / group) * group is the reference of trajectory b (the evaluator's layout:
 *                      the true V first, then one trajectory per model)
 *   err (B, nrec, 2)   nrec = nsteps / rec_every + 1; at step r rec_every
 *                      err[b, r, 0] = trapz_y trapz_x (|psi_b| - |psi_ref(b)|)^2,
 *                      err[b, r, 1] = the same integral of |psi_ref(b)|^2;
 *                      for a reference trajectory the first entry is exactly 0.0, and the second
 *                      entry of every member of a group is its reference's bit for bit
 *   scratch            blindno_gpe2d_error_scratch_doubles(B, nx, ny) = 3 B N + 2 B ceil(N /
 *                      BLINDNO_GPE2D_ERR_TILE) doubles, N = nx ny, 16-byte aligned: the working
 *                      field (2 B N), one |psi| frame per trajectory (B N) and the per-tile partial
 *                      sums; contents undefined afterwards
 * The integrator is blindno_gpe2d_solve's launch sequence argument for argument; only the record is
 * redirected to the one-frame buffer, so every |psi| that is reduced has the bits that entry would
 * have recorded.  After each launch that writes a frame two kernels reduce it in a fixed order: per
 * tile the terms w (d d) and w (b b) with w = wx wy as blindno_trapz2_frames forms them
 * (lane-strided sums, then a fixed tree), then one workgroup per trajectory adds its tiles (each
 * thread ascending strided tiles, then the same tree).  No location is touched by two workgroups
 * of a launch, every offset is formed in 64 bits, a second call is bit-identical and a group's
 * result does not depend on the rest of the batch.
 * blindno_gpe2d_error_launches(nsteps, order, rec_every) = blindno_gpe2d_launches(nsteps, order) +
 * 2 (nsteps / rec_every + 1) kernels are enqueued -- the caller bounds that number.
 * hipErrorInvalidValue, with nothing launched, for everything blindno_gpe2d_solve refuses for the
 * shared arguments, group < 1, B % group != 0, a NULL x, y, err or scratch, or a scratch that is
 * not 16-byte aligned; the queries return -1 for such arguments. */
int64_t blindno_gpe2d_error_scratch_doubles(int B, int nx, int ny);
int64_t blindno_gpe2d_error_launches(int nsteps, int order, int rec_every);
int blindno_gpe2d_error(const double* psi0, const double* V, const double* g, const double* kappa,
                        const double* x, const double* y, double dx, double dy, double dt,
                        int nsteps, int order, int rec_every, int group, double* err,
                        double* scratch, int B, int nx, int ny, int psi0_batched,
                        blindno_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* BLINDNO_GPE2D_ERR_H */
