/* libblindno C ABI, part 6: the grid-resident 3D Gross-Pitaevskii split-step solver and the 3D
 * trapezoid density residual.
 *
 * Included by blindno.h (include that one); same conventions: every entry returns a hipError_t
 * code as int (0 = success) unless it is a size query, pointers are device pointers, the last
 * argument is the stream, nothing is allocated and nothing synchronises inside.  The Python
 * binding keeps these entries in blindno._lib.ABI["blindno_gpe3d.h"].
 */
#ifndef BLINDNO_GPE3D_H
#define BLINDNO_GPE3D_H

#include "blindno.h"

#ifdef __cplusplus
extern "C" {
#endif

/* nx, ny and nz of blindno_gpe3d_solve are each a power of two in this range (not necessarily
 * equal).  MAX_N is what the narrowest column tile's LDS supports: 4 columns x 1024 points, two
 * buffers plus the tables, is 152 KiB of the CU's 160 KiB, as in the 2D solver. */
#define BLINDNO_GPE3D_MIN_N 4
#define BLINDNO_GPE3D_MAX_N 1024
/* nx ny nz of one trajectory is at most this (256^3: a 256 MiB working field per trajectory). */
#define BLINDNO_GPE3D_MAX_CELLS (1 << 24)

/* ---- i psi_t = -1/2 (psi_xx + psi_yy + psi_zz) + (V + g|psi|^2 + kappa|psi|^4) psi on a periodic
 * nx x ny x nz grid, B trajectories, fp64 (csrc/gpe3d.hip).  Point (ix, iy, iz) of a field is
 * element (ix*ny + iy)*nz + iz (z contiguous); complex fields are interleaved (re, im) doubles,
 * 16-byte aligned.
 *   psi0     (B, nx, ny, nz, 2) if psi0_batched, else (nx, ny, nz, 2) shared by every trajectory
 *   V        (B, nx, ny, nz);  g, kappa (B)
 *   rec_abs  (B, nrec, nx, ny, nz) |psi| of the recorded steps, doubles, or floats when
 *            rec_abs_f32 (the fp64 value rounded once); may be NULL
 *   rec_psi  (B, nrec, nx, ny, nz, 2) the recorded fields; may be NULL
 *   psi_out  (B, nx, ny, nz, 2) the field after nsteps steps; may be NULL
 *   scratch  blindno_gpe3d_scratch_doubles(B, nx, ny, nz) = 2 B nx ny nz doubles (the working
 *            field; contents undefined afterwards)
 * nrec = nsteps / rec_every + 1: steps 0, rec_every, 2 rec_every, ... are recorded.
 * The integrator is blindno_gpe2d_solve's with one more axis: N(h) multiplies by
 * exp(-i h (V + g|psi|^2 + kappa|psi|^4)) pointwise, L(h) = ifftn(exp(-i h/2 (kx^2 + ky^2 + kz^2))
 * fftn), kx = 2 pi fftfreq(nx, dx), ky and kz likewise; order 2 is Strang N(dt/2) L(dt) N(dt/2)
 * per step (the two half steps at a step boundary stay two applications), order 4 the nine-stage
 * Yoshida sequence.  L is applied as L_x L_y L_z, one launch per axis with the pointwise work
 * fused in: blindno_gpe3d_launches(nsteps, order) = 3 nsteps (order 2) or 12 nsteps (order 4)
 * kernels are enqueued on `stream` (1 when nsteps = 0) -- the caller bounds that number.  The only
 * ordering between them is the stream's; nothing is accumulated across workgroups, so a second
 * call is bit-identical and a trajectory's result does not depend on the rest of the batch.
 * Every offset is formed in 64 bits.
 * hipErrorInvalidValue, with nothing launched, for B <= 0, nx, ny or nz not a power of two in
 * [BLINDNO_GPE3D_MIN_N, BLINDNO_GPE3D_MAX_N], nx ny nz > BLINDNO_GPE3D_MAX_CELLS, an order other
 * than 2 or 4, rec_every < 1, nsteps < 0, dx, dy or dz not positive, rec_abs_f32 not 0 or 1, a
 * NULL psi0, V, g, kappa or scratch, a complex pointer that is not 16-byte aligned, or a record
 * whose byte size does not fit 63 bits; the size queries return -1 for such arguments. */
int64_t blindno_gpe3d_scratch_doubles(int B, int nx, int ny, int nz);
int64_t blindno_gpe3d_launches(int nsteps, int order);
int blindno_gpe3d_solve(const double* psi0, const double* V, const double* g, const double* kappa,
                        double dx, double dy, double dz, double dt, int nsteps, int order,
                        int rec_every, void* rec_abs, int rec_abs_f32, double* rec_psi,
                        double* psi_out, double* scratch, int B, int nx, int ny, int nz,
                        int psi0_batched, blindno_stream_t stream);

/* ---- the 3D density residual of time_averaged_L2_error_3d: per frame f of a, b
 * (frames, nx, ny, nz)
 *   out[2f]   = trapz_z(trapz_y(trapz_x((a_f - b_f)^2))),   out[2f+1] = the same of b_f^2
 * on the grids x (nx), y (ny), z (nz) (numpy.trapz along each axis), fp64.  One workgroup per
 * frame (the entry takes no scratch), a two-stage reduction in a fixed order (deterministic). */
int blindno_trapz3_frames(const double* a, const double* b, const double* x, const double* y,
                          const double* z, double* out, int frames, int nx, int ny, int nz,
                          blindno_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* BLINDNO_GPE3D_H */
