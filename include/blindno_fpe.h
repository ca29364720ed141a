/* libblindno C ABI, part 3: Fokker-Planck propagation on grids of any size, up to three dimensions.
 *
 * Included by blindno.h (include that one); same conventions: every entry returns a hipError_t
 * code as int (0 = success) unless it is a size query, pointers are device pointers, the last
 * argument is the stream, nothing is allocated and nothing synchronises inside.  The Python
 * binding keeps these entries in blindno._lib.ABI["blindno_fpe.h"].
 */
#ifndef BLINDNO_FPE_H
#define BLINDNO_FPE_H

#include "blindno.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The largest grid blindno_fp_propagate_nd accepts: N = nx*ny*nz <= 2^26 cells (and
 * B * ceil(N / 256) < 2^31 workgroups per pass). */
#define BLINDNO_FP_ND_MAX_CELLS (1 << 26)

/* ---- dp/dt = M p, the finite-volume master equation of blindno_fp_propagate (fplanck's
 * fokker_planck.master_matrix) on a grid of N = nx*ny*nz cells, cell i = (ix*ny + iy)*nz + iz; ny
 * = nz = 1 is a 1D grid, nz = 1 a 2D one.  fp64 only (csrc/fpe_nd.hip).
 *   p0   (B, N)       initial densities
 *   coef (B, 7, N)    [diag, cxm, cxp, cym, cyp, czm, czp] per trajectory: the cell's total
 *                     out-rate, then the in-rates from its six neighbours.  Neighbour indices wrap per axis (the periodic case); a zero coefficient
 *                     makes a wall.  Rows of an absent axis are zero.
 *   out  (B, nout, N) out[:, 0] = p0, out[:, o] = exp(o dt_out M) p0
 *   scratch           blindno_fp_propagate_nd_scratch_doubles(B, nx, ny, nz) = 2 B N doubles
 *                     (the two Horner iterates; contents undefined afterwards)
 * The integrator is blindno_fp_propagate's: each output interval is `substeps` steps of the
 * degree-`degree` Taylor polynomial of exp(h M), h = dt_out / substeps, in Horner form
 * w <- p + (h / k) M w, k = degree..1, with the same per-cell operation order and the two z terms
 * appended, so with nz = 1 (zero z rows) the result is bit-identical to blindno_fp_propagate.
 * Unlike that kernel the grid is not bound to one workgroup's LDS: the density and the iterates
 * stay in global memory, each Horner pass is one launch on `stream`, and
 * (nout - 1) * substeps * degree + 1 kernels are enqueued in all -- the caller bounds that
 * product.  No atomics: a second call is bit-identical, and a trajectory's result does not depend
 * on the rest of the batch.
 * hipErrorInvalidValue, with nothing launched, for B <= 0, a dimension < 1, nout < 1,
 * substeps < 1, degree < 1, a NULL pointer (scratch included) or N above
 * BLINDNO_FP_ND_MAX_CELLS; the size query returns -1 for such a grid. */
int64_t blindno_fp_propagate_nd_scratch_doubles(int B, int nx, int ny, int nz);
int blindno_fp_propagate_nd(const double* p0, const double* coef, double* out, double* scratch,
                            int B, int nx, int ny, int nz, int nout, int substeps, int degree,
                            double dt_out, blindno_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* BLINDNO_FPE_H */
