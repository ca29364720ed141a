/* libblindno C ABI, part 7: record-free Fokker-Planck propagation with the density-error sums
 * reduced on the device.
 *
 * Included by blindno.h (include that one); same conventions: every entry returns a hipError_t
 * code as int (0 = success) unless it is a size query, pointers are device pointers, the last
 * argument is the stream, nothing is allocated and nothing synchronises inside.  The Python
 * binding keeps these entries in blindno._lib.ABI["blindno_fpe_err.h"].
 */
#ifndef BLINDNO_FPE_ERR_H
#define BLINDNO_FPE_ERR_H

#include "blindno.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- blindno_fp_propagate_nd (blindno_fpe.h) without its record: the squared density error of
 * every trajectory against a reference trajectory of the same batch, per output time.  fp64 only
 * (csrc/fpe_nd.hip).
 *   p0   (B, N), coef (B, 7, N)   exactly as in blindno_fp_propagate_nd; N = nx*ny*nz, nz = 1 is a
 *                     2D grid and ny = nz = 1 a 1D one
 *   group             trajectories come in consecutive groups of `group`; trajectory g*group is the
 *                     reference of trajectories g*group .. g*group + group - 1 (the evaluator's
 *                     layout: the true field first, then one trajectory per model)
 *   err  (B, nout, 2) err[b, o, 0] = sum_i (p_b(t_o)[i] - p_ref(b)(t_o)[i])^2,
 *                     err[b, o, 1] = sum_i p_ref(b)(t_o)[i]^2,  t_o = o dt_out, o = 0 .. nout-1;
 *                     for the reference itself the first entry is exactly 0.0
 *   scratch           blindno_fp_error_nd_scratch_doubles(B, nx, ny, nz) = 3 B N + 2 B ceil(N / 256)
 *                     doubles (the density, the two Horner iterates and the per-tile partial sums;
 *                     contents undefined afterwards)
 * The integrator is blindno_fp_propagate_nd's bit for bit -- the same pass kernel, h = dt_out /
 * substeps, Horner order and degree-1 special case -- so every density has the bits that entry
 * would have recorded; no frame is written anywhere.  After the initial state and after every
 * output interval two launches reduce the sums in a fixed order: per-tile partials (256 cells, a
 * fixed tree), then one workgroup per trajectory adds the tiles in index order.  A second call is
 * bit-identical, and a group's result does not depend on the rest of the batch.
 * (nout - 1) * substeps * degree + 2 nout + 1 kernels are enqueued in all -- the caller bounds
 * that product.
 * hipErrorInvalidValue, with nothing launched, for B <= 0, group < 1, B % group != 0, a dimension
 * < 1, nout < 1, substeps < 1, degree < 1, a NULL pointer (scratch included) or N above
 * BLINDNO_FP_ND_MAX_CELLS; the size query returns -1 for such a grid. */
int64_t blindno_fp_error_nd_scratch_doubles(int B, int nx, int ny, int nz);
int blindno_fp_error_nd(const double* p0, const double* coef, double* err, double* scratch, int B,
                        int group, int nx, int ny, int nz, int nout, int substeps, int degree,
                        double dt_out, blindno_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* BLINDNO_FPE_ERR_H */
