"""blindno_fp_error_nd (csrc/fpe_nd.hip), the record-free Fokker-Planck propagation whose per-frame
density-error sums are reduced on the device (needs a GPU).

The yardstick is blindno_fp_propagate_nd's record for the same arguments (the existing entry, itself
held to scipy's expm_multiply by tests/test_gpu_fpe_nd.py), its sums taken with math.fsum.  Each of
the two sums has to agree to a relative (N + 2) 2^-53: the terms are non-negative, so any summation
order is within (N - 1) u of the exact sum, plus one rounding each for the difference and the
square.  That bound only holds if every density has the record's bits, i.e. the integrator is the
same bit for bit.

Every case: B = 6 distinct trajectories (trajectory 1 a copy of trajectory 0), group = 3, 1 and 6,
substeps 1 and 3, nout 1 and 4, degree 18 and degree 1, the substep length at the integrator's own
bound ||h M||_1 = 1/2.
"""
import ctypes
import math

import numpy as np
import pytest
import torch

import fpe3d_ref
from fpe3d_ref import initial, make_sim

pytestmark = pytest.mark.gpu

B = 6
INVALID = 1          # hipErrorInvalidValue
U = 2.0 ** -53

# shape: periodic flags.  60 cells: one partial tile; 294: a full tile and a partial one; 2D; 1D
SHAPES = {(5, 4, 3): (False, True, False),
          (7, 6, 7): (False, False, False),
          (16, 16, 1): (True, False, False),
          (300, 1, 1): (False, False, False)}


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")


_BATCH = {}


def _batch(dims):
    """(sims, p0 (B, N), coef (B, 7, N), h) of the case, built once; trajectory 1 is trajectory 0."""
    if dims not in _BATCH:
        sims = [make_sim(dims, SHAPES[dims], k) for k in range(B)]
        sims[1] = sims[0]
        p0 = np.stack([initial(s, k) for k, s in enumerate(sims)])
        p0[1] = p0[0]
        coef = np.stack([s.coefficients_nd() for s in sims])
        h = 0.5 / (2.0 * float(coef[:, 0].max()))
        for a in (p0, coef):
            a.setflags(write=False)
        _BATCH[dims] = (sims, p0, coef, h)
    return _BATCH[dims]


def _run_err(p0, coef, dims, group, nout, substeps, degree, h):
    from blindno._lib import call, ptr, query, stream_ptr
    n = p0.shape[0]
    p0_d, coef_d = torch.from_numpy(np.ascontiguousarray(p0)).cuda(), torch.from_numpy(np.ascontiguousarray(coef)).cuda()
    err = torch.full((n, nout, 2), float("nan"), dtype=torch.float64, device="cuda")
    scratch = torch.full((query("blindno_fp_error_nd_scratch_doubles", n, *dims),), float("nan"),
                         dtype=torch.float64, device="cuda")
    call("blindno_fp_error_nd", ptr(p0_d), ptr(coef_d), ptr(err), ptr(scratch), n, group, *dims, nout, substeps,
         degree, substeps * h, stream_ptr())
    torch.cuda.synchronize()
    return err.cpu().numpy()


def _run_record(p0, coef, dims, nout, substeps, degree, h):
    from blindno._lib import call, ptr, query, stream_ptr
    n = p0.shape[0]
    p0_d, coef_d = torch.from_numpy(np.ascontiguousarray(p0)).cuda(), torch.from_numpy(np.ascontiguousarray(coef)).cuda()
    out = torch.full((n, nout, p0.shape[1]), float("nan"), dtype=torch.float64, device="cuda")
    scratch = torch.empty(query("blindno_fp_propagate_nd_scratch_doubles", n, *dims), dtype=torch.float64, device="cuda")
    call("blindno_fp_propagate_nd", ptr(p0_d), ptr(coef_d), ptr(out), ptr(scratch), n, *dims, nout, substeps, degree,
         substeps * h, stream_ptr())
    torch.cuda.synchronize()
    return out.cpu().numpy()


def _fsums(rec, group):
    """(B, nout, 2) sums of the record's frames, each with math.fsum."""
    n, nout, _ = rec.shape
    out = np.zeros((n, nout, 2))
    for b in range(n):
        r = rec[b // group * group]
        for o in range(nout):
            d = rec[b, o] - r[o]
            out[b, o] = math.fsum(d * d), math.fsum(r[o] * r[o])
    return out


# ---- 1. the sums against the record entry; reference rows; determinism; group independence
@pytest.mark.parametrize("degree", [18, 1])
@pytest.mark.parametrize("dims", list(SHAPES))
def test_sums_match_the_record(dims, degree):
    _need_gpu()
    _, p0, coef, h = _batch(dims)
    N = p0.shape[1]
    bound = (N + 2) * U
    worst = 0.0
    for substeps in (1, 3):
        for nout in (1, 4):
            rec = _run_record(p0, coef, dims, nout, substeps, degree, h)
            assert np.isfinite(rec).all()
            if nout > 1:
                assert not np.array_equal(rec[:, 0], rec[:, -1])         # the interval is not a no-op
            for group in (3, 1, 6):
                got = _run_err(p0, coef, dims, group, nout, substeps, degree, h)
                ref = _fsums(rec, group)
                assert np.isfinite(got).all() and (ref[..., 1] > 0).all()
                rel = np.abs(got - ref) / np.where(ref > 0, ref, 1.0)
                worst = max(worst, float(rel.max()))
                assert (rel <= bound).all(), (substeps, nout, group, float(rel.max()), bound)
                assert (got[ref == 0.0] == 0.0).all()
                # the reference rows, and trajectory 1 (the reference's own p0 and coef), exactly 0.0
                refs = np.arange(0, B, group)
                assert (got[refs, :, 0] == 0.0).all() and (got[refs, :, 1] > 0).all()
                assert (got[1, :, 0] == 0.0).all()
                # every other trajectory differs from its reference from the first frame on
                others = [b for b in range(B) if b % group and b != 1]
                assert (got[others, :, 0] > 0).all()
                # a second call repeats the bits
                assert _run_err(p0, coef, dims, group, nout, substeps, degree, h).tobytes() == got.tobytes()
                # a group run alone has the bits it has inside the batch
                if group < B:
                    g = B // group - 1
                    sl = slice(g * group, (g + 1) * group)
                    alone = _run_err(p0[sl], coef[sl], dims, group, nout, substeps, degree, h)
                    assert alone.tobytes() == got[sl].tobytes(), (substeps, nout, group)
    print(f"{dims} degree {degree}: worst relative deviation {worst:.3e} = {worst / U:.1f} u, bound {N + 2} u")


# ---- 2. rejected arguments launch nothing
def test_rejects_bad_arguments():
    _need_gpu()
    import blindno
    from blindno._lib import query, stream_ptr
    lib = blindno.load_library()
    dims = (5, 4, 3)
    _, p0, coef, h = _batch(dims)
    N, nout = p0.shape[1], 4
    p0_d, coef_d = torch.from_numpy(p0.copy()).cuda(), torch.from_numpy(coef.copy()).cuda()
    err = torch.full((B, nout, 2), -3.5, dtype=torch.float64, device="cuda")
    scratch = torch.full((query("blindno_fp_error_nd_scratch_doubles", B, *dims),), -3.5, dtype=torch.float64,
                         device="cuda")
    P = lambda t: ctypes.c_void_p(t.data_ptr())   # noqa: E731
    st = stream_ptr()
    good = dict(B=B, group=3, nx=5, ny=4, nz=3, nout=nout, substeps=1, degree=18)
    bad = [dict(B=0), dict(B=-3), dict(group=0), dict(group=-1), dict(group=4), dict(group=12), dict(nx=0),
           dict(ny=0), dict(nz=0), dict(nz=-2), dict(nout=0), dict(substeps=0), dict(degree=0),
           dict(nx=1 << 14, ny=1 << 14, nz=1 << 14), dict(nx=2 ** 31 - 1, ny=2 ** 31 - 1, nz=2 ** 31 - 1),
           dict(nx=(1 << 13) + 1, ny=1 << 13, nz=1)]            # one row above BLINDNO_FP_ND_MAX_CELLS
    for kw in bad:
        a = dict(good, **kw)
        rc = lib.blindno_fp_error_nd(P(p0_d), P(coef_d), P(err), P(scratch), *[a[k] for k in good], h, st)
        assert rc == INVALID, (kw, rc)
    ptrs = [P(p0_d), P(coef_d), P(err), P(scratch)]
    for k in range(4):                                          # each NULL pointer
        rc = lib.blindno_fp_error_nd(*[None if j == k else p for j, p in enumerate(ptrs)],
                                     *[good[k2] for k2 in good], h, st)
        assert rc == INVALID, k
    torch.cuda.synchronize()
    assert bool((err == -3.5).all()) and bool((scratch == -3.5).all())     # nothing ran
    rc = lib.blindno_fp_error_nd(*ptrs, *[good[k] for k in good], h, st)
    torch.cuda.synchronize()
    assert rc == 0 and bool(torch.isfinite(err).all())


# ---- 3. buffers: every err element written, nothing outside err and scratch
@pytest.mark.parametrize("substeps,degree", [(3, 18), (3, 1), (2, 2)])
def test_buffers_stay_in_bounds(substeps, degree):
    _need_gpu()
    from blindno._lib import call, ptr, query, stream_ptr
    dims = (7, 6, 7)                                            # 294 cells: no multiple of the tile
    _, p0, coef, h = _batch(dims)
    nout, Mg = 4, 256
    n_scr = query("blindno_fp_error_nd_scratch_doubles", B, *dims)
    assert n_scr == 3 * B * 294 + 2 * B * 2
    bufs = []
    for n in (B * nout * 2, n_scr):
        t = torch.full((n + 2 * Mg,), float("nan"), dtype=torch.float64, device="cuda")
        t[:Mg] = -7.25
        t[-Mg:] = -7.25
        bufs.append(t)
    p0_d, coef_d = torch.from_numpy(p0.copy()).cuda(), torch.from_numpy(coef.copy()).cuda()
    call("blindno_fp_error_nd", ptr(p0_d), ptr(coef_d), ptr(bufs[0][Mg:]), ptr(bufs[1][Mg:]), B, 3, *dims, nout,
         substeps, degree, substeps * h, stream_ptr())
    torch.cuda.synchronize()
    err = bufs[0][Mg:-Mg].cpu().numpy().reshape(B, nout, 2)
    assert np.isfinite(err).all()
    for t in bufs:
        assert bool((t[:Mg] == -7.25).all()) and bool((t[-Mg:] == -7.25).all())
    assert np.array_equal(p0_d.cpu().numpy(), p0) and np.array_equal(coef_d.cpu().numpy(), coef)
    assert err.tobytes() == _run_err(p0, coef, dims, 3, nout, substeps, degree, h).tobytes()


# ---- 4. the metric against expm_multiply of the independently assembled matrix
@pytest.mark.parametrize("substeps", [1, 3])
def test_metric_matches_expm_multiply(substeps):
    """mean_o sqrt(num_o) / (sqrt(den_o) + 1e-12) from the kernel's sums against the same metric of
    tests/fpe3d_ref.py's records at (5, 4, 3), to the 1e-9 tests/test_gpu_fpe_nd.py holds the
    propagator to against that checker."""
    _need_gpu()
    dims = (5, 4, 3)
    sims, p0, coef, h = _batch(dims)
    nout = 4
    if "expm" not in _BATCH:
        _BATCH["expm"] = np.stack([fpe3d_ref.propagate(fpe3d_ref.matrix_of(s), p0[k], 9 * h, 10)
                                   for k, s in enumerate(sims)])
        _BATCH["expm"].setflags(write=False)
    ref = _BATCH["expm"][:, ::substeps][:, :nout]
    got = _run_err(p0, coef, dims, 3, nout, substeps, 18, h)
    for b in range(B):
        r = ref[b // 3 * 3]
        want = float(np.mean(np.linalg.norm(ref[b] - r, axis=1) / (np.linalg.norm(r, axis=1) + 1e-12)))
        metric = float(np.mean(np.sqrt(got[b, :, 0]) / (np.sqrt(got[b, :, 1]) + 1e-12)))
        print(f"substeps {substeps} trajectory {b}: metric {metric!r}, expm_multiply {want!r}")
        if b % 3 == 0 or b == 1:
            assert metric == 0.0 and want == 0.0
        else:
            assert want > 1e-3 and abs(metric - want) <= 1e-9 * want, (b, metric, want)
