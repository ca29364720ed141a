"""blindno_fp_propagate_nd (csrc/fpe_nd.hip), the grid-resident Fokker-Planck propagator, on the
HIP device (needs a GPU): bit-equality with the LDS-resident blindno_fp_propagate on 1D / 2D
grids, scipy's expm_multiply of tests/fpe3d_ref.py's independently assembled matrix on 3D grids
and on grids past the LDS kernel's 8192 cells (rel-L2 <= 1e-9, the bar tests/test_fpe.py holds the
LDS kernel to), batch independence, determinism, buffer bounds, mass conservation, argument
checks, and the two generators that depend on it (fpe_2d_dataset at 128 x 128, fpe_3d_dataset
feeding NIOFP3D).

Every kernel case runs degree 18, B = 3 distinct trajectories, nout = 4 and substeps 1 and 3, with
the substep length at the integrator's own bound ||h M||_1 = 1/2 (fpe.THETA).
"""
import ctypes

import numpy as np
import pytest
import torch

import fpe3d_ref
from conftest import rel_l2
from fpe3d_ref import NM, initial, make_sim

pytestmark = pytest.mark.gpu

DEGREE, NOUT, B = 18, 4, 3
INVALID = 1          # hipErrorInvalidValue


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")


def _batch(dims, periodic, fields=True):
    sims = [make_sim(dims, periodic, k, fields) for k in range(B)]
    p0 = np.stack([initial(s, k) for k, s in enumerate(sims)])
    h = 0.5 / (2.0 * max(float(s.coefficients_nd()[0].max()) for s in sims))
    return sims, p0, h


def _run_nd(sims, p0, dims, substeps, h, nout=NOUT, degree=DEGREE):
    from blindno._lib import call, ptr, query, stream_ptr
    coef = torch.from_numpy(np.stack([s.coefficients_nd() for s in sims])).cuda()
    p0_d = torch.from_numpy(np.ascontiguousarray(p0)).cuda()
    n = len(sims)
    out = torch.full((n, nout, p0.shape[1]), float("nan"), dtype=torch.float64, device="cuda")
    scratch = torch.full((query("blindno_fp_propagate_nd_scratch_doubles", n, *dims),), float("nan"),
                         dtype=torch.float64, device="cuda")
    call("blindno_fp_propagate_nd", ptr(p0_d), ptr(coef), ptr(out), ptr(scratch), n, *dims, nout, substeps,
         degree, substeps * h, stream_ptr())
    torch.cuda.synchronize()
    return out.cpu().numpy()


def _run_lds(sims, p0, dims, substeps, h, nout=NOUT, degree=DEGREE, dt_out=None):
    from blindno._lib import call, ptr, stream_ptr
    dt_out = substeps * h if dt_out is None else dt_out
    coef = torch.from_numpy(np.stack([s.coefficients() for s in sims])).cuda()
    p0_d = torch.from_numpy(np.ascontiguousarray(p0)).cuda()
    out = torch.full((len(sims), nout, p0.shape[1]), float("nan"), dtype=torch.float64, device="cuda")
    call("blindno_fp_propagate", ptr(p0_d), ptr(coef), ptr(out), len(sims), dims[0], dims[1], nout, substeps,
         degree, dt_out, stream_ptr())
    torch.cuda.synchronize()
    return out.cpu().numpy()


_REF = {}


def _reference(name, sims, p0, h):
    """expm_multiply records at t = 0, h, 2h, ... 9h per trajectory (computed once per case;
    substeps s reads rows 0, s, 2s, 3s)."""
    if name not in _REF:
        _REF[name] = np.stack([fpe3d_ref.propagate(fpe3d_ref.matrix_of(s), p0[k], 9 * h, 10)
                               for k, s in enumerate(sims)])
        _REF[name].setflags(write=False)
    return _REF[name]


# ---- 1. nz = 1: bit-equal to the LDS kernel
@pytest.mark.parametrize("substeps", [1, 3])
@pytest.mark.parametrize("dims,periodic", [((37, 1, 1), (False, False, False)),
                                           ((13, 11, 1), (False, True, False)),
                                           ((90, 90, 1), (False, False, False))])
def test_bit_equal_to_lds_kernel(dims, periodic, substeps):
    _need_gpu()
    sims, p0, h = _batch(dims, periodic)
    got = _run_nd(sims, p0, dims, substeps, h)
    ref = _run_lds(sims, p0, dims, substeps, h)
    assert np.isfinite(ref).all() and not np.array_equal(ref[:, 0], ref[:, -1])
    assert got.tobytes() == ref.tobytes(), np.abs(got - ref).max()


@pytest.mark.parametrize("degree,substeps", [(1, 1), (1, 2), (1, 3), (2, 3), (3, 2)])
def test_low_degrees_bit_equal_to_lds_kernel(degree, substeps):
    """Degree 1 is the one case where the pass reads its neighbours from p itself (p cannot be
    updated in place and moves through the scratch buffers); degrees 2 and 3 end on either iterate."""
    _need_gpu()
    dims = (13, 11, 1)
    sims, p0, h = _batch(dims, (False, True, False))
    got = _run_nd(sims, p0, dims, substeps, h, degree=degree)
    ref = _run_lds(sims, p0, dims, substeps, h, degree=degree)
    assert np.isfinite(ref).all() and got.tobytes() == ref.tobytes()


# ---- 2. against expm_multiply of the independent matrix
CASES = {"5x4x3_periodic": ((5, 4, 3), (True, True, True)),
         "7x6x5_reflecting": ((7, 6, 5), (False, False, False)),
         "17x33x9": ((17, 33, 9), (False, True, False)),
         "96x95x1": ((96, 95, 1), (False, False, False)),
         "21x20x22": ((21, 20, 22), (False, False, True))}


@pytest.mark.parametrize("substeps", [1, 3])
@pytest.mark.parametrize("name", list(CASES))
def test_matches_expm_multiply(name, substeps):
    _need_gpu()
    dims, periodic = CASES[name]
    sims, p0, h = _batch(dims, periodic)
    assert int(np.prod(dims)) > 8192 or dims[2] > 1          # no case the LDS kernel could run
    got = _run_nd(sims, p0, dims, substeps, h)
    ref = _reference(name, sims, p0, h)[:, ::substeps][:, :NOUT]
    assert np.array_equal(got[:, 0], p0)
    errs = [rel_l2(got[k], ref[k]) for k in range(B)]
    moved = [rel_l2(ref[k, -1], ref[k, 0]) for k in range(B)]
    print(f"{name} substeps {substeps}: rel-L2 {errs}, the density itself moved {moved}")
    assert min(moved) > 1e-3                                 # the interval is not a no-op
    assert max(errs) <= 1e-9, errs


# ---- 3. independence and determinism
@pytest.mark.parametrize("substeps", [1, 3])
def test_batch_independence_and_determinism(substeps):
    _need_gpu()
    dims, periodic = CASES["17x33x9"]
    sims, p0, h = _batch(dims, periodic)
    a = _run_nd(sims, p0, dims, substeps, h)
    b = _run_nd(sims, p0, dims, substeps, h)
    assert a.tobytes() == b.tobytes()
    for k in range(B):
        one = _run_nd(sims[k:k + 1], p0[k:k + 1], dims, substeps, h)
        assert one[0].tobytes() == a[k].tobytes(), k


# ---- 4. buffers: every out element written, nothing outside out and scratch
@pytest.mark.parametrize("substeps,degree", [(1, 18), (3, 18), (3, 1), (2, 2)])
def test_buffers_stay_in_bounds(substeps, degree):
    _need_gpu()
    from blindno._lib import call, ptr, query, stream_ptr
    dims, periodic = CASES["17x33x9"]                       # 5049 cells: no multiple of the tile
    sims, p0, h = _batch(dims, periodic)
    N, Mg = p0.shape[1], 256
    n_out, n_scr = B * NOUT * N, query("blindno_fp_propagate_nd_scratch_doubles", B, *dims)
    assert n_scr == 2 * B * N
    bufs = []
    for n in (n_out, n_scr):
        t = torch.full((n + 2 * Mg,), float("nan"), dtype=torch.float64, device="cuda")
        t[:Mg] = -7.25
        t[-Mg:] = -7.25
        bufs.append(t)
    coef = torch.from_numpy(np.stack([s.coefficients_nd() for s in sims])).cuda()
    p0_d = torch.from_numpy(p0).cuda()
    call("blindno_fp_propagate_nd", ptr(p0_d), ptr(coef), ptr(bufs[0][Mg:]), ptr(bufs[1][Mg:]), B, *dims, NOUT,
         substeps, degree, substeps * h, stream_ptr())
    torch.cuda.synchronize()
    out = bufs[0][Mg:-Mg].cpu().numpy()
    assert np.isfinite(out).all()
    for t in bufs:
        assert bool((t[:Mg] == -7.25).all()) and bool((t[-Mg:] == -7.25).all())
    assert torch.equal(p0_d.cpu(), torch.from_numpy(p0))
    if degree == 18:                                         # the sliced buffers change no result
        assert out.tobytes() == _run_nd(sims, p0, dims, substeps, h).tobytes()


# ---- 5. mass between reflecting walls
@pytest.mark.parametrize("substeps", [1, 3])
@pytest.mark.parametrize("dims", [(7, 6, 5), (21, 20, 22), (96, 95, 1)])
def test_mass_is_conserved(dims, substeps):
    _need_gpu()
    sims, p0, h = _batch(dims, (False, False, False))
    got = _run_nd(sims, p0, dims, substeps, h)
    mass = got.sum(axis=-1)
    print(f"{dims} substeps {substeps}: max |sum p - 1| = {np.abs(mass - 1).max():.3e}")
    assert np.abs(mass - 1.0).max() <= 1e-12


# ---- 6. rejected arguments launch nothing
def test_rejects_bad_arguments():
    _need_gpu()
    import blindno
    from blindno._lib import stream_ptr
    lib = blindno.load_library()
    dims = (5, 4, 3)
    sims, p0, h = _batch(dims, (True, True, True))
    N = p0.shape[1]
    coef = torch.from_numpy(np.stack([s.coefficients_nd() for s in sims])).cuda()
    p0_d = torch.from_numpy(p0).cuda()
    out = torch.full((B, NOUT, N), -3.5, dtype=torch.float64, device="cuda")
    scratch = torch.full((2 * B * N,), -3.5, dtype=torch.float64, device="cuda")
    P = lambda t: ctypes.c_void_p(t.data_ptr())   # noqa: E731
    st = stream_ptr()
    good = dict(B=B, nx=5, ny=4, nz=3, nout=NOUT, substeps=1, degree=DEGREE)
    bad = [dict(B=0), dict(B=-1), dict(nx=0), dict(ny=0), dict(nz=0), dict(nz=-2), dict(nout=0), dict(substeps=0),
           dict(degree=0), dict(nx=1 << 14, ny=1 << 14, nz=1 << 14), dict(nx=2 ** 31 - 1, ny=2 ** 31 - 1, nz=2 ** 31 - 1)]
    for kw in bad:
        a = dict(good, **kw)
        rc = lib.blindno_fp_propagate_nd(P(p0_d), P(coef), P(out), P(scratch), a["B"], a["nx"], a["ny"], a["nz"],
                                         a["nout"], a["substeps"], a["degree"], h, st)
        assert rc == INVALID, (kw, rc)
    rc = lib.blindno_fp_propagate_nd(P(p0_d), P(coef), P(out), None, *[good[k] for k in good], h, st)
    assert rc == INVALID                                     # a null scratch
    torch.cuda.synchronize()
    assert bool((out == -3.5).all()) and bool((scratch == -3.5).all())     # nothing ran
    rc = lib.blindno_fp_propagate_nd(P(p0_d), P(coef), P(out), P(scratch), *[good[k] for k in good], h, st)
    torch.cuda.synchronize()
    assert rc == 0 and bool(torch.isfinite(out).all())


# ---- propagate_many dispatch: the grid-resident path through the public interface
def test_propagate_many_dispatch():
    """A 3D grid and a 2D grid past 8192 cells run through propagate_many / propagate_interval
    (their own substep counts, TAYLOR_DEGREE) and match expm_multiply; a small 2D grid still
    gives the LDS kernel's bits."""
    _need_gpu()
    from blindno import fpe
    for name in ("7x6x5_reflecting", "96x95x1"):
        dims, periodic = CASES[name]
        sims, p0, h = _batch(dims, periodic)
        res = fpe.propagate_many(sims, list(p0), 9 * h, Nsteps=4)
        ref = _reference(name, sims, p0, h)[:, ::3]
        for k, (t, Pt) in enumerate(res):
            assert np.allclose(t, np.linspace(0, 9 * h, 4)) and Pt.shape == (4,) + tuple(sims[k].Ngrid)
            assert rel_l2(Pt.reshape(4, -1), ref[k]) <= 1e-9
    dims = (13, 11, 1)
    sims, p0, h = _batch(dims, (False, True, False))
    t, Pt = sims[0].propagate_interval(p0[0], 9 * h, Nsteps=4)
    dt_out = 9 * h / 3
    s = fpe.substeps_for(sims[0].coefficients(), dt_out)
    lds = _run_lds(sims[:1], p0[:1] / np.sum(p0[0]), dims, s, None, dt_out=dt_out)
    assert Pt.reshape(4, -1).tobytes() == lds[0].tobytes()


# ---- 7. the 2D generator on a 128 x 128 grid
def test_fpe_2d_dataset_at_128():
    _need_gpu()
    from blindno import datagen
    np.random.seed(11)
    d = datagen.fpe_2d_dataset(M=1, nsteps=3, extent=1280 * NM)
    tr = d["trajectories"]
    assert tr.shape == (1, 3, 128, 128) and d["grid"].shape == (1, 2, 128, 128)
    assert d["potential"].shape == d["drag"].shape == (1, 128, 128)
    assert (tr >= 0).all() and np.abs(tr.reshape(3, -1).sum(-1) - 1.0).max() <= 1e-10
    assert rel_l2(tr[0, 2], tr[0, 0]) > 1e-2


# ---- 8. the 3D generator feeding NIOFP3D
def test_fpe_3d_dataset_trains_niofp3d():
    _need_gpu()
    import blindno
    from blindno import data, datagen, ops
    np.random.seed(12)
    d = datagen.fpe_3d_dataset(M=2, nsteps=6, extent=80 * NM)
    assert set(d) == {"time", "grid", "trajectories", "potential", "drag"}
    tr = d["trajectories"]
    assert tr.shape == (2, 6, 8, 8, 8) and d["grid"].shape == (2, 3, 8, 8, 8) and d["time"].shape == (2, 6)
    assert d["potential"].shape == d["drag"].shape == (2, 8, 8, 8)
    assert (tr >= 0).all() and np.abs(tr.reshape(2, 6, -1).sum(-1) - 1.0).max() <= 1e-10
    ds = data.TrajectoryDataset3D(arrays=d)
    X, Y = data.device_tensors(ds)
    assert X.shape == (2, 6, 8, 8, 8) and Y.shape == (2, 8, 8, 8, 2)
    torch.manual_seed(0)
    m = blindno.NIOFP3D(3, 2, 32, 25, 2, 4, 3, 2, "cuda", down=True).cuda().train()
    ax = [torch.linspace(-1, 1, 8, device="cuda")] * 3
    grid = torch.stack(torch.meshgrid(*ax, indexing="ij"), -1).contiguous()
    opt = torch.optim.Adam(m.parameters(), lr=1e-3)
    before = {k: p.detach().clone() for k, p in m.named_parameters()}
    out = m(X, grid, bag_idx=np.arange(6))       # the whole 6-record bag (the train-mode draw needs T > 50)
    assert out.shape == (2, 8, 8, 8, 2)
    loss = ops.MSEFn.apply(out, Y, None)
    loss.backward()
    assert bool(torch.isfinite(loss))
    trained = [k for k, p in m.named_parameters() if p.grad is not None]
    assert set(before) - set(trained) <= {"fc0.weight", "fc0.bias"}      # fc0 enters as .data
    assert all(bool(torch.isfinite(m.get_parameter(k).grad).all()) for k in trained)
    opt.step()
    torch.cuda.synchronize()
    # Adam moves every parameter whose gradient is not exactly zero (a convolution bias ahead of a
    # batch-statistics BatchNorm has a true gradient of 0)
    moved = {k for k in trained if not torch.equal(before[k], m.get_parameter(k).detach())}
    assert moved == {k for k in trained if bool(m.get_parameter(k).grad.ne(0).any())}
    assert {k.split(".")[0] for k in moved} >= {"trunk", "branch", "fno"}
    assert all(k in moved for k in trained if k.endswith(".weight"))
