"""The grid-resident 2D GPE solver (blindno_gpe2d_solve, csrc/gpe_nd.hip), the 2D density error
(blindno_trapz2_frames), the generator, the evaluator and the 2d_GPE experiment (needs a GPU).

The checker is tests/gpe2d_ref.py: numpy.fft.fft2 with one 2D phase per kinetic step, where the
kernels factorise the step per axis.  Bars: rel-L2 1e-10 against it, the project's bar for the 1D
solver (row a14 of test_gpu_evaluators.py; two fp64 formulations of this integrator differ by
3e-14 .. 1.6e-13 over 1000 steps on the CPU, so the bar leaves >= 500x over the rounding floor);
1e-10 against the reference's own 1D goldens in the y- or x-independent case; 1e-12 for a plane
wave's analytic phase; 1e-11 for the mass over 1000 steps (the 1D test's bar; the CPU reference
drifts <= 2e-13).
"""
import functools
import os

import numpy as np
import pytest
import torch

import gpe2d_ref
from conftest import load_golden, rel_l2
from oracle import gpe_ref

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    import blindno
    blindno.load_library()


SHAPES = [(4, 4), (8, 32), (32, 8), (64, 64), (16, 256), (256, 16), (1024, 4), (4, 1024)]
B = 3
G = np.array([2.0, 0.5, 1.3])
KAPPA = np.array([2.0, 1.0, 0.2])


def _steps(shape):
    return 20 if max(shape) == 1024 else 200


@functools.lru_cache(maxsize=None)
def _case(shape, order):
    """Inputs and the numpy reference of one (shape, order): B = 3 trajectories with their own V,
    g, kappa; records for a batched psi0 (every step) and for a shared psi0 (every 7th step).
    Computed once, shared by the tests below, never modified."""
    nx, ny = shape
    rs = np.random.RandomState(nx * 7 + ny + order)
    x = np.linspace(-10, 10, nx)
    y = np.linspace(-8, 8, ny)
    V = gpe2d_ref.training_potentials(B, x, y, rs)
    base = gpe_ref.initial_condition(2, x)[:, None] * gpe_ref.initial_condition(3, y)[None, :]
    psi0 = np.stack([base * np.exp(1j * (0.3 * b * x[:, None] + 0.2 * y[None, :])) + 0.05 * b for b in range(B)])
    dt, ns = 0.005, _steps(shape)
    tf = dt * (ns + 0.5)
    full = [gpe2d_ref.solve(psi0[b], x, y, dt, tf, order, G[b], KAPPA[b], V[b]) for b in range(B)]
    sh = [gpe2d_ref.solve(psi0[1], x, y, dt, tf, order, G[b], KAPPA[b], V[b], rec_every=7) for b in range(B)]
    for a in (x, y, V, psi0):
        a.setflags(write=False)
    return dict(x=x, y=y, V=V, psi0=psi0, dt=dt, tf=tf, ns=ns, t=full[0][0], psi=np.stack([f[1] for f in full]),
                t7=sh[0][0], psi7=np.stack([s[1] for s in sh]), fin7=np.stack([s[2] for s in sh]))


@pytest.mark.parametrize("order", [2, 4])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_solver_matches_numpy_reference(shape, order):
    from blindno import gpe
    c = _case(shape, order)
    r = gpe.solve_batch_2d(c["psi0"], c["x"], c["y"], c["dt"], c["tf"], order, G, KAPPA, c["V"], want_psi=True)
    psi, ab = r["psi"].cpu().numpy(), r["abs"].cpu().numpy()
    assert psi.shape == (B, c["ns"] + 1, *shape) and ab.shape == psi.shape and np.allclose(r["t"], c["t"])
    e_psi, e_abs, e_fin = rel_l2(psi, c["psi"]), rel_l2(ab, np.abs(c["psi"])), rel_l2(r["final"].cpu().numpy(), c["psi"][:, -1])
    print(f"batched psi0 {shape} order {order}: psi {e_psi:.3e} |psi| {e_abs:.3e} final {e_fin:.3e}")
    assert e_psi <= 1e-10 and e_abs <= 1e-10 and e_fin <= 1e-10
    assert max(rel_l2(psi[b], c["psi"][b]) for b in range(B)) <= 1e-10
    # one psi0 for the batch, every 7th step (7 does not divide the step count)
    assert c["ns"] % 7 != 0
    r7 = gpe.solve_batch_2d(c["psi0"][1], c["x"], c["y"], c["dt"], c["tf"], order, G, KAPPA, c["V"], rec_every=7,
                            want_psi=True)
    psi7 = r7["psi"].cpu().numpy()
    assert psi7.shape == (B, c["ns"] // 7 + 1, *shape) and np.allclose(r7["t"], c["t7"])
    e7, ea7 = rel_l2(psi7, c["psi7"]), rel_l2(r7["abs"].cpu().numpy(), np.abs(c["psi7"]))
    ef7 = rel_l2(r7["final"].cpu().numpy(), c["fin7"])
    print(f"shared psi0 {shape} order {order} rec 7: psi {e7:.3e} |psi| {ea7:.3e} final {ef7:.3e}")
    assert e7 <= 1e-10 and ea7 <= 1e-10 and ef7 <= 1e-10


@pytest.mark.parametrize("order", [2, 4])
@pytest.mark.parametrize("axis", [0, 1])
def test_solver_reproduces_the_1d_goldens(order, axis):
    """psi0 and V constant along one axis of length 4: the length-4 transform of a constant is
    exact, so every row (column) must be the reference's own 1D trajectory."""
    from blindno import gpe
    g = load_golden(f"gpe_solve_o{order}")
    x = g["x"]
    z = np.linspace(-1, 1, 4)
    p1 = gpe.initial_condition(int(g["ic"]), x)
    rep = (lambda a: np.repeat(a[:, None], 4, 1)) if axis == 0 else (lambda a: np.repeat(a[None, :], 4, 0))
    grids = (x, z) if axis == 0 else (z, x)
    r = gpe.solve_batch_2d(rep(p1), *grids, float(g["dt"]), float(g["t_final"]), order, float(g["g"]),
                           float(g["kappa"]), rep(g["V"]), want_psi=True)
    psi = r["psi"][0].cpu().numpy()
    assert np.allclose(r["t"], g["t"]) and psi.shape[0] == g["psi"].shape[0]
    for c in range(4):
        line = psi[:, :, c] if axis == 0 else psi[:, c, :]
        e = rel_l2(line, g["psi"])
        print(f"order {order} axis {axis} line {c}: {e:.3e}")
        assert e <= 1e-10
        ab = r["abs"][0].cpu().numpy()
        assert rel_l2(ab[:, :, c] if axis == 0 else ab[:, c, :], np.abs(g["psi"])) <= 1e-10


@pytest.mark.parametrize("order", [2, 4])
def test_plane_wave_acquires_the_analytic_phase(order):
    """V = g = kappa = 0: exp(i(kx x + ky y)) on the periodic grid only turns by
    exp(-i(kx^2 + ky^2) t / 2).  Order 2 applies L(dt) once per step, so t is the time.  The
    reference's nine-stage order-4 sequence applies L(a1) L(a2) L(a2) L(a1) with a1 = 1/(2 - 2^(1/3)),
    a2 = -2^(1/3)/(2 - 2^(1/3)), whose kinetic coefficients sum to 2 (a1 + a2) = -0.7024, not 1 (the
    1D kernel and oracle.gpe_ref.step restate it as it is): there the same statement holds with the
    kinetic time 2 (a1 + a2) t that the sequence actually applies."""
    from blindno import gpe
    nx, ny = 64, 32
    Lx, Ly = 20.0, 12.0
    x = np.arange(nx) * (Lx / nx) - 10
    y = np.arange(ny) * (Ly / ny) - 6
    kx, ky = 2 * np.pi * 3 / Lx, -2 * np.pi * 5 / Ly
    psi0 = np.exp(1j * (kx * x[:, None] + ky * y[None, :]))
    dt, ns = 0.005, 200
    r = gpe.solve_batch_2d(psi0, x, y, dt, dt * (ns + 0.5), order, 0.0, 0.0, np.zeros((nx, ny)), rec_every=50,
                           want_psi=True)
    psi = r["psi"][0].cpu().numpy()
    assert psi.shape[0] == 5
    ksum = 1.0 if order == 2 else sum(c for kind, c in gpe2d_ref.stages(4) if kind == "l")
    assert order == 2 or abs(ksum - 2 * (1 - 2 ** (1 / 3)) / (2 - 2 ** (1 / 3))) < 1e-15
    for k in range(5):
        t = k * 50 * dt * ksum                                   # kinetic time after 50 k steps
        want = psi0 * np.exp(-0.5j * (kx * kx + ky * ky) * t)
        e = np.abs(psi[k] - want).max()
        print(f"order {order} t {t:.3f}: {e:.3e}")
        assert e <= 1e-12


@pytest.fixture(scope="module")
def mass_run():
    from blindno import gpe
    n = 64
    x = np.linspace(-10, 10, n)
    V = gpe.training_potentials_2d(64, x, x, np.random.RandomState(0))
    psi0 = gpe.initial_condition(2, x)[:, None] * gpe.initial_condition(2, x)[None, :]
    args = (psi0, x, x, 0.005, 5.0, 2, 2.0, 2.0)
    return args, V, gpe.solve_batch_2d(*args, V, rec_every=100, want_psi=True)


def test_mass_is_conserved_at_scale(mass_run):
    _, _, r = mass_run
    assert r["abs"].shape == (64, 11, 64, 64)
    m = (r["abs"] ** 2).sum((-1, -2))
    drift = float((m / m[:, :1] - 1).abs().max())
    print(f"mass drift over 1000 steps, B = 64: {drift:.3e}")
    assert drift <= 1e-11


def test_batch_independence_and_determinism(mass_run):
    from blindno import gpe
    args, V, r = mass_run
    one = gpe.solve_batch_2d(*args, V[17], rec_every=100, want_psi=True)
    for k in ("abs", "psi", "final"):
        assert torch.equal(one[k][0], r[k][17]), k
    again = gpe.solve_batch_2d(*args, V, rec_every=100, want_psi=True)
    for k in ("abs", "psi", "final"):
        assert torch.equal(again[k], r[k]), k


def _raw_solve(c, order, nsteps, rec_every, rabs, f32, rpsi, fin, scratch="auto", B_=B, shape=None, batched=1,
               dx=None, psi0=None):
    """blindno_gpe2d_solve through the raw binding, on caller-made buffers."""
    from blindno._lib import call, ptr, query, stream_ptr
    nx, ny = shape or c["V"].shape[1:]
    dev = "cuda"
    p0 = torch.from_numpy(np.array(c["psi0"]).view(np.float64)).to(dev) if psi0 is None else psi0
    Vd = torch.from_numpy(np.array(c["V"])).to(dev)
    gd, kd = torch.from_numpy(G).to(dev), torch.from_numpy(KAPPA).to(dev)
    if isinstance(scratch, str):
        scratch = torch.empty(max(1, query("blindno_gpe2d_scratch_doubles", B, *c["V"].shape[1:])), dtype=torch.float64,
                              device=dev)
    dx = float(c["x"][1] - c["x"][0]) if dx is None else dx
    return call("blindno_gpe2d_solve", ptr(p0), ptr(Vd), ptr(gd), ptr(kd), dx, float(c["y"][1] - c["y"][0]),
                c["dt"], nsteps, order, rec_every, ptr(rabs), f32, ptr(rpsi), ptr(fin), ptr(scratch), B_, nx, ny,
                batched, stream_ptr())


@pytest.mark.parametrize("shape", [(8, 32), (64, 64)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_outputs_fully_written_margins_untouched(shape):
    """Outputs NaN-prefilled between sentinel margins: every element written, no margin touched;
    the fp32 |psi| record is the fp64 one rounded; each output works on its own."""
    c = _case(shape, 2)
    nx, ny = shape
    ns, re_ = 20, 7
    nrec = ns // re_ + 1
    M = 64                                                     # margin, doubles (16-byte aligned)

    def guarded(n, dtype=torch.float64):
        t = torch.full((n + 2 * M,), -777.0, dtype=dtype, device="cuda")
        t[M:M + n] = float("nan")
        return t

    def check(t, n):
        assert bool((t[:M] == -777.0).all()) and bool((t[M + n:] == -777.0).all()), "margin overwritten"
        assert not bool(torch.isnan(t[M:M + n]).any()), "output not fully written"
        return t[M:M + n]

    n_abs, n_psi, n_fin = B * nrec * nx * ny, 2 * B * nrec * nx * ny, 2 * B * nx * ny
    a64, a32, ps, fi = guarded(n_abs), guarded(n_abs, torch.float32), guarded(n_psi), guarded(n_fin)
    _raw_solve(c, 2, ns, re_, a64[M:], 0, ps[M:], fi[M:])
    abs64, psi, fin = check(a64, n_abs), check(ps, n_psi), check(fi, n_fin)
    want = torch.from_numpy(np.ascontiguousarray(c["psi"][:, 0:ns + 1:re_]).view(np.float64)).cuda().reshape(-1)
    assert rel_l2(psi.cpu().numpy(), want.cpu().numpy()) <= 1e-10
    pc = torch.view_as_complex(psi.view(B, nrec, nx, ny, 2))
    assert rel_l2(abs64.view(B, nrec, nx, ny).cpu().numpy(), pc.abs().cpu().numpy()) <= 1e-14
    # the step-20 field is not a recorded step (20 % 7 != 0): final comes from its own store
    assert rel_l2(torch.view_as_complex(fin.view(B, nx, ny, 2)).cpu().numpy(), c["psi"][:, ns]) <= 1e-10
    # fp32 record alone (no psi, no final)
    _raw_solve(c, 2, ns, re_, a32[M:], 1, None, None)
    assert torch.equal(check(a32, n_abs), abs64.to(torch.float32))
    # psi alone / final alone
    ps2, fi2 = guarded(n_psi), guarded(n_fin)
    _raw_solve(c, 2, ns, re_, None, 0, ps2[M:], None)
    assert torch.equal(check(ps2, n_psi), psi)
    _raw_solve(c, 2, ns, re_, None, 0, None, fi2[M:])
    assert torch.equal(check(fi2, n_fin), fin)
    # no steps at all: the record is psi0 and so is the final field
    ps3, fi3 = guarded(2 * B * nx * ny), guarded(n_fin)
    _raw_solve(c, 2, 0, 1, None, 0, ps3[M:], fi3[M:])
    p0 = torch.from_numpy(np.array(c["psi0"]).view(np.float64)).cuda().reshape(-1)
    assert torch.equal(check(ps3, 2 * B * nx * ny), p0) and torch.equal(check(fi3, n_fin), p0)


def test_python_outputs_on_their_own():
    from blindno import gpe
    c = _case((8, 32), 2)
    a = (c["psi0"], c["x"], c["y"], c["dt"], c["tf"], 2, G, KAPPA, c["V"])
    both = gpe.solve_batch_2d(*a, rec_every=7, want_psi=True)
    only_abs = gpe.solve_batch_2d(*a, rec_every=7)
    only_psi = gpe.solve_batch_2d(*a, rec_every=7, want_abs=False, want_psi=True)
    f32 = gpe.solve_batch_2d(*a, rec_every=7, abs_dtype=torch.float32)
    assert sorted(only_abs) == ["abs", "final", "t"] and sorted(only_psi) == ["final", "psi", "t"]
    assert torch.equal(only_abs["abs"], both["abs"]) and torch.equal(only_psi["psi"], both["psi"])
    assert f32["abs"].dtype == torch.float32 and torch.equal(f32["abs"], both["abs"].to(torch.float32))
    assert torch.equal(f32["final"], both["final"])


def test_refusals_leave_the_stream_usable():
    """Every refusal of the C entry (hipErrorInvalidValue before any launch) and of the Python
    guards raises BlindnoError; a valid solve on the same stream then still gives the right
    answer."""
    from blindno import gpe
    from blindno._lib import BlindnoError
    c = _case((8, 32), 2)
    nrec = 3
    rabs = torch.empty(B * nrec * 8 * 32, dtype=torch.float64, device="cuda")
    fin = torch.empty(2 * B * 8 * 32, dtype=torch.float64, device="cuda")
    ok = dict(order=2, nsteps=2, rec_every=1)
    bad = [dict(shape=(12, 32)), dict(shape=(8, 2)), dict(shape=(2048, 32)), dict(shape=(8, 0)), dict(order=3),
           dict(order=1), dict(rec_every=0), dict(rec_every=-2), dict(scratch=None), dict(B_=0), dict(nsteps=-1),
           dict(dx=0.0), dict(f32=2), dict(psi0=fin[1:])]
    for kw in bad:
        a = dict(ok, f32=0)
        a.update(kw)
        with pytest.raises(BlindnoError, match="blindno_gpe2d_solve failed"):
            _raw_solve(c, a.pop("order"), a.pop("nsteps"), a.pop("rec_every"), rabs, a.pop("f32"), None, fin, **a)
    with pytest.raises(BlindnoError, match="blindno_trapz2_frames failed"):
        from blindno._lib import call, ptr, stream_ptr
        call("blindno_trapz2_frames", ptr(rabs), ptr(rabs), ptr(rabs), ptr(rabs), ptr(fin), 0, 8, 32, stream_ptr())
    args = (c["psi0"], c["x"], c["y"])
    for kw, pat in [(dict(dt=1.0, t_final=gpe.MAX_LAUNCHES_2D // 2 + 1.5, rec_every=1 << 30), "MAX_LAUNCHES_2D"),
                    (dict(dt=0.005, t_final=5.0, order=3), "order"),
                    (dict(dt=0.005, t_final=5.0, rec_every=0), "rec_every")]:
        a = dict(order=2, rec_every=1)
        a.update(kw)
        with pytest.raises(BlindnoError, match=pat):
            gpe.solve_batch_2d(*args, a["dt"], a["t_final"], a["order"], G, KAPPA, c["V"], rec_every=a["rec_every"])
    big = np.broadcast_to(c["V"][:1, :1, :1], (64, 256, 256))
    xb = np.linspace(-10, 10, 256)
    with pytest.raises(BlindnoError, match="MAX_RECORD_BYTES"):
        gpe.solve_batch_2d(np.ones((256, 256), complex), xb, xb, 0.005, 5.0, 2, 2, 2, big)
    with pytest.raises(BlindnoError, match="power of two"):
        gpe.solve_batch_2d(np.ones((12, 32), complex), np.linspace(0, 1, 12), c["y"], 0.005, 0.1, 2, 1, 1, np.zeros((12, 32)))
    torch.cuda.synchronize()
    r = gpe.solve_batch_2d(*args, c["dt"], c["tf"], 2, G, KAPPA, c["V"], want_psi=True)
    assert rel_l2(r["psi"].cpu().numpy(), c["psi"]) <= 1e-10


def test_generator_matches_reference():
    from blindno import gpe
    ref = gpe2d_ref.generate(3, 32, 32, rng=np.random.RandomState(11))
    d64 = gpe.generate_training_data_2d(3, 32, 32, rng=np.random.RandomState(11), y_dtype=np.float64, batch=2)
    d32 = gpe.generate_training_data_2d(3, 32, 32, rng=np.random.RandomState(11))
    assert sorted(d64) == sorted(ref) == ["V", "g", "kappa", "y"]
    assert d64["y"].shape == ref["y"].shape == (3, 101, 32, 32) and d64["y"].dtype == np.float64
    assert np.allclose(d64["V"], ref["V"], rtol=1e-14, atol=0) and np.array_equal(d64["g"], ref["g"])
    assert np.array_equal(d64["kappa"], ref["kappa"])
    e = rel_l2(d64["y"], ref["y"])
    print(f"generator vs reference: {e:.3e}")
    assert e <= 1e-10
    assert d32["y"].dtype == np.float32 and np.array_equal(d32["y"], d64["y"].astype(np.float32))
    assert np.array_equal(d32["V"], d64["V"])


def test_time_averaged_L2_error_2d():
    from blindno import gpe
    rs = np.random.RandomState(4)
    nt, nx, ny = 7, 33, 20                                       # any grid: the integral is not an FFT
    x = np.sort(rs.uniform(-3, 3, nx))                           # non-uniform spacings as numpy.trapz takes them
    y = np.linspace(-2, 5, ny)
    t = np.sort(rs.uniform(0, 2, nt))
    ref, pred = rs.rand(nt, nx, ny) + 0.1, rs.rand(nt, nx, ny) + 0.1
    want = gpe2d_ref.time_averaged_L2_error(t, ref, pred, x, y)
    v = gpe.time_averaged_L2_error_2d(t, ref, t, pred, (x, y))
    v2 = gpe.time_averaged_L2_error_2d(t, torch.from_numpy(ref).cuda(), t, torch.from_numpy(pred).cuda(), [x, y])
    print(f"2D density error: {v!r} vs numpy {want!r}")
    assert abs(v - want) <= 1e-12 * abs(want) and abs(v2 - want) <= 1e-12 * abs(want)
    with pytest.raises(ValueError):
        gpe.time_averaged_L2_error_2d(t, ref, t, pred[:, :-1], (x, y))
    with pytest.raises(ValueError):
        gpe.time_averaged_L2_error_2d(t, ref, t, pred, (x,))


def test_compute_time_error_gpe_2d_pipeline(tmp_path):
    """One batched pipeline against its steps run one trajectory at a time."""
    from blindno import NIOFP2D_FNO, evaluate, gpe, timeerror
    rs = np.random.RandomState(9)
    T, N = 21, 64
    mk = lambda m: dict(y=rs.rand(m, T, N, N), V=rs.rand(m, N, N) * 3, g=rs.rand(m), kappa=rs.rand(m) * 0.1)  # noqa: E731
    train, test = mk(4), mk(3)
    models = {}
    for name, seed in (("fno", 1), ("fno_b", 2)):
        torch.manual_seed(seed)
        models[name] = NIOFP2D_FNO(2, 3, 100, 25, 2, 6, 5, 1, heads=("fno_V",)).cuda()
    kw = dict(t_final=0.5, dt=0.005, rec_every=5)
    errs = timeerror.compute_time_error_gpe_2d(models, train, test, [2, 0, 7], outdir=str(tmp_path), **kw)
    assert list(errs) == ["fno", "fno_b"] and errs["fno"].shape == (2,)
    sc = evaluate.compute_train_scalers_gpe(train)
    tn = evaluate.normalize_gpe(test, sc)
    x = np.linspace(-10, 10, N)
    psi0 = gpe.initial_condition(2, x)[:, None] * gpe.initial_condition(2, x)[None, :]
    i = 2
    pv = evaluate.predict(models["fno_b"], torch.tensor(tn["y"][i][None], dtype=torch.float32, device="cuda"),
                          evaluate.grid2d(N, N, "cuda")).cpu().numpy()[0, :, :, 0] * sc["V_max"]
    one = lambda V: gpe.solve_batch_2d(psi0, x, x, kw["dt"], kw["t_final"], 2, test["g"][i], test["kappa"][i], V,  # noqa: E731
                                       rec_every=5)
    a, b = one(tn["V"][i] * sc["V_max"]), one(pv)
    e = gpe.time_averaged_L2_error_2d(a["t"], a["abs"][0], b["t"], b["abs"][0], (x, x))
    assert np.isfinite(e) and e > 0
    # the solver and the integrals are independent of the batch bit for bit; the fp32 model forward
    # may order its sums differently for one sample than for two (predicted V moves by a few fp32
    # ulps), the bar test_fpe.py's 2D pipeline test sets for the same reason
    print(f"pipeline {errs['fno_b'][0]!r} vs one at a time {e!r}")
    assert abs(errs["fno_b"][0] - e) <= 1e-6 * e + 1e-15
    d = np.load(tmp_path / "fno" / "sample_0_V_and_err.npy", allow_pickle=True).item()
    assert d["Err_L2_rel"] == errs["fno"][1] and d["pred_V"].shape == (N, N)
    assert np.load(tmp_path / "ErrL2_relative_fno_Nsamples_2.npy").shape == (2,)


def test_trainer_2d_gpe_end_to_end(tmp_path):
    """Generate 10 orbits at 64^2 (a power of two whose padded size 80 holds 2 x 32 modes), train
    the 2d_GPE experiment for 2 epochs at batch 4."""
    from blindno import evaluate, gpe, trainer
    d = gpe.generate_training_data_2d(10, 64, 64, rng=np.random.RandomState(2))
    assert d["y"].shape == (10, 101, 64, 64) and d["y"].dtype == np.float32
    data = str(tmp_path / "gpe2d.npy")
    gpe.save_training_data(d, data)
    out = str(tmp_path / "results_2d_GPE_fno")
    exp = trainer._experiments()["2d_GPE"]
    t = trainer.Trainer(exp, data, out, torch.device("cuda"), epochs=2, save_interval=2, batch=4, log=lambda s: None)
    hist = t.fit()
    assert len(t.train_idx) == 8 and len(hist["train_losses"]) == 2 and len(hist["test_losses"]) == 1
    assert all(np.isfinite(v) for v in hist["train_losses"] + hist["test_losses"])
    ck = f"model_checkpoint_best_{hist['test_losses'][0]:.6f}.pt"
    assert sorted(os.listdir(out)) == sorted([ck, "test_losses.npy", "train_losses.npy"])   # the 1D GPE names
    sd = evaluate.load_checkpoint_robust(os.path.join(out, ck))
    assert any(k.startswith("fno_V.") for k in sd) and not any(k.startswith("fno_drift.") for k in sd)
    model = exp.model(64, "cuda")
    model.load_state_dict(sd)
    pred = evaluate.predict(model.cuda(), t.Xte, t.grid, 2)
    assert pred.shape == (2, 64, 64, 1) and bool(torch.isfinite(pred).all())
