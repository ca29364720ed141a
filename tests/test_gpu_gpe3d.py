"""The grid-resident 3D GPE solver (blindno_gpe3d_solve, csrc/gpe_nd.hip), the 3D density error
(blindno_trapz3_frames), the generator and the evaluator (needs a GPU).

The checker is tests/gpe3d_ref.py: numpy.fft.fftn with one 3D phase per kinetic step, where the
kernels factorise the step per axis.  Bars: rel-L2 1e-10 against it and against solve_batch_2d /
the reference's own 1D goldens when one or two axes carry nothing (the project's bar for the 1D
and 2D solvers); 1e-12 for a plane wave's analytic phase; 1e-11 for the mass over 1000 steps;
1e-12 relative for the density error against numpy.trapz applied three times.
"""
import functools
import itertools

import numpy as np
import pytest
import torch

import gpe2d_ref
import gpe3d_ref
from conftest import load_golden, rel_l2
from oracle import gpe_ref

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    import blindno
    blindno.load_library()


MAX_N = 1024                                                     # BLINDNO_GPE3D_MAX_N
SHAPES = [(4, 4, 4), (4, 8, 16), (16, 4, 8), (8, 16, 4), (32, 8, 4), (64, 4, 4), (4, 64, 4), (4, 4, 64),
          (16, 16, 16), (32, 32, 32), (MAX_N, 4, 4), (4, MAX_N, 4), (4, 4, MAX_N)]
B = 3
G = np.array([2.0, 0.5, 0.0])                                    # the last trajectory is linear
KAPPA = np.array([2.0, 1.0, 0.0])
NS, DT = 7, 0.005
TF = DT * (NS + 0.5)


def _grids(shape):
    return tuple(np.linspace(-L, L, n) for L, n in zip((10, 8, 6), shape))   # dx != dy != dz


@functools.lru_cache(maxsize=None)
def _case(shape, order):
    """Inputs and the numpy reference of one (shape, order): B = 3 trajectories with their own V,
    g, kappa; records for a batched psi0 (every step) and for a shared psi0 (every 3rd step).
    Computed once, shared by the tests below, never modified."""
    rs = np.random.RandomState(shape[0] * 49 + shape[1] * 7 + shape[2] + order)
    x, y, z = _grids(shape)
    V = gpe3d_ref.training_potentials(B, x, y, z, rs)
    f = gpe_ref.initial_condition
    base = f(2, x)[:, None, None] * f(3, y)[None, :, None] * f(1, z)[None, None, :]
    ph = 0.3 * x[:, None, None] + 0.2 * y[None, :, None] - 0.25 * z[None, None, :]
    psi0 = np.stack([base * np.exp(1j * (b + 1) * ph) + 0.05 * b for b in range(B)])
    full = [gpe3d_ref.solve(psi0[b], x, y, z, DT, TF, order, G[b], KAPPA[b], V[b]) for b in range(B)]
    sh = [gpe3d_ref.solve(psi0[1], x, y, z, DT, TF, order, G[b], KAPPA[b], V[b], rec_every=3) for b in range(B)]
    for a in (x, y, z, V, psi0):
        a.setflags(write=False)
    return dict(x=x, y=y, z=z, V=V, psi0=psi0, t=full[0][0], psi=np.stack([r[1] for r in full]),
                t3=sh[0][0], psi3=np.stack([s[1] for s in sh]), fin3=np.stack([s[2] for s in sh]))


@pytest.mark.parametrize("order", [2, 4])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_solver_matches_numpy_reference(shape, order):
    from blindno import gpe
    c = _case(shape, order)
    a = (c["x"], c["y"], c["z"], DT, TF, order, G, KAPPA, c["V"])
    r = gpe.solve_batch_3d(c["psi0"], *a, want_psi=True)
    psi, ab = r["psi"].cpu().numpy(), r["abs"].cpu().numpy()
    assert psi.shape == (B, NS + 1, *shape) and ab.shape == psi.shape and np.allclose(r["t"], c["t"])
    e_psi, e_abs, e_fin = rel_l2(psi, c["psi"]), rel_l2(ab, np.abs(c["psi"])), rel_l2(r["final"].cpu().numpy(), c["psi"][:, -1])
    print(f"batched psi0 {shape} order {order}: psi {e_psi:.3e} |psi| {e_abs:.3e} final {e_fin:.3e}")
    assert e_psi <= 1e-10 and e_abs <= 1e-10 and e_fin <= 1e-10
    assert max(rel_l2(psi[b], c["psi"][b]) for b in range(B)) <= 1e-10
    # one psi0 for the batch, every 3rd step (3 does not divide 7)
    r3 = gpe.solve_batch_3d(c["psi0"][1], *a, rec_every=3, want_psi=True)
    psi3 = r3["psi"].cpu().numpy()
    assert psi3.shape == (B, NS // 3 + 1, *shape) and np.allclose(r3["t"], c["t3"])
    e3, ea3 = rel_l2(psi3, c["psi3"]), rel_l2(r3["abs"].cpu().numpy(), np.abs(c["psi3"]))
    ef3 = rel_l2(r3["final"].cpu().numpy(), c["fin3"])
    print(f"shared psi0 {shape} order {order} rec 3: psi {e3:.3e} |psi| {ea3:.3e} final {ef3:.3e}")
    assert e3 <= 1e-10 and ea3 <= 1e-10 and ef3 <= 1e-10
    assert max(rel_l2(psi3[b], c["psi3"][b]) for b in range(B)) <= 1e-10
    # the float32 |psi| record is the fp64 record rounded once
    f32 = gpe.solve_batch_3d(c["psi0"][1], *a, rec_every=3, abs_dtype=torch.float32)
    assert f32["abs"].dtype == torch.float32 and torch.equal(f32["abs"], r3["abs"].to(torch.float32))
    assert torch.equal(f32["final"], r3["final"])


def _problem2(n1, n2, seed):
    rs = np.random.RandomState(seed)
    a, b = np.linspace(-10, 10, n1), np.linspace(-8, 8, n2)
    V = gpe2d_ref.training_potentials(2, a, b, rs)
    p = gpe_ref.initial_condition(2, a)[:, None] * gpe_ref.initial_condition(3, b)[None, :] * np.exp(0.3j * a)[:, None]
    return a, b, V, np.stack([p, p * np.exp(0.2j * b)[None, :] + 0.05])


@pytest.mark.parametrize("order", [2, 4])
@pytest.mark.parametrize("axis", [0, 1, 2])
def test_reduces_to_the_2d_solver(axis, order):
    """Inputs constant along one axis (4 points): every slice across it is solve_batch_2d's
    result on the other two axes."""
    from blindno import gpe
    a, b, V2, p2 = _problem2(8, 16, axis)
    c = np.linspace(-3, 3, 4)
    g, k = np.array([1.5, 0.4]), np.array([0.7, 2.0])
    r2 = gpe.solve_batch_2d(p2, a, b, DT, TF, order, g, k, V2, rec_every=3, want_psi=True)
    grids = [a, b]
    grids.insert(axis, c)
    rep = lambda f: np.repeat(np.expand_dims(f, axis + 1), 4, axis + 1)     # noqa: E731
    r3 = gpe.solve_batch_3d(rep(p2), *grids, DT, TF, order, g, k, rep(V2), rec_every=3, want_psi=True)
    assert np.allclose(r3["t"], r2["t"])
    for s in range(4):
        e = [rel_l2(np.take(r3[key].cpu().numpy(), s, ax), r2[key].cpu().numpy())
             for key, ax in (("psi", axis + 2), ("abs", axis + 2), ("final", axis + 1))]
        print(f"order {order} constant axis {axis} slice {s}: psi {e[0]:.3e} |psi| {e[1]:.3e} final {e[2]:.3e}")
        assert max(e) <= 1e-10


@pytest.mark.parametrize("order", [2, 4])
@pytest.mark.parametrize("axis", [0, 1, 2])
def test_solver_reproduces_the_1d_goldens(order, axis):
    """psi0 and V depend on one axis only, the other two have 4 points (the length-4 transform of a
    constant is exact): every line along that axis must be the reference's own 1D trajectory."""
    from blindno import gpe
    g = load_golden(f"gpe_solve_o{order}")
    x = g["x"]
    grids = [np.linspace(-1, 1, 4), np.linspace(-2, 2, 4), np.linspace(-3, 3, 4)]
    grids[axis] = x
    shape = [4, 4, 4]
    shape[axis] = len(x)
    ix = [None, None, None]
    ix[axis] = slice(None)
    rep = lambda a: np.broadcast_to(a[tuple(ix)], shape)                      # noqa: E731
    r = gpe.solve_batch_3d(rep(gpe.initial_condition(int(g["ic"]), x)), *grids, float(g["dt"]), float(g["t_final"]),
                           order, float(g["g"]), float(g["kappa"]), rep(g["V"]), want_psi=True)
    psi, ab = np.moveaxis(r["psi"][0].cpu().numpy(), axis + 1, 1), np.moveaxis(r["abs"][0].cpu().numpy(), axis + 1, 1)
    assert np.allclose(r["t"], g["t"]) and psi.shape == (g["psi"].shape[0], len(x), 4, 4)
    worst = max(rel_l2(psi[:, :, i, j], g["psi"]) for i in range(4) for j in range(4))
    worst_abs = max(rel_l2(ab[:, :, i, j], np.abs(g["psi"])) for i in range(4) for j in range(4))
    print(f"order {order} axis {axis}: worst line psi {worst:.3e} |psi| {worst_abs:.3e}")
    assert worst <= 1e-10 and worst_abs <= 1e-10


def test_axis_permutations():
    """Solving transposed inputs gives the transposed result, for each of the 6 axis orders: a
    swapped stride or spacing would show (dx != dy != dz)."""
    from blindno import gpe
    c = _case((4, 8, 16), 2)
    grids = (c["x"], c["y"], c["z"])
    assert len({round(float(a[1] - a[0]), 6) for a in grids}) == 3
    base = gpe.solve_batch_3d(c["psi0"], *grids, DT, TF, 2, G, KAPPA, c["V"], rec_every=3, want_psi=True)
    for perm in itertools.permutations(range(3)):
        bp = (0,) + tuple(p + 1 for p in perm)
        r = gpe.solve_batch_3d(c["psi0"].transpose(bp), *(grids[p] for p in perm), DT, TF, 2, G, KAPPA,
                               c["V"].transpose(bp), rec_every=3, want_psi=True)
        rp = (0, 1) + tuple(p + 2 for p in perm)
        e = [rel_l2(r["psi"].cpu().numpy(), base["psi"].cpu().numpy().transpose(rp)),
             rel_l2(r["abs"].cpu().numpy(), base["abs"].cpu().numpy().transpose(rp)),
             rel_l2(r["final"].cpu().numpy(), base["final"].cpu().numpy().transpose(bp))]
        print(f"axes {perm}: psi {e[0]:.3e} |psi| {e[1]:.3e} final {e[2]:.3e}")
        assert max(e) <= 1e-10


@pytest.mark.parametrize("order", [2, 4])
def test_plane_wave_acquires_the_analytic_phase(order):
    """V = g = kappa = 0: exp(i k.x) on the periodic grid only turns by exp(-i |k|^2 t / 2).  Order 2
    applies L(dt) once per step, so t is the time; the nine-stage order-4 sequence applies the
    kinetic time 2 (a1 + a2) t (tests/test_gpu_gpe2d.py explains)."""
    from blindno import gpe
    n, L = (16, 8, 32), (20.0, 12.0, 16.0)
    x, y, z = (np.arange(m) * (l / m) - l / 2 for m, l in zip(n, L))
    k = (2 * np.pi * 3 / L[0], -2 * np.pi * 2 / L[1], 2 * np.pi * 5 / L[2])
    psi0 = np.exp(1j * (k[0] * x[:, None, None] + k[1] * y[None, :, None] + k[2] * z[None, None, :]))
    dt, ns = 0.005, 200
    r = gpe.solve_batch_3d(psi0, x, y, z, dt, dt * (ns + 0.5), order, 0.0, 0.0, np.zeros(n), rec_every=50, want_psi=True)
    psi = r["psi"][0].cpu().numpy()
    assert psi.shape[0] == 5
    ksum = 1.0 if order == 2 else sum(c for kind, c in gpe3d_ref.stages(4) if kind == "l")
    for j in range(5):
        t = j * 50 * dt * ksum                                   # kinetic time after 50 j steps
        want = psi0 * np.exp(-0.5j * sum(v * v for v in k) * t)
        e = np.abs(psi[j] - want).max()
        print(f"order {order} t {t:.3f}: {e:.3e}")
        assert e <= 1e-12


@pytest.fixture(scope="module")
def mass_run():
    from blindno import gpe
    n = 16
    x = np.linspace(-10, 10, n)
    V = gpe.training_potentials_3d(8, x, x, x, np.random.RandomState(0))
    psi0 = gpe3d_ref.initial_field(x, x, x)
    args = (psi0, x, x, x, 0.005, 5.0, 2, 2.0, 2.0)
    return args, V, gpe.solve_batch_3d(*args, V, rec_every=100, want_psi=True)


def test_mass_is_conserved(mass_run):
    _, _, r = mass_run
    assert r["abs"].shape == (8, 11, 16, 16, 16)
    m = (r["abs"] ** 2).sum((-1, -2, -3))
    drift = float((m / m[:, :1] - 1).abs().max())
    print(f"mass drift over 1000 Strang steps, B = 8: {drift:.3e}")
    assert drift <= 1e-11


def test_batch_independence_and_determinism(mass_run):
    from blindno import gpe
    args, V, r = mass_run
    one = gpe.solve_batch_3d(*args, V[5], rec_every=100, want_psi=True)
    for k in ("abs", "psi", "final"):
        assert torch.equal(one[k][0], r[k][5]), k
    again = gpe.solve_batch_3d(*args, V, rec_every=100, want_psi=True)
    for k in ("abs", "psi", "final"):
        assert torch.equal(again[k], r[k]), k


def _raw_solve(c, order, nsteps, rec_every, rabs, f32, rpsi, fin, scratch="auto", B_=B, shape=None, batched=1,
               dx=None, dy=None, dz=None, psi0=None):
    """blindno_gpe3d_solve through the raw binding, on caller-made buffers."""
    from blindno._lib import call, ptr, query, stream_ptr
    nx, ny, nz = shape or c["V"].shape[1:]
    dev = "cuda"
    p0 = torch.from_numpy(np.array(c["psi0"]).view(np.float64)).to(dev) if psi0 is None else psi0
    Vd = torch.from_numpy(np.array(c["V"])).to(dev)
    gd, kd = torch.from_numpy(G).to(dev), torch.from_numpy(KAPPA).to(dev)
    if isinstance(scratch, str):
        scratch = torch.empty(query("blindno_gpe3d_scratch_doubles", B, *c["V"].shape[1:]), dtype=torch.float64, device=dev)
    d = [float(a[1] - a[0]) for a in (c["x"], c["y"], c["z"])]
    d = [v if o is None else o for v, o in zip(d, (dx, dy, dz))]
    return call("blindno_gpe3d_solve", ptr(p0), ptr(Vd), ptr(gd), ptr(kd), *d, DT, nsteps, order, rec_every, ptr(rabs),
                f32, ptr(rpsi), ptr(fin), ptr(scratch), B_, nx, ny, nz, batched, stream_ptr())


@pytest.mark.parametrize("shape", [(4, 8, 16), (16, 16, 16)], ids=lambda s: "x".join(map(str, s)))
def test_outputs_fully_written_margins_untouched(shape):
    """Outputs NaN-prefilled between sentinel margins: every element written, no margin touched;
    the fp32 |psi| record is the fp64 one rounded; each output works on its own."""
    c = _case(shape, 2)
    cells = int(np.prod(shape))
    re_ = 3
    nrec = NS // re_ + 1
    M = 64                                                     # margin, elements (16-byte aligned)

    def guarded(n, dtype=torch.float64):
        t = torch.full((n + 2 * M,), -777.0, dtype=dtype, device="cuda")
        t[M:M + n] = float("nan")
        return t

    def check(t, n):
        assert bool((t[:M] == -777.0).all()) and bool((t[M + n:] == -777.0).all()), "margin overwritten"
        assert not bool(torch.isnan(t[M:M + n]).any()), "output not fully written"
        return t[M:M + n]

    n_abs, n_psi, n_fin = B * nrec * cells, 2 * B * nrec * cells, 2 * B * cells
    a64, a32, ps, fi = guarded(n_abs), guarded(n_abs, torch.float32), guarded(n_psi), guarded(n_fin)
    _raw_solve(c, 2, NS, re_, a64[M:], 0, ps[M:], fi[M:])
    abs64, psi, fin = check(a64, n_abs), check(ps, n_psi), check(fi, n_fin)
    want = np.ascontiguousarray(c["psi"][:, 0:NS + 1:re_]).view(np.float64).reshape(-1)
    assert rel_l2(psi.cpu().numpy(), want) <= 1e-10
    pc = torch.view_as_complex(psi.view(B, nrec, *shape, 2))
    assert rel_l2(abs64.view(B, nrec, *shape).cpu().numpy(), pc.abs().cpu().numpy()) <= 1e-14
    # the step-7 field is not a recorded step (7 % 3 != 0): final comes from its own store
    assert rel_l2(torch.view_as_complex(fin.view(B, *shape, 2)).cpu().numpy(), c["psi"][:, NS]) <= 1e-10
    # fp32 record alone (no psi, no final)
    _raw_solve(c, 2, NS, re_, a32[M:], 1, None, None)
    assert torch.equal(check(a32, n_abs), abs64.to(torch.float32))
    # psi alone / final alone / nothing but the scratch field
    ps2, fi2 = guarded(n_psi), guarded(n_fin)
    _raw_solve(c, 2, NS, re_, None, 0, ps2[M:], None)
    assert torch.equal(check(ps2, n_psi), psi)
    _raw_solve(c, 2, NS, re_, None, 0, None, fi2[M:])
    assert torch.equal(check(fi2, n_fin), fin)
    _raw_solve(c, 2, NS, re_, None, 0, None, None)
    # order 4 writes the same set of elements
    ps4, fi4 = guarded(n_psi), guarded(n_fin)
    _raw_solve(c, 4, NS, re_, None, 0, ps4[M:], fi4[M:])
    check(ps4, n_psi), check(fi4, n_fin)
    # no steps at all: the record is psi0 and so is the final field
    ps3, fi3 = guarded(2 * B * cells), guarded(n_fin)
    _raw_solve(c, 2, 0, 1, None, 0, ps3[M:], fi3[M:])
    p0 = torch.from_numpy(np.array(c["psi0"]).view(np.float64)).cuda().reshape(-1)
    assert torch.equal(check(ps3, 2 * B * cells), p0) and torch.equal(check(fi3, n_fin), p0)


def test_refusals_leave_the_stream_usable():
    """Every refusal of the C entry (hipErrorInvalidValue before any launch) and of the Python
    guards raises BlindnoError; a valid solve on the same stream then still gives the right
    answer."""
    from blindno import gpe
    from blindno._lib import BlindnoError, call, ptr, stream_ptr
    shape = (4, 8, 16)
    c = _case(shape, 2)
    cells = 4 * 8 * 16
    rabs = torch.empty(B * 3 * cells, dtype=torch.float64, device="cuda")
    fin = torch.empty(2 * B * cells, dtype=torch.float64, device="cuda")
    ok = dict(order=2, nsteps=2, rec_every=1)
    bad = [dict(shape=(12, 8, 16)), dict(shape=(4, 12, 16)), dict(shape=(4, 8, 24)),          # not a power of two
           dict(shape=(2, 8, 16)), dict(shape=(4, 2, 16)), dict(shape=(4, 8, 2)), dict(shape=(4, 8, 0)),   # below 4
           dict(shape=(2 * MAX_N, 8, 16)), dict(shape=(4, 2 * MAX_N, 16)), dict(shape=(4, 8, 2 * MAX_N)),  # above MAX_N
           dict(shape=(512, 256, 256)), dict(shape=(MAX_N, MAX_N, 32)),                      # the cell cap
           dict(order=3), dict(order=1), dict(rec_every=0), dict(rec_every=-2), dict(nsteps=-1),
           dict(dx=0.0), dict(dy=-1.0), dict(dz=0.0), dict(dz=float("nan")),
           dict(scratch=None), dict(B_=0), dict(f32=2), dict(psi0=fin[1:])]
    for kw in bad:
        a = dict(ok, f32=0)
        a.update(kw)
        with pytest.raises(BlindnoError, match="blindno_gpe3d_solve failed"):
            _raw_solve(c, a.pop("order"), a.pop("nsteps"), a.pop("rec_every"), rabs, a.pop("f32"), None, fin, **a)
    with pytest.raises(BlindnoError, match="blindno_gpe3d_solve failed"):                   # misaligned output
        _raw_solve(c, 2, 2, 1, rabs, 0, None, fin[1:])
    with pytest.raises(BlindnoError, match="blindno_trapz3_frames failed"):
        call("blindno_trapz3_frames", ptr(rabs), ptr(rabs), ptr(rabs), ptr(rabs), ptr(rabs), ptr(fin), 0, 4, 8, 16,
             stream_ptr())
    args = (c["psi0"], c["x"], c["y"], c["z"])
    for kw, pat in [(dict(dt=1.0, t_final=gpe.MAX_LAUNCHES_3D // 3 + 1.5, rec_every=1 << 30), "MAX_LAUNCHES_3D"),
                    (dict(dt=0.005, t_final=5.0, order=3), "order"),
                    (dict(dt=0.005, t_final=5.0, rec_every=0), "rec_every")]:
        a = dict(order=2, rec_every=1)
        a.update(kw)
        with pytest.raises(BlindnoError, match=pat):
            gpe.solve_batch_3d(*args, a["dt"], a["t_final"], a["order"], G, KAPPA, c["V"], rec_every=a["rec_every"])
    big = np.broadcast_to(c["V"][:1, :1, :1, :1], (64, 64, 64, 64))
    xb = np.linspace(-10, 10, 64)
    with pytest.raises(BlindnoError, match="MAX_RECORD_BYTES"):
        gpe.solve_batch_3d(np.ones((64, 64, 64), complex), xb, xb, xb, 0.005, 5.0, 2, 2, 2, big)
    with pytest.raises(BlindnoError, match="power of two"):
        gpe.solve_batch_3d(np.ones((12, 8, 16), complex), np.linspace(0, 1, 12), c["y"], c["z"], 0.005, 0.1, 2, 1, 1,
                           np.zeros((12, 8, 16)))
    torch.cuda.synchronize()
    r = gpe.solve_batch_3d(*args, DT, TF, 2, G, KAPPA, c["V"], want_psi=True)
    assert rel_l2(r["psi"].cpu().numpy(), c["psi"]) <= 1e-10


@pytest.mark.parametrize("dims", [(5, 6, 9, 7), (2, 16, 20, 24)], ids=["5x6x9x7", "2x16x20x24"])
def test_time_averaged_L2_error_3d(dims):
    """Against numpy.trapz applied three times: a frame smaller than one sweep of the workgroup
    (378 points) and one of many sweeps (7680 points); any grid, the integral is not an FFT."""
    from blindno import gpe
    nt, nx, ny, nz = dims
    rs = np.random.RandomState(4)
    x = np.sort(rs.uniform(-3, 3, nx))                           # non-uniform spacings as numpy.trapz takes them
    y = np.linspace(-2, 5, ny)
    z = np.cumsum(rs.uniform(0.1, 0.4, nz))
    t = np.sort(rs.uniform(0, 2, nt))
    ref, pred = rs.rand(*dims) + 0.1, rs.rand(*dims) + 0.1
    want = gpe3d_ref.time_averaged_L2_error(t, ref, pred, x, y, z)
    v = gpe.time_averaged_L2_error_3d(t, ref, t, pred, (x, y, z))
    v2 = gpe.time_averaged_L2_error_3d(t, torch.from_numpy(ref).cuda(), t, torch.from_numpy(pred).cuda(), [x, y, z])
    print(f"3D density error {dims}: {v!r} vs numpy {want!r}")
    assert abs(v - want) <= 1e-12 * abs(want) and v2 == v
    with pytest.raises(ValueError):
        gpe.time_averaged_L2_error_3d(t, ref, t, pred[:, :, :-1], (x, y, z))
    with pytest.raises(ValueError):
        gpe.time_averaged_L2_error_3d(t, ref, t, pred, (x, y))
    with pytest.raises(ValueError):
        gpe.time_averaged_L2_error_3d(t, ref, t + 0.5, pred, (x, y, z))


@pytest.fixture(scope="module")
def generated():
    from blindno import gpe
    d32 = gpe.generate_training_data_3d(3, 16, 16, 16, t_final=0.1, rng=np.random.RandomState(11))
    d64 = gpe.generate_training_data_3d(3, 16, 16, 16, t_final=0.1, rng=np.random.RandomState(11), y_dtype=np.float64,
                                        batch=2)
    return d32, d64


def test_generator_matches_reference(generated):
    from blindno import gpe
    d32, d64 = generated
    ref = gpe3d_ref.generate(3, 16, 16, 16, t_final=0.1, rng=np.random.RandomState(11))
    assert sorted(d64) == sorted(d32) == sorted(ref) == ["V", "g", "kappa", "y"]
    assert d64["y"].shape == ref["y"].shape == (3, 3, 16, 16, 16) and d64["y"].dtype == np.float64
    assert d64["V"].shape == (3, 16, 16, 16) and d64["g"].shape == d64["kappa"].shape == (3,)
    x = np.linspace(-10, 10, 16)
    assert np.array_equal(d64["V"], gpe.training_potentials_3d(3, x, x, x, np.random.RandomState(11)))
    assert np.allclose(d64["V"], ref["V"], rtol=1e-14, atol=0) and np.array_equal(d64["g"], ref["g"])
    assert np.array_equal(d64["kappa"], ref["kappa"]) and set(d64["g"]) == {2}
    e = rel_l2(d64["y"], ref["y"])
    print(f"generator vs reference: {e:.3e}")
    assert e <= 1e-10
    assert d32["y"].dtype == np.float32 and np.array_equal(d32["y"], d64["y"].astype(np.float32))
    assert np.array_equal(d32["V"], d64["V"])


def _grid3(n):
    ax = [torch.linspace(-1, 1, m) for m in n]
    return torch.stack(torch.meshgrid(*ax, indexing="ij"), -1).contiguous()


def test_generated_set_feeds_the_3d_model(generated, tmp_path):
    """save_training_data -> ParameterDataset -> one eager NIOFP3D_FNO train step (forward, MSE,
    backward) against the fp64 checker tests/nio3d_fno_ref.py at that suite's bars."""
    import blindno
    import nio3d_fno_ref
    from blindno import data, gpe
    d32, _ = generated
    path = str(tmp_path / "gpe3d.npy")
    gpe.save_training_data(d32, path)
    ds = data.ParameterDataset(path)
    assert len(ds) == 3 and ds[0][0].shape == (3, 16, 16, 16) and ds[0][1].shape == (16, 16, 16, 1)
    X, Y = data.device_tensors(ds, [0, 2], device="cuda")
    assert X.shape == (2, 3, 16, 16, 16) and Y.shape == (2, 16, 16, 16, 1) and X.dtype == torch.float32
    torch.manual_seed(3)
    m = blindno.NIOFP3D_FNO(2, 8, 4, 1, "cuda", input_modes=4).cuda().train()
    grid = _grid3((16, 16, 16)).cuda()
    idx = np.array([2, 0, 2, 1, 1, 2, 0])                      # a bag with repeats
    out = m(X, grid, bag_idx=idx)
    loss = blindno.mse_loss(out, Y)
    loss.backward()
    torch.cuda.synchronize()
    loss = loss.detach()
    p = nio3d_fno_ref.leaves({k: v.detach().cpu().numpy() for k, v in m.state_dict().items()})
    ref = nio3d_fno_ref.niofp3d_fno(p, X.cpu().double(), grid.cpu().double(), idx=idx.tolist())
    ref_loss = ((ref - Y.cpu().double()) ** 2).mean()
    ref_loss.backward()
    ref_loss = ref_loss.detach()
    e = rel_l2(out.detach().cpu().numpy(), ref.detach().numpy())
    worst = (0.0, "")
    for k, prm in m.named_parameters():
        if k.startswith("fc0."):
            assert prm.grad is None, k
            continue
        got, want = prm.grad, p[k].grad
        if got.is_complex():
            got, want = torch.view_as_real(got), torch.view_as_real(want)
        worst = max(worst, (rel_l2(got.cpu().numpy(), want.numpy()), k))
    print(f"fwd {e:.2e}, loss {float(loss):.6e} vs {float(ref_loss):.6e}, worst gradient {worst[0]:.2e} ({worst[1]})")
    assert e <= 1e-5 and worst[0] <= 1e-4
    assert abs(float(loss) - float(ref_loss)) <= 1e-5 * float(ref_loss)


def test_compute_time_error_gpe_3d_pipeline(tmp_path, monkeypatch):
    """One batched pipeline against its steps run one trajectory at a time, and against itself
    with a record limit that forces one solve_batch_3d call per trajectory."""
    from blindno import NIOFP3D_FNO, evaluate, gpe, timeerror
    rs = np.random.RandomState(9)
    T, N = 5, 16
    mk = lambda m: dict(y=rs.rand(m, T, N, N, N), V=rs.rand(m, N, N, N) * 3, g=rs.rand(m), kappa=rs.rand(m) * 0.1)  # noqa: E731
    train, test = mk(4), mk(3)
    models = {}
    for name, seed in (("fno", 1), ("fno_b", 2)):
        torch.manual_seed(seed)
        models[name] = NIOFP3D_FNO(2, 8, 4, 1, "cuda", input_modes=4).cuda()
    kw = dict(t_final=0.1, dt=0.005, rec_every=5)
    errs = timeerror.compute_time_error_gpe_3d(models, train, test, [2, 0, 7], outdir=str(tmp_path), **kw)
    assert list(errs) == ["fno", "fno_b"] and errs["fno"].shape == (2,)
    sc = evaluate.compute_train_scalers_gpe(train)
    tn = evaluate.normalize_gpe(test, sc)
    x = np.linspace(-10, 10, N)
    psi0 = gpe3d_ref.initial_field(x, x, x)
    i = 2
    pv = evaluate.predict(models["fno_b"], torch.tensor(tn["y"][i][None], dtype=torch.float32, device="cuda"),
                          timeerror.grid3d(N, N, N, "cuda")).cpu().numpy()[0, ..., 0] * sc["V_max"]
    one = lambda V: gpe.solve_batch_3d(psi0, x, x, x, kw["dt"], kw["t_final"], 2, test["g"][i], test["kappa"][i], V,  # noqa: E731
                                       rec_every=5)
    a, b = one(tn["V"][i] * sc["V_max"]), one(pv)
    assert a["abs"].shape == (1, 5, N, N, N)
    e = gpe.time_averaged_L2_error_3d(a["t"], a["abs"][0], b["t"], b["abs"][0], (x, x, x))
    assert np.isfinite(e) and e > 0
    # the solver and the integrals are independent of the batch bit for bit; the fp32 model forward
    # may order its sums differently for one sample than for two: the 2D pipeline test's bar
    print(f"pipeline {errs['fno_b'][0]!r} vs one at a time {e!r}")
    assert abs(errs["fno_b"][0] - e) <= 1e-6 * e + 1e-15
    d = np.load(tmp_path / "fno" / "sample_0_V_and_err.npy", allow_pickle=True).item()
    assert d["Err_L2_rel"] == errs["fno"][1] and d["pred_V"].shape == (N, N, N) and sorted(d)[-3:] == ["x", "y", "z"]
    assert np.load(tmp_path / "ErrL2_relative_fno_Nsamples_2.npy").shape == (2,)
    # chunked: a limit of one trajectory's record (5 frames x 16^3 x 8 B) -> six calls, same digits
    calls = []
    real = gpe.solve_batch_3d
    monkeypatch.setattr(gpe, "solve_batch_3d", lambda *a_, **k_: (calls.append(np.shape(a_[9])[0]), real(*a_, **k_))[1])
    monkeypatch.setattr(gpe, "MAX_RECORD_BYTES", 5 * N ** 3 * 8)
    errs1 = timeerror.compute_time_error_gpe_3d(models, train, test, [2, 0, 7], **kw)
    assert calls == [1] * 6
    calls.clear()
    monkeypatch.setattr(gpe, "MAX_RECORD_BYTES", 4 * 5 * N ** 3 * 8)                          # 4 fit: one index (3) per call
    errs3 = timeerror.compute_time_error_gpe_3d(models, train, test, [2, 0, 7], **kw)
    assert calls == [3, 3]
    for name in errs:
        assert np.array_equal(errs1[name], errs[name]) and np.array_equal(errs3[name], errs[name])
