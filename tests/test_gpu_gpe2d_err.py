"""The record-free 2D GPE density error (blindno_gpe2d_error, csrc/gpe_nd.hip; needs a GPU):
gpe.solve_error_batch_2d against the recorded path (solve_batch_2d + blindno_trapz2_frames, both
unchanged code) and against the numpy checker tests/gpe2d_ref.py, and the record_free path of
timeerror.compute_time_error_gpe_2d.

The cases are test_gpu_gpe2d._case's construction with B = 6 trajectories in groups of 3: their own
V, g, kappa and psi0 (a phase ramp per trajectory), grids linspace(-10, 10, nx) and
linspace(-8, 8, ny), NS = 7 steps of DT = 0.005.  The pass kernel is the solver's, launched by the
same sequence, so the shapes are the small ones at which the two new kernels take another path: N
below one run of 256 cells, below one tile of 1024 in both axis orders, exactly one tile, several
tiles; and one 1024 x 512 case whose 512 tiles make stage two's strided loop run twice.

U = 2^-53.  The bar against the recorded path is SUM(N) = 2.5 N U relative per entry (derived in
tests/test_gpu_gpe3d_err.py): both sides add the same N non-negative terms (the same bits: w = wx wy,
d = a - b, w (d d), w (b b)) in another order, each side is within gamma_(N-1) = (N - 1) U /
(1 - (N - 1) U) of the exact sum (Higham, Accuracy and Stability of Numerical Algorithms, 4.2), and
twice that is below 2.5 N U for N <= 2^24.
"""
import functools

import numpy as np
import pytest
import torch

import gpe2d_ref
from oracle import gpe_ref

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    import blindno
    blindno.load_library()


U = 2.0 ** -53
SHAPES = [(4, 4), (16, 8), (8, 64), (32, 32), (64, 32), (32, 128)]
IDS = lambda s: "x".join(map(str, s))                             # noqa: E731
B, GROUP = 6, 3
G = np.array([2.0, 0.5, 0.0, 1.0, 1.5, 0.25])                     # trajectory 2 is linear
KAPPA = np.array([2.0, 1.0, 0.0, 0.5, 0.0, 1.25])
NS, DT = 7, 0.005
TF = DT * (NS + 0.5)


def SUM(n):
    return 2.5 * n * U


@functools.lru_cache(maxsize=None)
def _case(shape, nb=B):
    """Inputs of one shape: nb trajectories with their own V and psi0.  Computed once, shared by the
    tests below, never modified."""
    nx, ny = shape
    rs = np.random.RandomState(nx * 7 + ny)
    x = np.linspace(-10, 10, nx)
    y = np.linspace(-8, 8, ny)                                    # dx != dy
    V = gpe2d_ref.training_potentials(nb, x, y, rs)
    f = gpe_ref.initial_condition
    base = f(2, x)[:, None] * f(3, y)[None, :]
    ph = 0.3 * x[:, None] + 0.2 * y[None, :]
    psi0 = np.stack([base * np.exp(1j * (b + 1) * ph) + 0.05 * b for b in range(nb)])
    for a in (x, y, V, psi0):
        a.setflags(write=False)
    return dict(x=x, y=y, V=V, psi0=psi0, N=nx * ny)


def _args(c, order, sl=slice(None)):
    return (c["x"], c["y"], DT, TF, order, G[sl], KAPPA[sl], c["V"][sl])


def _trapz2_frames(a, ref, c):
    """blindno_trapz2_frames of the frames a against ref (both (F, nx, ny) device tensors) -> (F, 2)."""
    from blindno._lib import call, ptr, stream_ptr
    a, ref = a.contiguous(), ref.contiguous()
    d = lambda v: torch.from_numpy(np.array(v)).cuda()            # noqa: E731
    out = torch.empty(a.shape[0], 2, dtype=torch.float64, device="cuda")
    call("blindno_trapz2_frames", ptr(a), ptr(ref), ptr(d(c["x"])), ptr(d(c["y"])), ptr(out), a.shape[0],
         *a.shape[1:], stream_ptr())
    return out


def _reduce_record(ab, group, c):
    """A (B, nrec, nx, ny) |psi| record, each trajectory against its group's first -> num, den as numpy."""
    nb, nrec = ab.shape[:2]
    ref = ab[torch.arange(nb, device="cuda") // group * group]
    s = _trapz2_frames(ab.reshape(nb * nrec, *ab.shape[2:]), ref.reshape(nb * nrec, *ab.shape[2:]), c)
    s = s.view(nb, nrec, 2).cpu().numpy()
    return s[..., 0], s[..., 1]


def _recorded(c, psi0, order, rec_every, group=GROUP, sl=slice(None)):
    """The recorded path: solve_batch_2d's fp64 |psi| record through blindno_trapz2_frames ->
    t, num (B, nrec), den (B, nrec) as numpy."""
    from blindno import gpe
    r = gpe.solve_batch_2d(psi0, *_args(c, order, sl), rec_every=rec_every)
    return (r["t"],) + _reduce_record(r["abs"], group, c)


def _streamed(c, psi0, order, rec_every, group=GROUP, sl=slice(None)):
    from blindno import gpe
    r = gpe.solve_error_batch_2d(psi0, *_args(c, order, sl), group=group, rec_every=rec_every)
    assert r["num"].dtype == r["den"].dtype == torch.float64 and r["num"].is_cuda
    return r["t"], r["num"].cpu().numpy(), r["den"].cpu().numpy()


def _close(a, b, tol):
    return bool(np.all(np.abs(a - b) <= tol * np.abs(b)))


@pytest.mark.parametrize("order", [2, 4])
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_matches_the_recorded_path(shape, order):
    """Batched and shared psi0, every step and every 3rd: every entry within SUM(N) of the recorded
    path's; references have num exactly 0; den is the reference's across a group, bit for bit."""
    c = _case(shape)
    for psi0, what in ((c["psi0"], "batched"), (c["psi0"][1], "shared")):
        for rec_every in (1, 3):
            t, num, den = _streamed(c, psi0, order, rec_every)
            tr, numr, denr = _recorded(c, psi0, order, rec_every)
            assert num.shape == den.shape == numr.shape == (B, NS // rec_every + 1)
            assert np.array_equal(t, tr)
            ok = denr > 0
            e_num = np.abs(num - numr)[numr > 0] / numr[numr > 0]
            e_den = np.abs(den - denr)[ok] / denr[ok]
            print(f"{shape} order {order} {what} psi0 rec {rec_every}: num {e_num.max() / U:.1f} U, "
                  f"den {e_den.max() / U:.1f} U (bar {SUM(c['N']) / U:.0f} U)")
            assert _close(num, numr, SUM(c["N"])) and _close(den, denr, SUM(c["N"]))
            assert np.all(num[::GROUP] == 0.0) and np.all(numr[::GROUP] == 0.0)
            # after a step every trajectory differs from its reference (its own V, g, kappa)
            assert np.all(num[np.arange(B) % GROUP != 0][:, 1:] > 0) and np.all(den > 0)
            for b in range(B):
                assert np.array_equal(den[b], den[b // GROUP * GROUP]), b


def test_more_tiles_than_stage_two_has_threads():
    """1024 x 512 is 512 tiles per trajectory: each of stage two's 256 threads adds two partials.
    B = 2 in one group, 2 Strang steps, every step reduced; against the recorded path only."""
    from blindno import gpe
    shape, nb = (1024, 512), 2
    c = _case(shape, nb)
    a = (c["psi0"], c["x"], c["y"], DT, DT * 2.5, 2, G[:nb], KAPPA[:nb], c["V"])
    r = gpe.solve_error_batch_2d(*a, group=nb, rec_every=1)
    rec = gpe.solve_batch_2d(*a, rec_every=1)
    num, den = r["num"].cpu().numpy(), r["den"].cpu().numpy()
    numr, denr = _reduce_record(rec["abs"], nb, c)
    assert num.shape == den.shape == numr.shape == (nb, 3) and np.array_equal(r["t"], rec["t"])
    print(f"{shape}: num {np.abs(num - numr)[1].max() / numr[1].max() / U:.1f} U, "
          f"den {(np.abs(den - denr) / denr).max() / U:.1f} U (bar {SUM(c['N']) / U:.0f} U)")
    assert _close(num, numr, SUM(c["N"])) and _close(den, denr, SUM(c["N"]))
    assert np.all(num[0] == 0.0) and np.all(num[1] > 0) and np.all(den > 0) and np.array_equal(den[0], den[1])


@functools.lru_cache(maxsize=None)
def _checker(shape, order):
    """num, den (B, NS + 1) from gpe2d_ref.solve records and numpy.trapz applied twice."""
    c = _case(shape)
    x, y = c["x"], c["y"]
    ab = np.stack([np.abs(gpe2d_ref.solve(c["psi0"][b], x, y, DT, TF, order, G[b], KAPPA[b], c["V"][b])[1])
                   for b in range(B)])
    trapz = getattr(np, "trapezoid", None) or np.trapz
    i2 = lambda f: trapz(trapz(f, x, axis=-2), y, axis=-1)        # noqa: E731
    ref = ab[np.arange(B) // GROUP * GROUP]
    return i2((ab - ref) ** 2), i2(ref ** 2)


@pytest.mark.parametrize("order", [2, 4])
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_matches_the_numpy_checker(shape, order):
    """The bar is not a fixed number: the recorded path (the parent's code) is measured against the
    checker on the same case first, per entry, as |sqrt(num) - sqrt(num_c)| / (sqrt(den) + sqrt(den_c))
    and the same with den in the numerator; the streaming path is allowed that distance plus SUM(N)."""
    c = _case(shape)
    numc, denc = _checker(shape, order)

    def dist(num, den):
        dn = np.sqrt(den) + np.sqrt(denc)
        return np.abs(np.sqrt(num) - np.sqrt(numc)) / dn, np.abs(np.sqrt(den) - np.sqrt(denc)) / dn

    _, numr, denr = _recorded(c, c["psi0"], order, 1)
    _, num, den = _streamed(c, c["psi0"], order, 1)
    (rn, rd), (sn, sd) = dist(numr, denr), dist(num, den)
    print(f"{shape} order {order}: recorded path vs checker num {rn.max():.3e} den {rd.max():.3e}; "
          f"streaming path num {sn.max():.3e} den {sd.max():.3e}; allowance {SUM(c['N']):.3e}")
    assert np.all(sn <= rn + SUM(c["N"])) and np.all(sd <= rd + SUM(c["N"]))


def test_determinism_and_batch_independence():
    from blindno import gpe
    c = _case((64, 32))
    a = (c["psi0"],) + _args(c, 2)
    r = gpe.solve_error_batch_2d(*a, group=GROUP, rec_every=3)
    again = gpe.solve_error_batch_2d(*a, group=GROUP, rec_every=3)
    assert torch.equal(again["num"], r["num"]) and torch.equal(again["den"], r["den"])
    sl = slice(GROUP, 2 * GROUP)
    alone = gpe.solve_error_batch_2d(c["psi0"][sl], *_args(c, 2, sl), group=GROUP, rec_every=3)
    assert alone["num"].shape == (GROUP, NS // 3 + 1)
    assert torch.equal(alone["num"], r["num"][sl]) and torch.equal(alone["den"], r["den"][sl])
    one = gpe.solve_error_batch_2d(*a, group=1, rec_every=3)
    assert bool((one["num"] == 0.0).all()) and bool((one["den"] > 0).all())
    assert torch.equal(one["den"][::GROUP], r["den"][::GROUP])     # a reference's den is its own |psi|^2
    whole = gpe.solve_error_batch_2d(*a, rec_every=3)              # group defaults to the batch
    explicit = gpe.solve_error_batch_2d(*a, group=B, rec_every=3)
    assert torch.equal(whole["num"], explicit["num"]) and torch.equal(whole["den"], explicit["den"])
    t, numr, denr = _recorded(c, c["psi0"], 2, 3, group=B)
    assert np.array_equal(whole["t"], t)
    assert _close(whole["num"].cpu().numpy(), numr, SUM(c["N"])) and _close(whole["den"].cpu().numpy(), denr, SUM(c["N"]))
    assert torch.equal(whole["den"], whole["den"][:1].expand(B, -1)) and torch.equal(whole["num"][:GROUP], r["num"][:GROUP])


@pytest.mark.parametrize("shape", [(4, 4), (64, 32)], ids=IDS)
def test_no_steps(shape):
    """t_final below dt: one frame, the sums of |psi0|, for both orders.  num against the kernel's own
    recorded frame (the same bits per term) at SUM(N).  den against numpy.trapz of numpy's |psi0|^2 at
    SUM(N) + 16 U: the 16 U is the 3D test's allowance kept as it is -- there a term w (b b) carries at
    most 8 roundings on either side with three weight factors; with two factors it carries fewer (two
    in w's factors, one in their product, hypot's, the square, the product), so 16 U holds a fortiori."""
    from blindno import gpe
    c = _case(shape)
    for order in (2, 4):
        r = gpe.solve_error_batch_2d(c["psi0"], c["x"], c["y"], DT, DT / 2, order, G, KAPPA, c["V"], group=GROUP)
        assert r["num"].shape == r["den"].shape == (B, 1) and np.array_equal(r["t"], [0.0])
        num, den = r["num"].cpu().numpy(), r["den"].cpu().numpy()
        trapz = getattr(np, "trapezoid", None) or np.trapz
        ref = np.abs(c["psi0"])[np.arange(B) // GROUP * GROUP]
        den_np = trapz(trapz(ref ** 2, c["x"], axis=1), c["y"], axis=1)
        print(f"{shape} order {order}: den vs numpy {(np.abs(den[:, 0] - den_np) / den_np).max() / U:.1f} U "
              f"(bar {(SUM(c['N']) + 16 * U) / U:.0f} U)")
        assert _close(den[:, 0], den_np, SUM(c["N"]) + 16 * U)
        assert np.all(num[::GROUP] == 0.0)
        # numpy's |psi0| and the kernel's hypot may differ in the last bit, which (a - b)^2 amplifies:
        # num is compared where the frame has the kernel's own bits
        rec = gpe.solve_batch_2d(c["psi0"], c["x"], c["y"], DT, DT / 2, order, G, KAPPA, c["V"])["abs"][:, 0]
        wantk = _trapz2_frames(rec, rec[torch.arange(B, device="cuda") // GROUP * GROUP], c).cpu().numpy()
        assert _close(num[:, 0], wantk[:, 0], SUM(c["N"])) and _close(den[:, 0], wantk[:, 1], SUM(c["N"]))
        assert np.all(num[np.arange(B) % GROUP != 0] > 0)


def _raw(c, order, nsteps, rec_every, group, err, scratch, shape=None, B_=B, x="auto", batched=1):
    """blindno_gpe2d_error through the raw binding, on caller-made buffers."""
    from blindno._lib import call, ptr, stream_ptr
    nx, ny = shape or c["V"].shape[1:]
    d = lambda v: torch.from_numpy(np.array(v)).cuda()            # noqa: E731
    p0 = d(np.array(c["psi0"]).view(np.float64))
    xd = d(c["x"]) if isinstance(x, str) else x
    sp = [float(a[1] - a[0]) for a in (c["x"], c["y"])]
    return call("blindno_gpe2d_error", ptr(p0), ptr(d(c["V"])), ptr(d(G)), ptr(d(KAPPA)), ptr(xd), ptr(d(c["y"])),
                *sp, DT, nsteps, order, rec_every, group, ptr(err), ptr(scratch), B_, nx, ny, batched, stream_ptr())


@pytest.mark.parametrize("shape", [(4, 4), (64, 32)], ids=IDS)
def test_outputs_fully_written_margins_untouched(shape):
    """err and scratch between sentinel margins, err NaN-prefilled: every entry written, no margin
    touched, with and without steps, both orders."""
    from blindno._lib import query
    c = _case(shape)
    M = 64                                                        # margin, doubles (16-byte aligned)
    ns = query("blindno_gpe2d_error_scratch_doubles", B, *shape)
    assert ns == 3 * B * c["N"] + 2 * B * max(1, c["N"] // 1024)
    for order, nsteps, rec_every in [(2, NS, 3), (4, NS, 1), (2, 0, 1), (4, 6, 3)]:
        nrec = nsteps // rec_every + 1
        err = torch.full((2 * B * nrec + 2 * M,), -777.0, dtype=torch.float64, device="cuda")
        err[M:M + 2 * B * nrec] = float("nan")
        scratch = torch.full((ns + 2 * M,), -777.0, dtype=torch.float64, device="cuda")
        _raw(c, order, nsteps, rec_every, GROUP, err[M:], scratch[M:])
        torch.cuda.synchronize()
        for t, n in ((err, 2 * B * nrec), (scratch, ns)):
            assert bool((t[:M] == -777.0).all()) and bool((t[M + n:] == -777.0).all()), "margin overwritten"
        got = err[M:M + 2 * B * nrec].view(B, nrec, 2)
        assert not bool(torch.isnan(got).any()), "err not fully written"
        if nsteps == NS:
            _, numr, denr = _recorded(c, c["psi0"], order, rec_every)
            assert _close(got[..., 0].cpu().numpy(), numr, SUM(c["N"])) and _close(got[..., 1].cpu().numpy(), denr, SUM(c["N"]))


def test_memory_is_the_scratch_not_the_record():
    """64^2, B = 6, 200 steps, every step reduced: the record would be 6 x 201 x 4096 x 8 B = 39.5 MB.
    The peak grows by the scratch, the uploaded inputs and the output, and at most 1 MiB of allocator
    rounding (it rounds each of the 8 blocks to 512 B)."""
    from blindno import gpe
    from blindno._lib import query
    n = 64
    c = _case((n, n))
    nsteps = 200
    a = (c["psi0"][1], c["x"], c["y"], DT, DT * (nsteps + 0.5), 2, G, KAPPA, c["V"])
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    r = gpe.solve_error_batch_2d(*a, group=GROUP)
    torch.cuda.synchronize()
    grew = torch.cuda.max_memory_allocated() - before
    N = c["N"]
    scratch = 8 * query("blindno_gpe2d_error_scratch_doubles", B, n, n)
    inputs = 16 * N + 8 * B * N + 2 * 8 * B + 2 * 8 * n            # shared psi0, V, g, kappa, x, y
    out = 8 * 2 * B * (nsteps + 1)
    record = 8 * B * (nsteps + 1) * N
    print(f"peak grew by {grew} B; scratch {scratch} + inputs {inputs} + err {out} = {scratch + inputs + out} B; "
          f"the record would be {record} B")
    assert r["num"].shape == (B, nsteps + 1) and bool(torch.isfinite(r["num"]).all())
    assert grew <= scratch + inputs + out + (1 << 20) < record / 15


def test_refusals_leave_the_stream_usable():
    from blindno import gpe
    from blindno._lib import BlindnoError, query
    shape = (16, 8)
    c = _case(shape)
    err = torch.empty(2 * B * (NS + 1), dtype=torch.float64, device="cuda")
    scratch = torch.empty(query("blindno_gpe2d_error_scratch_doubles", B, *shape), dtype=torch.float64, device="cuda")
    ok = dict(order=2, nsteps=NS, rec_every=1, group=GROUP)
    bad = [dict(group=0), dict(group=-3), dict(group=4), dict(group=5), dict(group=B + 1),     # B % group != 0
           dict(x=None), dict(shape=(12, 8)), dict(shape=(4, 24)), dict(shape=(4, 2)),
           dict(order=1), dict(order=3), dict(rec_every=0), dict(nsteps=-1), dict(B_=0),
           dict(err=None), dict(scratch=None), dict(scratch=scratch[1:])]
    for kw in bad:
        a = dict(ok, err=err, scratch=scratch)
        a.update(kw)
        with pytest.raises(BlindnoError, match="blindno_gpe2d_error failed"):
            _raw(c, a.pop("order"), a.pop("nsteps"), a.pop("rec_every"), a.pop("group"), a.pop("err"), a.pop("scratch"), **a)
    args = (c["psi0"], c["x"], c["y"])
    with pytest.raises(BlindnoError, match="whole groups"):
        gpe.solve_error_batch_2d(*args, DT, TF, 2, G, KAPPA, c["V"], group=4)
    with pytest.raises(BlindnoError, match="order"):
        gpe.solve_error_batch_2d(*args, DT, TF, 3, G, KAPPA, c["V"], group=GROUP)
    with pytest.raises(BlindnoError, match="power of two"):
        gpe.solve_error_batch_2d(np.ones((12, 8), complex), np.linspace(0, 1, 12), c["y"], DT, TF, 2, 1, 1, np.zeros((12, 8)))
    with pytest.raises(BlindnoError, match="MAX_LAUNCHES_2D"):
        gpe.solve_error_batch_2d(*args, 1.0, 600000.5, 2, G, KAPPA, c["V"], group=GROUP)
    torch.cuda.synchronize()
    _, num, den = _streamed(c, c["psi0"], 2, 1)
    _, numr, denr = _recorded(c, c["psi0"], 2, 1)
    assert _close(num, numr, SUM(c["N"])) and _close(den, denr, SUM(c["N"]))


def test_compute_time_error_gpe_2d_record_free(tmp_path, monkeypatch):
    """test_compute_time_error_gpe_2d_pipeline's setup at 32^2.  record_free=True returns the same keys
    and shapes, writes the same files, and its values are within 4 N U of the recorded path's (derived in
    tests/test_gpu_gpe3d_err.py: num and den each move by SUM(N) = 2.5 N U at most, the square roots
    halve that, the ratio adds the two halves, the time average of non-negative terms keeps it, and
    4 N U leaves room for the second-order terms and eps).

    Limits.  The default path's one call records 6 trajectories x 21 frames x 32^2 x 8 B; a limit one
    byte below that makes it raise ("raise rec_every") while a group's scratch (3 trajectories x 3
    doubles per cell and the partials) is far below: the record-free path returns its own earlier
    numbers to the last digit in one call, and again one byte below two groups' scratch (one group per
    call).  Last, a limit one byte below one group's scratch raises with the grid and the limit named."""
    import os
    from blindno import NIOFP2D_FNO, gpe, timeerror
    from blindno._lib import BlindnoError, query
    rs = np.random.RandomState(9)
    T, N = 21, 32
    mk = lambda m: dict(y=rs.rand(m, T, N, N), V=rs.rand(m, N, N) * 3, g=rs.rand(m), kappa=rs.rand(m) * 0.1)  # noqa: E731
    train, test = mk(4), mk(3)
    models = {}
    for name, seed in (("fno", 1), ("fno_b", 2)):
        torch.manual_seed(seed)
        models[name] = NIOFP2D_FNO(2, 3, 100, 25, 2, 6, 5, 1, heads=("fno_V",)).cuda()
    kw = dict(t_final=0.5, dt=0.005, rec_every=5)
    run = lambda **k: timeerror.compute_time_error_gpe_2d(models, train, test, [2, 0, 7], **{**kw, **k})  # noqa: E731
    bar = 4 * N ** 2 * U
    rec = run(outdir=str(tmp_path / "rec"))
    free = run(outdir=str(tmp_path / "free"), record_free=True)
    assert list(free) == list(rec) == ["fno", "fno_b"]
    for name in rec:
        assert free[name].shape == rec[name].shape == (2,) and free[name].dtype == rec[name].dtype
        print(f"{name}: recorded {rec[name]!r} record-free {free[name]!r} (bar {bar:.2e} relative)")
        assert np.all(rec[name] > 0) and _close(free[name], rec[name], bar)
    files = lambda d: sorted(os.path.relpath(os.path.join(r, f), d) for r, _, fs in os.walk(d) for f in fs)  # noqa: E731
    assert files(tmp_path / "free") == files(tmp_path / "rec") and len(files(tmp_path / "rec")) == 6
    a = np.load(tmp_path / "free" / "fno" / "sample_0_V_and_err.npy", allow_pickle=True).item()
    b = np.load(tmp_path / "rec" / "fno" / "sample_0_V_and_err.npy", allow_pickle=True).item()
    assert sorted(a) == sorted(b) and a["Err_L2_rel"] == free["fno"][1] and np.array_equal(a["pred_V"], b["pred_V"])
    assert a["pred_V"].shape == (N, N) and a["pred_V"].dtype == b["pred_V"].dtype
    assert np.array_equal(np.load(tmp_path / "free" / "ErrL2_relative_fno_b_Nsamples_2.npy"), free["fno_b"])
    group = 8 * query("blindno_gpe2d_error_scratch_doubles", 3, N, N)
    record = 6 * 21 * N * N * 8                                   # the default path's single call
    calls = []
    real = gpe.solve_error_batch_2d
    monkeypatch.setattr(gpe, "solve_error_batch_2d", lambda *a_, **k_: (calls.append(np.shape(a_[8])[0]), real(*a_, **k_))[1])
    # one byte below the single call's record, then one byte below two groups' scratch (one group per call)
    for limit, want_calls in ((record - 1, [6]), (2 * group - 1, [3, 3])):
        monkeypatch.setattr(gpe, "MAX_RECORD_BYTES", limit)
        assert group <= limit < record
        with pytest.raises(BlindnoError, match="raise rec_every"):
            run()
        calls.clear()
        small = run(record_free=True)
        assert calls == want_calls
        for name in free:
            assert np.array_equal(small[name], free[name])
    monkeypatch.setattr(gpe, "MAX_RECORD_BYTES", group - 1)
    with pytest.raises(BlindnoError, match=rf"32 x 32.*MAX_RECORD_BYTES = {group - 1}\b"):
        run(record_free=True)
