"""Float64 numpy restatement of the 3D Gross-Pitaevskii split-step integrator (TEST
INFRASTRUCTURE for tests/test_gpe3d.py and tests/test_gpu_gpe3d.py).

  i psi_t = -1/2 (psi_xx + psi_yy + psi_zz) + (V + g|psi|^2 + kappa|psi|^4) psi,  periodic grid

tests/gpe2d_ref.py with one more axis: N(h) multiplies by exp(-i h (V + g|psi|^2 + kappa|psi|^4)),
L(h) is ifftn(exp(-i h/2 (kx^2 + ky^2 + kz^2)) fftn psi) with numpy.fft.fftn -- one 3D transform
and one phase, NOT the per-axis factorisation the HIP kernels use, so agreement is an independent
check.  Orders 2 and 4 are gpe2d_ref.stages.  With inputs independent of one axis it equals
gpe2d_ref on every slice (tests/test_gpe3d.py), which ties it to the reference's 1D goldens
through the existing chain.  ``training_potentials`` restates the draws of
blindno.gpe.generate_training_data_3d.
"""
from __future__ import annotations

import numpy as np

import gpe2d_ref
from oracle import gpe_ref

nonlinear = gpe2d_ref.nonlinear
stages = gpe2d_ref.stages


def linear(psi, h, kx, ky, kz):
    ph = np.exp(-1j * h * 0.5 * (kx[:, None, None] ** 2 + ky[None, :, None] ** 2 + kz[None, None, :] ** 2))
    return np.fft.ifftn(ph * np.fft.fftn(psi))


def solve(psi0, x, y, z, dt, t_final, order, g, kappa, V, rec_every=1):
    """(t, psi record (nrec, nx, ny, nz) complex128, final field): every rec_every-th step, step 0
    included, as blindno.gpe.solve_batch_3d records them."""
    ks = [gpe_ref.wavenumbers(len(a), a[1] - a[0]) for a in (np.asarray(v, dtype=np.float64) for v in (x, y, z))]
    nt = int(t_final / dt) + 1
    t = np.linspace(0, t_final, nt)
    st = stages(order)
    psi = np.array(psi0, dtype=np.complex128)
    rec = [psi.copy()]
    for i in range(1, nt):
        for kind, c in st:
            psi = nonlinear(psi, c * dt, V, g, kappa) if kind == "n" else linear(psi, c * dt, *ks)
        if i % rec_every == 0:
            rec.append(psi.copy())
    return t[::rec_every][:len(rec)], np.stack(rec, 0), psi


def training_potentials(num_orbits, x, y, z, rng=np.random):
    """Per orbit, in this order: a ~ U(0.1, 0.3), b ~ U(0.5, 2), c ~ U(0.5, 2), x0, y0, z0 ~ U(-3, 3);
    V = a((x-x0)^2 + (y-y0)^2 + (z-z0)^2) + b cos^2(c(x-x0)) cos^2(c(y-y0)) cos^2(c(z-z0))."""
    Vs = []
    for _ in range(num_orbits):
        a = rng.uniform(0.1, 0.3)
        b = rng.uniform(0.5, 2)
        c = rng.uniform(0.5, 2)
        x0 = rng.uniform(-3, 3)
        y0 = rng.uniform(-3, 3)
        z0 = rng.uniform(-3, 3)
        V = np.empty((len(x), len(y), len(z)))
        for i, xv in enumerate(x):
            for j, yv in enumerate(y):
                V[i, j] = a * ((xv - x0) ** 2 + (yv - y0) ** 2 + (z - z0) ** 2) + \
                    b * np.cos(c * (xv - x0)) ** 2 * np.cos(c * (yv - y0)) ** 2 * np.cos(c * (z - z0)) ** 2
        Vs.append(V)
    return np.stack(Vs, 0)


def initial_field(x, y, z, ic=2):
    f = gpe_ref.initial_condition
    return f(ic, x)[:, None, None] * f(ic, y)[None, :, None] * f(ic, z)[None, None, :]


def generate(num_orbits, Nx, Ny, Nz, dt=0.005, t_final=5.0, order=2, rng=np.random):
    """The generator's dict in fp64: y = |psi|[::10] under psi0 = ic2(x) ic2(y) ic2(z), g = kappa = 2."""
    x, y, z = (np.linspace(-10, 10, n) for n in (Nx, Ny, Nz))
    V = training_potentials(num_orbits, x, y, z, rng)
    psi0 = initial_field(x, y, z)
    ys = [np.abs(solve(psi0, x, y, z, dt, t_final, order, 2.0, 2.0, V[m], rec_every=10)[1]) for m in range(num_orbits)]
    return {"y": np.stack(ys, 0), "g": np.full(num_orbits, 2), "kappa": np.full(num_orbits, 2), "V": V}


def time_averaged_L2_error(t, rho_ref, rho_pred, x, y, z, eps=1e-12):
    """numpy.trapz applied three times per frame, then the trapezoid time average."""
    trapz = getattr(np, "trapezoid", None) or np.trapz
    i3 = lambda f: trapz(trapz(trapz(f, x, axis=1), y, axis=1), z, axis=1)   # noqa: E731
    rel = np.sqrt(i3((rho_pred - rho_ref) ** 2)) / (np.sqrt(i3(rho_ref ** 2)) + eps)
    return float(trapz(rel, t) / (t[-1] - t[0]))
