"""Float64 numpy restatement of the 2D Gross-Pitaevskii split-step integrator (TEST
INFRASTRUCTURE for tests/test_gpe2d.py and tests/test_gpu_gpe2d.py).

  i psi_t = -1/2 (psi_xx + psi_yy) + (V + g|psi|^2 + kappa|psi|^4) psi,  periodic nx x ny grid

The reference's 1D scheme (1d_GPE/datagen_GPE.py:29-115, restated in oracle/gpe_ref.py) with one
more axis: N(h) multiplies by exp(-i h (V + g|psi|^2 + kappa|psi|^4)), L(h) is
ifft2(exp(-i h/2 (kx^2 + ky^2)) fft2 psi) with numpy.fft.fft2 -- one 2D transform and one phase,
NOT the per-axis factorisation the HIP kernels use, so agreement is an independent check.
``linear_separable`` is a second formulation (explicit DFT matrices per axis) the first is
checked against on the CPU.  The reference has no 2D generator: ``training_potentials`` restates
the draws of blindno.gpe.generate_training_data_2d.
"""
from __future__ import annotations

import numpy as np

from oracle import gpe_ref

YOSHIDA_C = gpe_ref.YOSHIDA_C


def nonlinear(psi, h, V, g, kappa):
    a = np.abs(psi)
    return np.exp(-1j * h * (V + g * a * a + kappa * a ** 4)) * psi


def linear(psi, h, kx, ky):
    ph = np.exp(-1j * h * 0.5 * (kx[:, None] ** 2 + ky[None, :] ** 2))
    return np.fft.ifft2(ph * np.fft.fft2(psi))


def linear_separable(psi, h, kx, ky):
    """The same step as two explicit O(n^2) DFTs per axis (oracle.gpe_ref's matrices)."""
    fx, ix = gpe_ref._dft_mats(len(kx))
    fy, iy = gpe_ref._dft_mats(len(ky))
    psi = ix @ (np.exp(-1j * h * 0.5 * kx * kx)[:, None] * (fx @ psi))
    return (iy @ (np.exp(-1j * h * 0.5 * ky * ky)[:, None] * (fy @ psi.T))).T


def stages(order):
    """[(kind, coefficient of dt)] of one step: Strang, or the nine-stage Yoshida sequence."""
    if order == 2:
        return [("n", 0.5), ("l", 1.0), ("n", 0.5)]
    if order == 4:
        a1 = 1.0 / YOSHIDA_C
        a2 = -(2 ** (1 / 3)) / YOSHIDA_C
        return [("n", a1), ("l", a1), ("n", a2), ("l", a2), ("n", a1), ("l", a2), ("n", a2), ("l", a1), ("n", a1)]
    raise ValueError("order must be 2 or 4")


def solve(psi0, x, y, dt, t_final, order, g, kappa, V, rec_every=1, lin=linear):
    """(t, psi record (nrec, nx, ny) complex128, final field): every rec_every-th step, step 0
    included, as blindno.gpe.solve_batch_2d records them."""
    x = np.asarray(x, dtype=np.float64)
    y = np.asarray(y, dtype=np.float64)
    kx = gpe_ref.wavenumbers(len(x), x[1] - x[0])
    ky = gpe_ref.wavenumbers(len(y), y[1] - y[0])
    nt = int(t_final / dt) + 1
    t = np.linspace(0, t_final, nt)
    st = stages(order)
    psi = np.array(psi0, dtype=np.complex128)
    rec = [psi.copy()]
    for i in range(1, nt):
        for kind, c in st:
            psi = nonlinear(psi, c * dt, V, g, kappa) if kind == "n" else lin(psi, c * dt, kx, ky)
        if i % rec_every == 0:
            rec.append(psi.copy())
    return t[::rec_every][:len(rec)], np.stack(rec, 0), psi


def training_potentials(num_orbits, x, y, rng=np.random):
    """Per orbit, in this order: a ~ U(0.1, 0.3), b ~ U(0.5, 2), c ~ U(0.5, 2), x0 ~ U(-3, 3),
    y0 ~ U(-3, 3); V = a((x-x0)^2 + (y-y0)^2) + b cos^2(c(x-x0)) cos^2(c(y-y0))  -> (M, Nx, Ny)."""
    Vs = []
    for _ in range(num_orbits):
        a = rng.uniform(0.1, 0.3)
        b = rng.uniform(0.5, 2)
        c = rng.uniform(0.5, 2)
        x0 = rng.uniform(-3, 3)
        y0 = rng.uniform(-3, 3)
        V = np.empty((len(x), len(y)))
        for i, xv in enumerate(x):
            V[i] = a * ((xv - x0) ** 2 + (y - y0) ** 2) + b * np.cos(c * (xv - x0)) ** 2 * np.cos(c * (y - y0)) ** 2
        Vs.append(V)
    return np.stack(Vs, 0)


def generate(num_orbits, Nx, Ny, dt=0.005, t_final=5.0, order=2, rng=np.random):
    """The generator's dict in fp64: y = |psi|[::10] under psi0 = ic2(x) ic2(y), g = kappa = 2."""
    x = np.linspace(-10, 10, Nx)
    y = np.linspace(-10, 10, Ny)
    V = training_potentials(num_orbits, x, y, rng)
    psi0 = gpe_ref.initial_condition(2, x)[:, None] * gpe_ref.initial_condition(2, y)[None, :]
    ys = [np.abs(solve(psi0, x, y, dt, t_final, order, 2.0, 2.0, V[m], rec_every=10)[1]) for m in range(num_orbits)]
    return {"y": np.stack(ys, 0), "g": np.full(num_orbits, 2), "kappa": np.full(num_orbits, 2), "V": V}


def time_averaged_L2_error(t, rho_ref, rho_pred, x, y, eps=1e-12):
    """numpy.trapz applied twice per frame, then the trapezoid time average."""
    trapz = getattr(np, "trapezoid", None) or np.trapz
    num = trapz(trapz((rho_pred - rho_ref) ** 2, x, axis=1), y, axis=1)
    den = trapz(trapz(rho_ref ** 2, x, axis=1), y, axis=1)
    rel = np.sqrt(num) / (np.sqrt(den) + eps)
    return float(trapz(rel, t) / (t[-1] - t[0]))
