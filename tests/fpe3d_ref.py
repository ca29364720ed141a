"""Independent assembly of the Fokker-Planck master matrix on 1D / 2D / 3D grids, the checker of
tests/test_fpe_nd.py and tests/test_gpu_fpe_nd.py (test infrastructure, never the product).

The method is the one blindno.fpe states (Holubec, Kroy & Steffenoni, PRE 99, 032117, 2019): cell
i hops to its neighbour j = i +- e_d at rate
    (D_i + D_j) / 2 / h_d^2 * exp(-beta (U_j - U_i - W_ij) / 2),   W_ij = +-h_d (F_d,i + F_d,j) / 2,
no hop across a reflecting wall, a wrapped hop across a periodic one; M[j, i] = rate(i -> j),
M[i, i] = -sum_j rate(i -> j).  Assembled here from explicit (source, target) index lists per axis
and direction into a scipy.sparse matrix -- neither the np.roll construction of blindno.fpe nor a
per-cell coefficient table -- and propagated with scipy.sparse.linalg.expm_multiply.
"""
from __future__ import annotations

import numpy as np


def master_matrix(U, F, D, h, beta, periodic):
    """Sparse CSC M for potential U (shape S), force F (ndim, *S), diffusion D (S), cell widths h
    (ndim,) and per-axis periodic flags."""
    import scipy.sparse as sp
    U = np.asarray(U, dtype=np.float64)
    S = U.shape
    N = U.size
    flat = np.arange(N).reshape(S)
    Uf, Df = U.reshape(-1), np.asarray(D, dtype=np.float64).reshape(-1)
    rows, cols, vals = [], [], []
    for d in range(len(S)):
        Fd = np.asarray(F[d], dtype=np.float64).reshape(-1)
        for step in (+1, -1):
            src = np.moveaxis(flat, d, 0)
            if step == +1:
                i, j = src[:-1], src[1:]            # interior hops i -> i + e_d
                wi, wj = src[-1:], src[:1]          # the hop across the boundary
            else:
                i, j = src[1:], src[:-1]
                wi, wj = src[:1], src[-1:]
            if periodic[d] and S[d] > 1:
                i, j = np.concatenate([i, wi]), np.concatenate([j, wj])
            elif periodic[d]:                       # one cell: it is its own neighbour
                i, j = wi, wj
            i, j = i.reshape(-1), j.reshape(-1)
            W = step * h[d] * (Fd[i] + Fd[j]) / 2
            rate = (Df[i] + Df[j]) / 2 / h[d] ** 2 * np.exp(-beta * (Uf[j] - Uf[i] - W) / 2)
            rows += [j, i]                          # gain of j, loss of i
            cols += [i, i]
            vals += [rate, -rate]
    return sp.coo_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))),
                         shape=(N, N)).tocsc()


def matrix_of(sim):
    """master_matrix of a blindno.fpe.fokker_planck's fields."""
    periodic = [b.name == "periodic" for b in sim.boundary]
    return master_matrix(sim.potential_values, sim.force_values, sim.diffusion, sim.resolution,
                         sim.beta, periodic)


def dense_from_coefficients_nd(c, dims):
    """The dense matrix a (7, N) coefficient table [diag, cxm, cxp, cym, cyp, czm, czp] stands
    for under blindno_fp_propagate_nd's addressing (cell i = (ix*ny + iy)*nz + iz, wrapping)."""
    nx, ny, nz = dims
    N = nx * ny * nz
    M = np.zeros((N, N))
    for i in range(N):
        ix, r = divmod(i, ny * nz)
        iy, iz = divmod(r, nz)
        at = lambda a, b, cc: ((a % nx) * ny + (b % ny)) * nz + (cc % nz)   # noqa: E731
        M[i, i] -= c[0, i]
        M[i, at(ix - 1, iy, iz)] += c[1, i]
        M[i, at(ix + 1, iy, iz)] += c[2, i]
        M[i, at(ix, iy - 1, iz)] += c[3, i]
        M[i, at(ix, iy + 1, iz)] += c[4, i]
        M[i, at(ix, iy, iz - 1)] += c[5, i]
        M[i, at(ix, iy, iz + 1)] += c[6, i]
    return M


def propagate(M, p0, tf, nsteps):
    """exp(M t) p0 at t = linspace(0, tf, nsteps) (rows)."""
    from scipy.sparse.linalg import expm_multiply
    return expm_multiply(M, p0, start=0, stop=tf, num=nsteps, endpoint=True)


# ---------------------------------------------------------------- simulators the two test files share
# blindno.fpe.fokker_planck objects on small grids whose potential, non-conservative force and drag
# field differ per trajectory ``k`` and are asymmetric along every axis (so a swapped pair of
# neighbour coefficients or a wrong wrap changes the result).
NM = 1e-9


def make_sim(dims, periodic, k=0, fields=True):
    """A simulator on a grid of ``dims`` cells (trailing 1s dropped: (37, 1, 1) is 1D), 10 nm
    cells, ``periodic`` a flag per axis.  ``fields=False``: free diffusion at constant drag."""
    from blindno import fpe
    shape = [n for n in dims if n > 1] or [dims[0]]
    nd = len(shape)
    ext = [(n - 0.5) * 10 * NM for n in shape]      # ceil(extent / resolution) = n exactly
    kT = fpe.K_B * 300.0
    bnd = [fpe.boundary.periodic if periodic[d] else fpe.boundary.reflecting for d in range(nd)]
    if not fields:
        return fpe.fokker_planck(temperature=300, drag=1e-9 * (1 + 0.2 * k), extent=ext, resolution=10 * NM,
                                 boundary=bnd)

    def pot(*g):
        v = (0.6 + 0.2 * k) * kT * np.ones_like(g[0])
        for d, a in enumerate(g):
            v = v * np.cos(2 * np.pi * a / ext[d] + 0.4 * (d + 1) + 0.3 * k)
        return v + sum(0.02 * (d + 1) * kT * a / (10 * NM) for d, a in enumerate(g))

    def force(*g):
        return np.array([(2 + d + k) * 1e-14 * np.sin(2 * np.pi * g[(d + 1) % nd] / ext[(d + 1) % nd] + 0.2 * d)
                         + 0 * g[0] for d in range(nd)])

    def drag(*g):
        r2 = sum((a - (d + 1) * 7 * NM) ** 2 for d, a in enumerate(g))
        return 1e-9 * (1.0 + (0.3 + 0.1 * k) * np.exp(-r2 / (60 * NM) ** 2))

    return fpe.fokker_planck(temperature=300, drag=drag, extent=ext, resolution=10 * NM, potential=pot,
                             force=force, boundary=bnd)


def initial(sim, k=0):
    """A normalised off-centre Gaussian bump on the simulator's grid, flattened."""
    v = np.ones_like(sim.grid[0])
    for d, a in enumerate(sim.grid):
        c = (0.15 * (d + 1) - 0.1 * k) * a.max()
        v = v * np.exp(-((a - c) / (25 * NM)) ** 2)
    v = v.reshape(-1)
    return v / v.sum()
