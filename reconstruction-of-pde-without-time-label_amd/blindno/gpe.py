"""Gross-Pitaevskii data generators / density propagators and the density-error metrics on the
GPU, fp64 like the reference: 1D (libblindno ``blindno_gpe_solve`` / ``blindno_trapz_rows``) and
2D (``blindno_gpe2d_solve`` / ``blindno_trapz2_frames``, the ``*_2d`` functions, with the
record-free ``solve_error_batch_2d`` on ``blindno_gpe2d_error``) and 3D
(``blindno_gpe3d_solve`` / ``blindno_trapz3_frames``, the ``*_3d`` functions at the end, with the
record-free ``solve_error_batch_3d`` on ``blindno_gpe3d_error``).

Reference (yl602019618/Reconstruction-of-PDE-without-Time-Label):
  get_initial_condition, solve_GPE_custom, generate_and_save_training_data
      1d_GPE/datagen_GPE.py:7-21, 86-115, 120-191
  time_averaged_L2_error
      1d_FPE/compute_time_error.py:240-295 = 1d_GPE/compute_time_error_GPE.py:162-203

The reference integrates one trajectory at a time in numpy (0.06 s per 1001-step trajectory at
Nx = 128); here every trajectory of a batch is one workgroup that keeps its field, twiddles and
phase tables in LDS for the whole time loop.
"""
from __future__ import annotations

from typing import Optional, Sequence, Union

import numpy as np
import torch

from ._lib import BlindnoError, call, ptr, query, stream_ptr

F64 = torch.float64


def initial_condition(ic: int, x: np.ndarray) -> np.ndarray:
    """get_initial_condition (1d_GPE/datagen_GPE.py:7-21)."""
    if ic == 1:
        return np.exp(-x ** 2 / 10)
    if ic == 2:
        return 2 * np.sin(x) / (np.exp(x) + np.exp(-x))
    if ic == 3:
        return 2 * np.cos(x) / (np.exp(x) + np.exp(-x))
    raise ValueError("ic must be 1, 2 or 3")


def _dev(device):
    dev = torch.device(device if device is not None else "cuda")
    if dev.type != "cuda":
        raise BlindnoError("the GPE solver runs on the HIP device only (there is no CPU path)")
    return dev


def solve_batch(psi0, x, dt: float, t_final: float, order: int, g, kappa, V, rec_every: int = 1,
                want_abs: bool = True, want_psi: bool = False, device=None):
    """Integrate B trajectories at once.

    psi0: (Nx,) or (B, Nx) complex initial field; V: (Nx,) or (B, Nx); g, kappa: scalars or
    (B,).  Returns a dict with ``t`` (numpy, the recorded times), ``abs`` (B, nrec, Nx) fp64
    device tensor of |psi| (if ``want_abs``), ``psi`` (B, nrec, Nx) complex128 (if
    ``want_psi``) and ``final`` (B, Nx) complex128.  Records every ``rec_every``-th step,
    step 0 included (``psi_abs[::rec_every]`` of the reference's full record)."""
    dev = _dev(device)
    x = np.asarray(x, dtype=np.float64)
    N = len(x)
    V = np.atleast_2d(np.asarray(V, dtype=np.float64))
    B = V.shape[0]
    psi0 = np.asarray(psi0, dtype=np.complex128)
    batched = psi0.ndim == 2
    if batched and psi0.shape[0] != B:
        raise BlindnoError("psi0 and V batch sizes differ")
    g = np.broadcast_to(np.asarray(g, dtype=np.float64), (B,)).copy()
    kappa = np.broadcast_to(np.asarray(kappa, dtype=np.float64), (B,)).copy()
    if N & (N - 1) or N < 4 or N > 2048:
        raise BlindnoError(f"Nx = {N}: the solver needs a power of two in [4, 2048]")
    nt = int(t_final / dt) + 1
    nsteps = nt - 1
    nrec = nsteps // rec_every + 1
    t_full = np.linspace(0, t_final, nt)
    p0 = torch.from_numpy(np.ascontiguousarray(psi0.view(np.float64))).to(dev)
    Vd = torch.from_numpy(np.ascontiguousarray(V)).to(dev)
    gd = torch.from_numpy(g).to(dev)
    kd = torch.from_numpy(kappa).to(dev)
    rabs = torch.empty(B, nrec, N, dtype=F64, device=dev) if want_abs else None
    rpsi = torch.empty(B, nrec, N, 2, dtype=F64, device=dev) if want_psi else None
    fin = torch.empty(B, N, 2, dtype=F64, device=dev)
    dx = float(x[1] - x[0])
    call("blindno_gpe_solve", ptr(p0), ptr(Vd), ptr(gd), ptr(kd), dx, float(dt), nsteps, int(order),
         int(rec_every), ptr(rabs), ptr(rpsi), ptr(fin), B, N, int(batched), stream_ptr(dev))
    out = {"t": t_full[::rec_every][:nrec], "final": torch.view_as_complex(fin)}
    if want_abs:
        out["abs"] = rabs
    if want_psi:
        out["psi"] = torch.view_as_complex(rpsi)
    return out


def solve_GPE_custom(init_func, x, dt, t_final, order, g, kappa, V):
    """Drop-in for the reference's ``solve_GPE_custom`` (1d_GPE/datagen_GPE.py:86-115): same
    arguments, returns (t, psi_record (Nt, Nx) complex128 numpy), computed on the GPU."""
    x = np.asarray(x, dtype=np.float64)
    r = solve_batch(init_func(x), x, dt, t_final, order, g, kappa, V, rec_every=1,
                    want_abs=False, want_psi=True)
    return np.linspace(0, t_final, int(t_final / dt) + 1), r["psi"][0].cpu().numpy()


def generate_training_data(num_orbits: int = 6000, Nx: int = 128, dt: float = 0.005,
                           t_final: float = 5.0, order: int = 2, num_time_samples: int = 100,
                           rng=np.random, device=None, batch: int = 4096):
    """generate_and_save_training_data (1d_GPE/datagen_GPE.py:120-191) without the file write:
    the same parameter draws from ``rng`` in the reference's order (a, b, c, x0, then the
    unused time-sample choice), initial condition 2, g = kappa = 2, y = |psi|[::10].  All
    orbits are integrated in batched launches.  Returns the reference's dict
    {'y': (M, Nt//10 + 1, Nx), 'g', 'kappa', 'V'} as numpy arrays."""
    x = np.linspace(-10, 10, Nx)
    nt = int(t_final / dt) + 1
    Vs, gs, ks = [], [], []
    for _ in range(num_orbits):
        a = rng.uniform(0.1, 0.3)
        b = rng.uniform(0.5, 2)
        c = rng.uniform(0.5, 2)
        x0 = rng.uniform(-3, 3)
        Vs.append(a * (x - x0) ** 2 + b * (np.cos(c * (x - x0))) ** 2)
        gs.append(2)
        ks.append(2)
        np.sort(rng.choice(np.arange(nt), size=num_time_samples, replace=False))
    V = np.stack(Vs, 0)
    psi0 = initial_condition(2, x)
    ys = []
    for s in range(0, num_orbits, batch):
        r = solve_batch(psi0, x, dt, t_final, order, 2.0, 2.0, V[s:s + batch], rec_every=10,
                        device=device)
        ys.append(r["abs"].cpu().numpy())
    return {"y": np.concatenate(ys, 0), "g": np.array(gs), "kappa": np.array(ks), "V": V}


def save_training_data(data: dict, save_path: str) -> None:
    """The reference's on-disk format: ``np.save`` of the dict (datagen_GPE.py:183-189);
    train_fno_GPE.py:38 reads it back with ``np.load(..., allow_pickle=True).item()``."""
    np.save(save_path, data, allow_pickle=True)


def time_averaged_L2_error(time_ref, rho_ref, time_pred, rho_pred, grid, eps: float = 1e-12,
                           device=None) -> float:
    """1d_FPE/compute_time_error.py:240-295: per-time sqrt(trapz((rho_pred - rho_ref)^2, x)) /
    (sqrt(trapz(rho_ref^2, x)) + eps), then the trapezoid time average / (t_end - t_0).
    rho_* are (Nt, Nx) numpy arrays or device tensors; the spatial integrals run on the GPU
    in fp64."""
    dev = _dev(device if device is not None else (rho_ref.device if torch.is_tensor(rho_ref) else None))
    if tuple(rho_ref.shape) != tuple(rho_pred.shape):
        raise ValueError(f"rho_ref shape {tuple(rho_ref.shape)} != rho_pred shape {tuple(rho_pred.shape)}")
    if isinstance(grid, (list, tuple)):
        if len(grid) != 1:
            raise ValueError(f"unsupported grid: len(grid) = {len(grid)}")
        xg = np.asarray(grid[0])
    else:
        xg = np.asarray(grid)
        if xg.ndim == 2 and xg.shape[0] == 1:
            xg = xg[0]
        elif xg.ndim != 1:
            raise ValueError(f"unsupported grid shape {xg.shape}")
    if not np.allclose(np.asarray(time_ref), np.asarray(time_pred)):
        raise ValueError("time_ref and time_pred differ")

    def d64(a):
        t = a if torch.is_tensor(a) else torch.from_numpy(np.asarray(a))
        return t.to(dev, F64).contiguous()

    a, b = d64(rho_pred), d64(rho_ref)
    xd = d64(xg)
    nt, n = a.shape
    s = torch.empty(nt, 2, dtype=F64, device=dev)
    call("blindno_trapz_rows", ptr(a), ptr(b), ptr(xd), ptr(s), nt, n, stream_ptr(dev))
    rel = s[:, 0].clamp_min(0).sqrt() / (s[:, 1].clamp_min(0).sqrt() + eps)
    t = d64(time_ref)
    integral = (0.5 * (rel[:-1] + rel[1:]) * (t[1:] - t[:-1])).sum()
    return float(integral / (t[-1] - t[0]))


# ------------------------------------------------------------------------------ 2D and 3D
# The reference lists a 2D GPE experiment and ships no code for it; what follows is the project's
# own: the 1D scheme above carried to two and three dimensions (csrc/gpe_nd.hip, grid-resident:
# the field lives in global memory and every kinetic step is one launch per axis).  The ``_*_nd``
# functions are the bodies; the public ``*_2d`` / ``*_3d`` functions pass them their grids and
# their launch limit, and everything else follows from the number of grids.

# The launches one solve_batch_2d call may enqueue (2 per Strang step, 8 per Yoshida step).
# Largest power of two whose worst case stays under 120 s at the time per launch measured by
# tools/bench_gpe2d.py at 256^2, B = 16 (profiles/gpe2d_bench.json: 31.16 us per launch;
# 120 s / 31.16 us = 3.85 M, 2^21 launches take 65.4 s and 2^22 would take 130.7 s).
MAX_LAUNCHES_2D = 1 << 21
# The launches one solve_batch_3d call may enqueue (3 per Strang step, 12 per Yoshida step).  The
# rule of MAX_LAUNCHES_2D: the largest power of two whose worst case stays under 120 s at the time
# per launch measured by tools/bench_gpe3d.py at its headline shape, 64^3 with B = 16
# (profiles/gpe3d_bench.json: 77.39 us per launch; 120 s / 77.39 us = 1.55 M, 2^20 launches take
# 81.1 s and 2^21 would take 162.3 s).
MAX_LAUNCHES_3D = 1 << 20
# The bytes of record (|psi| and psi together) one call may allocate: 8 GiB.
MAX_RECORD_BYTES = 8 << 30


def _problem_nd(psi0, grids, g, kappa, V, order, rec_every):
    """The host-side checks that the solve and error functions share, in their order.  Returns
    (grids, shape, psi0, batched, g, kappa, V) as fp64 / complex128 numpy, V with its batch axis."""
    grids = [np.asarray(a, dtype=np.float64) for a in grids]
    dim = len(grids)
    shape = tuple(len(a) for a in grids)
    dims = ", ".join(str(n) for n in shape)
    V = np.asarray(V, dtype=np.float64)
    if V.ndim == dim:
        V = V[None]
    if V.ndim != dim + 1 or V.shape[1:] != shape:
        raise BlindnoError(f"V has shape {V.shape}; expected (B, {dims}) or ({dims})")
    B = V.shape[0]
    psi0 = np.asarray(psi0, dtype=np.complex128)
    batched = psi0.ndim == dim + 1
    if psi0.shape[-dim:] != shape or psi0.ndim not in (dim, dim + 1):
        raise BlindnoError(f"psi0 has shape {psi0.shape}; expected (B, {dims}) or ({dims})")
    if batched and psi0.shape[0] != B:
        raise BlindnoError("psi0 and V batch sizes differ")
    g = np.broadcast_to(np.asarray(g, dtype=np.float64), (B,)).copy()
    kappa = np.broadcast_to(np.asarray(kappa, dtype=np.float64), (B,)).copy()
    for name, n in zip(("Nx", "Ny", "Nz"), shape):
        if n & (n - 1) or n < 4 or n > 1024:
            raise BlindnoError(f"{name} = {n}: the {dim}D solver needs a power of two in [4, 1024]")
    if dim == 3 and int(np.prod(shape)) > 1 << 24:      # the 2D entries set no cell limit
        raise BlindnoError(f"{' x '.join(str(n) for n in shape)} cells: the 3D solver takes at most 2^24 per trajectory")
    if order not in (2, 4):
        raise BlindnoError(f"order = {order}: the solver has orders 2 and 4")
    if int(rec_every) < 1:
        raise BlindnoError(f"rec_every = {rec_every}: must be at least 1")
    return grids, shape, psi0, batched, g, kappa, V


def _upload(dev, psi0, V, g, kappa):
    # fresh C-ordered copies: the inputs may be read-only or broadcast views
    p0 = torch.from_numpy(np.array(psi0, order="C").view(np.float64)).to(dev)
    Vd = torch.from_numpy(np.array(V, order="C")).to(dev)
    return p0, Vd, torch.from_numpy(g).to(dev), torch.from_numpy(kappa).to(dev)


def _solve_batch_nd(psi0, grids, dt, t_final, order, g, kappa, V, rec_every, want_abs, want_psi, abs_dtype,
                    device, max_launches):
    grids, shape, psi0, batched, g, kappa, V = _problem_nd(psi0, grids, g, kappa, V, order, rec_every)
    dim, B, cells = len(grids), V.shape[0], int(np.prod(shape))
    if abs_dtype not in (torch.float64, torch.float32):
        raise BlindnoError(f"abs_dtype = {abs_dtype}: |psi| is recorded in float64 or float32")
    nt = int(t_final / dt) + 1
    nsteps = nt - 1
    nrec = nsteps // int(rec_every) + 1
    launches = query(f"blindno_gpe{dim}d_launches", nsteps, int(order))
    if launches > max_launches:
        raise BlindnoError(
            f"{nsteps} steps of order {order} are {launches} kernel launches (limit MAX_LAUNCHES_{dim}D = "
            f"{max_launches}); refusing to launch -- integrate in several calls, continuing from 'final'")
    abs_bytes = 8 if abs_dtype == torch.float64 else 4
    rec_bytes = B * nrec * cells * ((abs_bytes if want_abs else 0) + (16 if want_psi else 0))
    if rec_bytes > MAX_RECORD_BYTES:
        raise BlindnoError(
            f"the record of {B} trajectories x {nrec} frames x {' x '.join(str(n) for n in shape)} is {rec_bytes} "
            f"bytes (limit MAX_RECORD_BYTES = {MAX_RECORD_BYTES}); refusing to launch -- raise rec_every, record "
            f"float32 |psi| or solve fewer trajectories per call")
    dev = _dev(device)
    t_full = np.linspace(0, t_final, nt)
    p0, Vd, gd, kd = _upload(dev, psi0, V, g, kappa)
    rabs = torch.empty(B, nrec, *shape, dtype=abs_dtype, device=dev) if want_abs else None
    rpsi = torch.empty(B, nrec, *shape, 2, dtype=F64, device=dev) if want_psi else None
    fin = torch.empty(B, *shape, 2, dtype=F64, device=dev)
    scratch = torch.empty(query(f"blindno_gpe{dim}d_scratch_doubles", B, *shape), dtype=F64, device=dev)
    call(f"blindno_gpe{dim}d_solve", ptr(p0), ptr(Vd), ptr(gd), ptr(kd), *(float(a[1] - a[0]) for a in grids),
         float(dt), nsteps, int(order), int(rec_every), ptr(rabs), int(abs_dtype == torch.float32), ptr(rpsi),
         ptr(fin), ptr(scratch), B, *shape, int(batched), stream_ptr(dev))
    out = {"t": t_full[::rec_every][:nrec], "final": torch.view_as_complex(fin)}
    if want_abs:
        out["abs"] = rabs
    if want_psi:
        out["psi"] = torch.view_as_complex(rpsi)
    return out


def _solve_error_batch_nd(psi0, grids, dt, t_final, order, g, kappa, V, group, rec_every, device, max_launches):
    grids, shape, psi0, batched, g, kappa, V = _problem_nd(psi0, grids, g, kappa, V, order, rec_every)
    dim, B = len(grids), V.shape[0]
    group = B if group is None else int(group)
    if group < 1 or B % group:
        raise BlindnoError(f"{B} trajectories are not whole groups of {group}")
    nt = int(t_final / dt) + 1
    nsteps = nt - 1
    nrec = nsteps // int(rec_every) + 1
    launches = query(f"blindno_gpe{dim}d_error_launches", nsteps, int(order), int(rec_every))
    if launches > max_launches:
        raise BlindnoError(
            f"{nsteps} steps of order {order} with {nrec} reduced frames are {launches} kernel launches (limit "
            f"MAX_LAUNCHES_{dim}D = {max_launches}); refusing to launch -- raise rec_every or shorten t_final")
    doubles = query(f"blindno_gpe{dim}d_error_scratch_doubles", B, *shape)
    if 8 * doubles > MAX_RECORD_BYTES:
        raise BlindnoError(
            f"the scratch of {B} trajectories x {' x '.join(str(n) for n in shape)} is {8 * doubles} bytes (limit "
            f"MAX_RECORD_BYTES = {MAX_RECORD_BYTES}); refusing to launch -- solve fewer groups per call")
    dev = _dev(device)
    t_full = np.linspace(0, t_final, nt)
    p0, Vd, gd, kd = _upload(dev, psi0, V, g, kappa)
    gridsd = [torch.from_numpy(np.array(a)).to(dev) for a in grids]
    err = torch.empty(B, nrec, 2, dtype=F64, device=dev)
    scratch = torch.empty(doubles, dtype=F64, device=dev)
    call(f"blindno_gpe{dim}d_error", ptr(p0), ptr(Vd), ptr(gd), ptr(kd), *(ptr(a) for a in gridsd),
         *(float(a[1] - a[0]) for a in grids), float(dt), nsteps, int(order), int(rec_every), group, ptr(err),
         ptr(scratch), B, *shape, int(batched), stream_ptr(dev))
    return {"t": t_full[::rec_every][:nrec], "num": err[:, :, 0], "den": err[:, :, 1]}


def _time_averaged_L2_error_nd(dim, time_ref, rho_ref, time_pred, rho_pred, grid, eps, device):
    axes = "xyz"[:dim]
    dev = _dev(device if device is not None else (rho_ref.device if torch.is_tensor(rho_ref) else None))
    if tuple(rho_ref.shape) != tuple(rho_pred.shape) or len(rho_ref.shape) != dim + 1:
        raise ValueError(f"rho_ref shape {tuple(rho_ref.shape)} / rho_pred shape {tuple(rho_pred.shape)}: "
                         f"expected two equal (Nt, {', '.join('N' + a for a in axes)}) arrays")
    if not isinstance(grid, (list, tuple)) or len(grid) != dim:
        raise ValueError(f"grid must be ({', '.join(axes)})")
    gs = [np.asarray(a, dtype=np.float64).reshape(-1) for a in grid]
    nt, *shape = (int(v) for v in rho_ref.shape)
    if [len(a) for a in gs] != shape:
        raise ValueError(f"grid sizes {tuple(len(a) for a in gs)} do not match the frames {tuple(shape)}")
    if not np.allclose(np.asarray(time_ref), np.asarray(time_pred)):
        raise ValueError("time_ref and time_pred differ")

    def d64(a):
        t = a if torch.is_tensor(a) else torch.from_numpy(np.asarray(a))
        return t.to(dev, F64).contiguous()

    a, b = d64(rho_pred), d64(rho_ref)
    gsd = [d64(a_) for a_ in gs]
    s = torch.empty(nt, 2, dtype=F64, device=dev)
    call(f"blindno_trapz{dim}_frames", ptr(a), ptr(b), *(ptr(a_) for a_ in gsd), ptr(s), nt, *shape, stream_ptr(dev))
    return time_averaged_L2_error_from_sums(d64(time_ref), s[:, 0], s[:, 1], eps)


def time_averaged_L2_error_from_sums(t, num, den, eps: float = 1e-12) -> float:
    """The end of ``time_averaged_L2_error_2d`` / ``_3d``, shared with the record-free path: from the
    per-time integrals num = trapz((rho_pred - rho_ref)^2) and den = trapz(rho_ref^2), (Nt,) each,
    rel = sqrt(max(num, 0)) / (sqrt(max(den, 0)) + eps), then the trapezoid time average of rel over
    ``t`` divided by (t_end - t_0).  ``num`` / ``den`` are fp64 tensors (on any device) or arrays;
    ``t`` is brought to their device."""
    num = num if torch.is_tensor(num) else torch.from_numpy(np.asarray(num, dtype=np.float64))
    den = den if torch.is_tensor(den) else torch.from_numpy(np.asarray(den, dtype=np.float64))
    t = t if torch.is_tensor(t) else torch.from_numpy(np.asarray(t, dtype=np.float64))
    t = t.to(num.device, F64)
    rel = num.clamp_min(0).sqrt() / (den.clamp_min(0).sqrt() + eps)
    integral = (0.5 * (rel[:-1] + rel[1:]) * (t[1:] - t[:-1])).sum()
    return float(integral / (t[-1] - t[0]))


# ------------------------------------------------------------------------------------- 2D

def solve_batch_2d(psi0, x, y, dt: float, t_final: float, order: int, g, kappa, V,
                   rec_every: int = 1, want_abs: bool = True, want_psi: bool = False,
                   abs_dtype=torch.float64, device=None):
    """``solve_batch`` on a periodic 2D grid: integrate B trajectories at once.

    psi0: (Nx, Ny) or (B, Nx, Ny) complex initial field; V: (Nx, Ny) or (B, Nx, Ny); g, kappa:
    scalars or (B,); x (Nx), y (Ny) uniform grids, each a power of two in [4, 1024] points.
    Returns a dict with ``t`` (numpy, the recorded times), ``abs`` (B, nrec, Nx, Ny) device tensor
    of |psi| in ``abs_dtype`` (fp64, or fp32 = the fp64 value rounded on the device; if
    ``want_abs``), ``psi`` (B, nrec, Nx, Ny) complex128 (if ``want_psi``) and ``final``
    (B, Nx, Ny) complex128.  Records every ``rec_every``-th step, step 0 included.

    Refused before anything is launched (BlindnoError): a request of more than MAX_LAUNCHES_2D
    kernel launches, a record above MAX_RECORD_BYTES, and whatever blindno_gpe2d_solve refuses."""
    return _solve_batch_nd(psi0, (x, y), dt, t_final, order, g, kappa, V, rec_every, want_abs, want_psi, abs_dtype,
                           device, MAX_LAUNCHES_2D)


def training_potentials_2d(num_orbits: int, x: np.ndarray, y: np.ndarray, rng=np.random) -> np.ndarray:
    """The random draws of ``generate_training_data_2d``, per orbit in this order: a ~ U(0.1, 0.3),
    b ~ U(0.5, 2), c ~ U(0.5, 2), x0 ~ U(-3, 3), y0 ~ U(-3, 3) ->
    V = a ((x - x0)^2 + (y - y0)^2) + b cos^2(c (x - x0)) cos^2(c (y - y0)), (M, Nx, Ny)."""
    X, Y = x[:, None], y[None, :]
    Vs = []
    for _ in range(num_orbits):
        a = rng.uniform(0.1, 0.3)
        b = rng.uniform(0.5, 2)
        c = rng.uniform(0.5, 2)
        x0 = rng.uniform(-3, 3)
        y0 = rng.uniform(-3, 3)
        Vs.append(a * ((X - x0) ** 2 + (Y - y0) ** 2) + b * np.cos(c * (X - x0)) ** 2 * np.cos(c * (Y - y0)) ** 2)
    return np.stack(Vs, 0)


def generate_training_data_2d(num_orbits: int, Nx: int = 256, Ny: int = 256, dt: float = 0.005,
                              t_final: float = 5.0, order: int = 2, rng=np.random, device=None,
                              batch: int = 16, y_dtype=np.float32):
    """The 2D GPE training set (the project's own generator: the reference has none).  Per orbit
    the draws of ``training_potentials_2d`` on [-10, 10]^2, psi0 = ic2(x) ic2(y) (initial
    condition 2 along each axis), g = kappa = 2, y = |psi|[::10].  Returns the 1D generator's dict
    {'y': (M, Nt//10 + 1, Nx, Ny), 'g', 'kappa', 'V'}, so ``save_training_data`` and
    ``data.ParameterDataset`` take it unchanged.

    Unlike the 1D generator, whose record is fp64 as the reference's, ``y`` is float32 by default
    (``y_dtype=np.float64`` for the full record): a 256^2 orbit's 101 frames are 53 MB in fp64,
    and the models read float32.  The cast happens on the device, before the host copy, and is
    the fp64 value rounded once."""
    if np.dtype(y_dtype) not in (np.dtype(np.float32), np.dtype(np.float64)):
        raise ValueError("y_dtype must be float32 or float64")
    x = np.linspace(-10, 10, Nx)
    y = np.linspace(-10, 10, Ny)
    V = training_potentials_2d(num_orbits, x, y, rng)
    psi0 = initial_condition(2, x)[:, None] * initial_condition(2, y)[None, :]
    tdt = torch.float32 if np.dtype(y_dtype) == np.dtype(np.float32) else torch.float64
    ys = []
    for s in range(0, num_orbits, batch):
        r = solve_batch_2d(psi0, x, y, dt, t_final, order, 2.0, 2.0, V[s:s + batch], rec_every=10,
                           abs_dtype=tdt, device=device)
        ys.append(r["abs"].cpu().numpy())
    return {"y": np.concatenate(ys, 0), "g": np.full(num_orbits, 2), "kappa": np.full(num_orbits, 2), "V": V}


def time_averaged_L2_error_2d(time_ref, rho_ref, time_pred, rho_pred, grid, eps: float = 1e-12,
                              device=None) -> float:
    """``time_averaged_L2_error`` for (Nt, Nx, Ny) densities on ``grid = (x, y)``: per time
    sqrt(trapz_y(trapz_x((rho_pred - rho_ref)^2))) / (sqrt(trapz_y(trapz_x(rho_ref^2))) + eps),
    then the trapezoid time average / (t_end - t_0).  rho_* are numpy arrays or device tensors;
    the spatial integrals run on the GPU in fp64 (blindno_trapz2_frames)."""
    return _time_averaged_L2_error_nd(2, time_ref, rho_ref, time_pred, rho_pred, grid, eps, device)


def solve_error_batch_2d(psi0, x, y, dt: float, t_final: float, order: int, g, kappa, V,
                         group: Optional[int] = None, rec_every: int = 1, device=None):
    """``solve_batch_2d`` without a record (blindno_gpe2d_error): the same B trajectories, integrated
    by the same launch sequence, but of every ``rec_every``-th step only the two integrals
    ``time_averaged_L2_error_2d`` needs come back.  Trajectories come in consecutive groups of
    ``group`` (default: the whole batch) whose first member is the group's reference.

    psi0, x, y, dt, t_final, order, g, kappa, V: as in ``solve_batch_2d``.  Returns a dict with ``t``
    (numpy, the recorded times) and the fp64 device tensors ``num`` (B, nrec) =
    trapz_y trapz_x (|psi_b| - |psi_ref(b)|)^2 and ``den`` (B, nrec) = the same integral of
    |psi_ref(b)|^2; ``num`` of a reference is exactly 0.  The device holds three doubles per cell and
    trajectory whatever nrec is (the working field and one |psi| frame), plus two per 1024 cells;
    ``time_averaged_L2_error_from_sums`` turns a trajectory's two rows into its error.

    Refused before anything is launched (BlindnoError): a batch that is not whole groups, more than
    MAX_LAUNCHES_2D kernel launches (blindno_gpe2d_error_launches: the solver's plus two per recorded
    step), scratch above MAX_RECORD_BYTES, and whatever blindno_gpe2d_error refuses."""
    return _solve_error_batch_nd(psi0, (x, y), dt, t_final, order, g, kappa, V, group, rec_every, device,
                                 MAX_LAUNCHES_2D)


# ------------------------------------------------------------------------------------- 3D

def solve_batch_3d(psi0, x, y, z, dt: float, t_final: float, order: int, g, kappa, V,
                   rec_every: int = 1, want_abs: bool = True, want_psi: bool = False,
                   abs_dtype=torch.float64, device=None):
    """``solve_batch_2d`` on a periodic 3D grid: integrate B trajectories at once.

    psi0: (Nx, Ny, Nz) or (B, Nx, Ny, Nz) complex initial field; V: (Nx, Ny, Nz) or
    (B, Nx, Ny, Nz); g, kappa: scalars or (B,); x (Nx), y (Ny), z (Nz) uniform grids, each a power
    of two in [4, 1024] points with Nx Ny Nz <= 2^24.  Returns a dict with ``t`` (numpy, the
    recorded times), ``abs`` (B, nrec, Nx, Ny, Nz) device tensor of |psi| in ``abs_dtype`` (fp64,
    or fp32 = the fp64 value rounded on the device; if ``want_abs``), ``psi``
    (B, nrec, Nx, Ny, Nz) complex128 (if ``want_psi``) and ``final`` (B, Nx, Ny, Nz) complex128.
    Records every ``rec_every``-th step, step 0 included.

    Refused before anything is launched (BlindnoError): a request of more than MAX_LAUNCHES_3D
    kernel launches, a record above MAX_RECORD_BYTES, and whatever blindno_gpe3d_solve refuses."""
    return _solve_batch_nd(psi0, (x, y, z), dt, t_final, order, g, kappa, V, rec_every, want_abs, want_psi,
                           abs_dtype, device, MAX_LAUNCHES_3D)


def training_potentials_3d(num_orbits: int, x: np.ndarray, y: np.ndarray, z: np.ndarray,
                           rng=np.random) -> np.ndarray:
    """The random draws of ``generate_training_data_3d``, per orbit in this order: a ~ U(0.1, 0.3),
    b ~ U(0.5, 2), c ~ U(0.5, 2), x0, y0, z0 ~ U(-3, 3) ->
    V = a ((x - x0)^2 + (y - y0)^2 + (z - z0)^2) + b cos^2(c (x - x0)) cos^2(c (y - y0)) cos^2(c (z - z0)),
    (M, Nx, Ny, Nz)."""
    X, Y, Z = x[:, None, None], y[None, :, None], z[None, None, :]
    Vs = []
    for _ in range(num_orbits):
        a = rng.uniform(0.1, 0.3)
        b = rng.uniform(0.5, 2)
        c = rng.uniform(0.5, 2)
        x0 = rng.uniform(-3, 3)
        y0 = rng.uniform(-3, 3)
        z0 = rng.uniform(-3, 3)
        Vs.append(a * ((X - x0) ** 2 + (Y - y0) ** 2 + (Z - z0) ** 2) +
                  b * np.cos(c * (X - x0)) ** 2 * np.cos(c * (Y - y0)) ** 2 * np.cos(c * (Z - z0)) ** 2)
    return np.stack(Vs, 0)


def generate_training_data_3d(num_orbits: int, Nx: int = 64, Ny: int = 64, Nz: int = 64, dt: float = 0.005,
                              t_final: float = 5.0, order: int = 2, rng=np.random, device=None,
                              batch: int = 16, y_dtype=np.float32):
    """The 3D GPE training set (the project's own generator).  Per orbit the draws of
    ``training_potentials_3d`` on [-10, 10]^3, psi0 = ic2(x) ic2(y) ic2(z), g = kappa = 2,
    y = |psi|[::10].  Returns the 1D generator's dict {'y': (M, Nt//10 + 1, Nx, Ny, Nz), 'g',
    'kappa', 'V'}, so ``save_training_data`` and ``data.ParameterDataset`` take it unchanged.

    ``y`` is float32 by default, as in 2D (``y_dtype=np.float64`` for the full record): the cast
    happens on the device and is the fp64 value rounded once.  The default ``batch`` keeps one
    call's record under MAX_RECORD_BYTES at the defaults even in fp64: 16 orbits x 101 frames x
    64^3 points x 8 B = 3.4 GB of the 8 GiB."""
    if np.dtype(y_dtype) not in (np.dtype(np.float32), np.dtype(np.float64)):
        raise ValueError("y_dtype must be float32 or float64")
    x = np.linspace(-10, 10, Nx)
    y = np.linspace(-10, 10, Ny)
    z = np.linspace(-10, 10, Nz)
    V = training_potentials_3d(num_orbits, x, y, z, rng)
    psi0 = (initial_condition(2, x)[:, None, None] * initial_condition(2, y)[None, :, None] *
            initial_condition(2, z)[None, None, :])
    tdt = torch.float32 if np.dtype(y_dtype) == np.dtype(np.float32) else torch.float64
    ys = []
    for s in range(0, num_orbits, batch):
        r = solve_batch_3d(psi0, x, y, z, dt, t_final, order, 2.0, 2.0, V[s:s + batch], rec_every=10,
                           abs_dtype=tdt, device=device)
        ys.append(r["abs"].cpu().numpy())
    return {"y": np.concatenate(ys, 0), "g": np.full(num_orbits, 2), "kappa": np.full(num_orbits, 2), "V": V}


def time_averaged_L2_error_3d(time_ref, rho_ref, time_pred, rho_pred, grid, eps: float = 1e-12,
                              device=None) -> float:
    """``time_averaged_L2_error_2d`` for (Nt, Nx, Ny, Nz) densities on ``grid = (x, y, z)``: per
    time sqrt(trapz_z(trapz_y(trapz_x((rho_pred - rho_ref)^2)))) / (sqrt(the same of rho_ref^2) +
    eps), then the trapezoid time average / (t_end - t_0).  rho_* are numpy arrays or device
    tensors; the spatial integrals run on the GPU in fp64 (blindno_trapz3_frames)."""
    return _time_averaged_L2_error_nd(3, time_ref, rho_ref, time_pred, rho_pred, grid, eps, device)


def solve_error_batch_3d(psi0, x, y, z, dt: float, t_final: float, order: int, g, kappa, V,
                         group: Optional[int] = None, rec_every: int = 1, device=None):
    """``solve_batch_3d`` without a record (blindno_gpe3d_error): the same B trajectories, integrated
    by the same launch sequence, but of every ``rec_every``-th step only the two integrals
    ``time_averaged_L2_error_3d`` needs come back.  Trajectories come in consecutive groups of
    ``group`` (default: the whole batch) whose first member is the group's reference.

    psi0, x, y, z, dt, t_final, order, g, kappa, V: as in ``solve_batch_3d``.  Returns a dict with
    ``t`` (numpy, the recorded times) and the fp64 device tensors ``num`` (B, nrec) =
    trapz_z trapz_y trapz_x (|psi_b| - |psi_ref(b)|)^2 and ``den`` (B, nrec) = the same integral of
    |psi_ref(b)|^2; ``num`` of a reference is exactly 0.  The device holds three doubles per cell and
    trajectory whatever nrec is (the working field and one |psi| frame), plus two per 1024 cells.

    Refused before anything is launched (BlindnoError): a batch that is not whole groups, more than
    MAX_LAUNCHES_3D kernel launches (blindno_gpe3d_error_launches: the solver's plus two per recorded
    step), scratch above MAX_RECORD_BYTES, and whatever blindno_gpe3d_error refuses."""
    return _solve_error_batch_nd(psi0, (x, y, z), dt, t_final, order, g, kappa, V, group, rec_every, device,
                                 MAX_LAUNCHES_3D)
