"""Density-trajectory errors of predicted fields: 2d_Non_conservative_FPE/
compute_time_error.py:361-510 (``compute_time_error``, FPE forces), 1d_FPE/
compute_time_error.py:215-420 (``compute_time_error_1d``, potential + drag) and 1d_GPE/
compute_time_error_GPE.py:208-330 (``compute_time_error_gpe``, GPE potentials; its 2D
and 3D counterparts ``compute_time_error_gpe_2d`` / ``_3d`` are the project's own, as is
``compute_time_error_3d`` for the 3D FPE potential + drag field), each as one batched pipeline.

Per test index the reference normalises the bag with the train statistics, predicts (Fx, Fy)
with each model, de-normalises, propagates a Gaussian density (centre (-150, -150) nm, width
30 nm) under the true and under each predicted force with fplanck (``propagate_density_with_
force``, :300-319), and writes ``[index, model, rel_l2_Fx, rel_l2_Fy, ErrL2_density]`` to
metrics_all.csv, ErrL2 being ``time_averaged_relative_l2`` (:321-333).

Here every model's forward runs batched on the HIP path (blindno.evaluate.predict) and ALL
density propagations -- the reference one and one per model, for every index -- go into ONE
``blindno_fp_propagate`` launch (one workgroup per trajectory).  The propagator restates the
absent fplanck (blindno.fpe): parity UNPINNED.  The figures are out of scope.
"""
from __future__ import annotations

import csv
import os
from typing import Dict, Iterable, List, Optional

import numpy as np
import torch

from . import evaluate, fpe

NM = 1e-9
KIND = "2d_Non_conservative_FPE"


def time_averaged_relative_l2(pt_pred: np.ndarray, pt_ref: np.ndarray, eps: float = 1e-12) -> float:
    """compute_time_error.py:321-333: mean over t of ||P_pred[t] - P_ref[t]|| / (||P_ref[t]|| + eps)."""
    a = pt_pred.reshape(pt_pred.shape[0], -1)
    b = pt_ref.reshape(pt_ref.shape[0], -1)
    return float(np.mean(np.linalg.norm(a - b, axis=1) / (np.linalg.norm(b, axis=1) + eps)))


def build_fokker_planck(force, temperature=300.0, viscosity=8e-4, radius_nm=50.0, extent_nm=800.0,
                        resolution_nm=10.0):
    """compute_time_error.py:266-286."""
    drag = 6 * np.pi * viscosity * radius_nm * NM
    return fpe.fokker_planck(temperature=temperature, drag=drag, extent=[extent_nm * NM, extent_nm * NM],
                             resolution=resolution_nm * NM, boundary=fpe.boundary.reflecting, force=force)


def force_from_array(grid, Fx, Fy):
    """compute_time_error.py:288-298."""
    fx, fy = fpe.potential_from_data(grid, Fx), fpe.potential_from_data(grid, Fy)
    return lambda x, y: np.array([fx(x, y), fy(x, y)])


def compute_time_error(models: Dict[str, torch.nn.Module], train, test, indices: Iterable[int],
                       outdir: Optional[str] = None, nsteps: int = 500, dt: float = 10e-3,
                       batch: int = 8, device="cuda", **phys) -> List[list]:
    """Rows [index, model, rel_l2_Fx, rel_l2_Fy, ErrL2_density] in the reference's order (per
    index: the models in the given order); with ``outdir`` appended to metrics_all.csv."""
    stats = evaluate.compute_train_stats(KIND, train)
    data = np.load(test) if isinstance(test, str) else test
    traj = np.asarray(data["trajectories"])
    idx = [i for i in indices if 0 <= i < traj.shape[0]]
    if not idx:
        return []
    nx, ny = traj.shape[2], traj.shape[3]
    x = torch.tensor(np.stack([evaluate.normalize_input(np.array(traj[i], dtype=np.float32), stats)
                               for i in idx]), dtype=torch.float32, device=device)
    grid_t = evaluate.grid2d(nx, ny, device)
    preds = {name: evaluate.predict(m, x, grid_t, batch).cpu().numpy() for name, m in models.items()}
    grid = build_fokker_planck(lambda xx, yy: np.array([0 * xx, 0 * yy]), **phys).grid
    pdf = fpe.gaussian_pdf(center=(-150 * NM, -150 * NM), width=30 * NM)
    sims, fields = [], []
    for k, i in enumerate(idx):
        F = np.array(data["F"][i], dtype=np.float32)
        sims.append(build_fokker_planck(force_from_array(grid, F[0], F[1]), **phys))
        for name in models:
            pa, pb = evaluate.denormalize(KIND, preds[name][k], stats)
            fields.append((i, name, evaluate.rel_l2(pa, F[0]), evaluate.rel_l2(pb, F[1])))
            sims.append(build_fokker_planck(force_from_array(grid, pa, pb), **phys))
    res = fpe.propagate_many(sims, [pdf] * len(sims), dt, Nsteps=nsteps, device=device)
    rows = []
    per = 1 + len(models)
    for k in range(len(idx)):
        ref = res[k * per][1]
        for j in range(len(models)):
            i, name, rfx, rfy = fields[k * len(models) + j]
            rows.append([i, name, rfx, rfy, time_averaged_relative_l2(res[k * per + 1 + j][1], ref)])
    if outdir is not None:
        os.makedirs(outdir, exist_ok=True)
        path = os.path.join(outdir, "metrics_all.csv")
        header = not os.path.exists(path)
        with open(path, "a", newline="") as f:
            w = csv.writer(f)
            if header:
                w.writerow(["index", "model", "rel_l2_Fx", "rel_l2_Fy", "ErrL2_density"])
            w.writerows(rows)
    return rows


# ------------------------------------------------------------------------------- 1D GPE
def compute_time_error_gpe(models: Dict[str, torch.nn.Module], train, test, indices: Iterable[int],
                           outdir: Optional[str] = None, order: int = 2, dt: float = 0.005,
                           t_final: float = 5.0, init_ic: int = 2, batch: int = 32,
                           device="cuda") -> Dict[str, np.ndarray]:
    """1d_GPE/compute_time_error_GPE.py:208-330: per test index, V predicted by each model
    (de-normalised with the train V_max), |psi| propagated from initial condition ``init_ic`` on
    x = linspace(-10, 10, Nx) under the true V and under each prediction (true g, kappa), and
    time_averaged_L2_error of the densities.  All trajectories -- reference and every model's,
    for every index -- run in ONE blindno_gpe_solve launch; the errors' spatial integrals run on
    the GPU (blindno.gpe.time_averaged_L2_error).  Returns {model: errors in index order}; with
    ``outdir`` writes the reference's per-sample dicts <outdir>/<model>/sample_<idx>_V_and_err.npy
    and ErrL2_relative_<model>_Nsamples_<n>.npy."""
    from . import gpe
    sc = evaluate.compute_train_scalers_gpe(train)
    tn = evaluate.normalize_gpe(test, sc)
    y = np.asarray(tn["y"])
    idx = [int(i) for i in indices if 0 <= int(i) < y.shape[0]]
    if not idx:
        return {name: np.zeros(0) for name in models}
    nx = y.shape[2]
    xin = torch.tensor(np.stack([y[i] for i in idx]), dtype=torch.float32, device=device)
    grid_n = torch.linspace(0.0, 1.0, nx, device=device).unsqueeze(-1)
    preds = {}
    for name, m in models.items():
        p = evaluate.predict(m, xin, grid_n, batch).cpu().numpy()
        preds[name] = (p[..., 0] if p.ndim == 3 else p) * sc["V_max"]
    x = np.linspace(-10, 10, nx)
    V, g, kappa = [], [], []
    for k, i in enumerate(idx):
        gi = float(np.atleast_1d(test["g"][i])[0])
        ki = float(np.atleast_1d(test["kappa"][i])[0])
        for Vi in [tn["V"][i] * sc["V_max"]] + [preds[name][k] for name in models]:
            V.append(Vi)
            g.append(gi)
            kappa.append(ki)
    r = gpe.solve_batch(gpe.initial_condition(init_ic, x), x, dt, t_final, order, np.array(g),
                        np.array(kappa), np.array(V), rec_every=1, device=device)
    t, rho = r["t"], r["abs"]
    per = 1 + len(models)
    errs = {name: [] for name in models}
    for k, i in enumerate(idx):
        ref = rho[k * per]
        for j, name in enumerate(models):
            e = gpe.time_averaged_L2_error(t, ref, t, rho[k * per + 1 + j], x)
            errs[name].append(e)
            if outdir is not None:
                d = os.path.join(outdir, name)
                os.makedirs(d, exist_ok=True)
                np.save(os.path.join(d, f"sample_{i}_V_and_err.npy"),
                        {"x": x, "true_V": V[k * per], "pred_V": V[k * per + 1 + j], "g": g[k * per],
                         "kappa": kappa[k * per], "Err_L2_rel": e})
    out = {name: np.array(v, dtype=float) for name, v in errs.items()}
    if outdir is not None:
        for name, arr in out.items():
            np.save(os.path.join(outdir, f"ErrL2_relative_{name}_Nsamples_{len(idx)}.npy"), arr)
    return out


# ------------------------------------------------------------------------------- 2D GPE
def compute_time_error_gpe_2d(models: Dict[str, torch.nn.Module], train, test, indices: Iterable[int],
                              outdir: Optional[str] = None, order: int = 2, dt: float = 0.005,
                              t_final: float = 5.0, init_ic: int = 2, batch: int = 4, rec_every: int = 10,
                              device="cuda", record_free: bool = False) -> Dict[str, np.ndarray]:
    """The 2D counterpart of ``compute_time_error_gpe`` for the 2d_GPE experiment (the
    project's own; ``train`` / ``test`` are blindno.gpe.generate_training_data_2d dicts): per
    test index, V predicted by each model (de-normalised with the train V_max), |psi| propagated
    from psi0 = ic(x) ic(y) on [-10, 10]^2 under the true V and under each prediction (true g,
    kappa), and time_averaged_L2_error_2d of the densities.  All trajectories -- reference and
    every model's, for every index -- run in ONE blindno.gpe.solve_batch_2d call, recording every
    ``rec_every``-th step (a full 256^2 record of 1001 frames is 0.5 GB per trajectory; the call
    refuses a record above gpe.MAX_RECORD_BYTES).  Returns {model: errors in index order}; with
    ``outdir`` writes <outdir>/<model>/sample_<idx>_V_and_err.npy and
    ErrL2_relative_<model>_Nsamples_<n>.npy as the 1D function does (x and y in the dict).

    With ``record_free=True`` no |psi| record exists: the trajectories go through
    blindno.gpe.solve_error_batch_2d with group = 1 + len(models), in chunks of whole groups whose
    scratch (three doubles per cell and trajectory, whatever the number of frames) stays under
    gpe.MAX_RECORD_BYTES, and the two integrals per frame come back from the device.  The same
    integrator and the same per-cell terms, summed in another order: the errors agree with the
    recorded path's to 4 N 2^-53 relative (N cells), and test sets whose record the one recorded
    call refuses can be evaluated.  The returned dict and the files are the same."""
    from . import gpe
    sc = evaluate.compute_train_scalers_gpe(train)
    tn = evaluate.normalize_gpe(test, sc)
    yy = np.asarray(tn["y"])
    idx = [int(i) for i in indices if 0 <= int(i) < yy.shape[0]]
    if not idx:
        return {name: np.zeros(0) for name in models}
    nx, ny = yy.shape[2], yy.shape[3]
    xin = torch.tensor(np.stack([yy[i] for i in idx]), dtype=torch.float32, device=device)
    grid_n = evaluate.grid2d(nx, ny, device)
    preds = {}
    for name, m in models.items():
        p = evaluate.predict(m, xin, grid_n, batch).cpu().numpy()
        preds[name] = (p[..., 0] if p.ndim == 4 else p) * sc["V_max"]
    x = np.linspace(-10, 10, nx)
    y = np.linspace(-10, 10, ny)
    V, g, kappa = [], [], []
    for k, i in enumerate(idx):
        gi = float(np.atleast_1d(test["g"][i])[0])
        ki = float(np.atleast_1d(test["kappa"][i])[0])
        for Vi in [tn["V"][i] * sc["V_max"]] + [preds[name][k] for name in models]:
            V.append(Vi)
            g.append(gi)
            kappa.append(ki)
    psi0 = gpe.initial_condition(init_ic, x)[:, None] * gpe.initial_condition(init_ic, y)[None, :]
    per = 1 + len(models)
    if record_free:
        free = _gpe_errors_record_free(psi0, (x, y), dt, t_final, order, g, kappa, V, per, rec_every, device)
    else:
        r = gpe.solve_batch_2d(psi0, x, y, dt, t_final, order, np.array(g), np.array(kappa), np.array(V),
                               rec_every=rec_every, device=device)
        t, rho = r["t"], r["abs"]
    errs = {name: [] for name in models}
    for k, i in enumerate(idx):
        if not record_free:
            ref = rho[k * per]
        for j, name in enumerate(models):
            if record_free:
                e = free[k * per + 1 + j]
            else:
                e = gpe.time_averaged_L2_error_2d(t, ref, t, rho[k * per + 1 + j], (x, y))
            errs[name].append(e)
            if outdir is not None:
                d = os.path.join(outdir, name)
                os.makedirs(d, exist_ok=True)
                np.save(os.path.join(d, f"sample_{i}_V_and_err.npy"),
                        {"x": x, "y": y, "true_V": V[k * per], "pred_V": V[k * per + 1 + j], "g": g[k * per],
                         "kappa": kappa[k * per], "Err_L2_rel": e})
    out = {name: np.array(v, dtype=float) for name, v in errs.items()}
    if outdir is not None:
        for name, arr in out.items():
            np.save(os.path.join(outdir, f"ErrL2_relative_{name}_Nsamples_{len(idx)}.npy"), arr)
    return out


# ------------------------------------------------------------------------------- 3D GPE
def grid3d(nx: int, ny: int, nz: int, device) -> torch.Tensor:
    """The (Nx, Ny, Nz, 3) grid on [-1, 1]^3 the 3D models read (evaluate.grid2d with one more axis)."""
    g = np.meshgrid(*(np.linspace(-1, 1, n, dtype=np.float32) for n in (nx, ny, nz)), indexing="ij")
    return torch.tensor(np.stack(g, axis=3), device=device)


def _gpe_errors_record_free(psi0, grids, dt, t_final, order, g, kappa, V, per, rec_every, device) -> List[float]:
    """time_averaged_L2_error_2d / _3d (by the number of ``grids``) of every trajectory against its
    group's first (groups of ``per`` consecutive trajectories), through
    blindno.gpe.solve_error_batch_2d / _3d in chunks of whole groups that keep the scratch under
    gpe.MAX_RECORD_BYTES."""
    from . import gpe
    from ._lib import query
    dim = f"{len(grids)}d"
    shape = tuple(len(a) for a in grids)
    on = " x ".join(str(n) for n in shape)
    group_bytes = 8 * query(f"blindno_gpe{dim}_error_scratch_doubles", per, *shape)
    if group_bytes < 0:
        raise gpe.BlindnoError(f"the {dim.upper()} solver refuses a {on} grid")
    fit = int(gpe.MAX_RECORD_BYTES // group_bytes)            # groups per call (the scratch is linear in B)
    if fit < 1:
        raise gpe.BlindnoError(
            f"the scratch of one group of {per} trajectories on the {on} grid ({group_bytes} bytes) is "
            f"above MAX_RECORD_BYTES = {gpe.MAX_RECORD_BYTES}")
    solve = getattr(gpe, f"solve_error_batch_{dim}")
    out = []
    for s in range(0, len(V), fit * per):
        e = slice(s, s + fit * per)
        r = solve(psi0, *grids, dt, t_final, order, np.array(g[e]), np.array(kappa[e]), np.array(V[e]), group=per,
                  rec_every=rec_every, device=device)
        out += [gpe.time_averaged_L2_error_from_sums(r["t"], r["num"][b], r["den"][b]) for b in range(r["num"].shape[0])]
    return out


def compute_time_error_gpe_3d(models: Dict[str, torch.nn.Module], train, test, indices: Iterable[int],
                              outdir: Optional[str] = None, order: int = 2, dt: float = 0.005,
                              t_final: float = 5.0, init_ic: int = 2, batch: int = 2, rec_every: int = 10,
                              device="cuda", record_free: bool = False) -> Dict[str, np.ndarray]:
    """``compute_time_error_gpe_2d`` with the 3D solver and error (``train`` / ``test`` are
    blindno.gpe.generate_training_data_3d dicts; the models map x (B, T, Nx, Ny, Nz) and a
    (Nx, Ny, Nz, 3) grid to V, e.g. NIOFP3D_FNO(..., output_dim=1)): per test index, V predicted by
    each model (de-normalised with the train V_max), |psi| propagated from psi0 = ic(x) ic(y) ic(z)
    on [-10, 10]^3 under the true V and under each prediction (true g, kappa), and
    time_averaged_L2_error_3d of the densities.  All trajectories -- reference and every model's,
    for every index -- go into blindno.gpe.solve_batch_3d calls, each of as many trajectories (whole
    indices where one fits) as keep its fp64 |psi| record, every ``rec_every``-th step, under
    gpe.MAX_RECORD_BYTES; the solver is independent of the batch bit for bit, so the chunking does
    not change a digit.  Returns {model: errors in index order}; with ``outdir`` writes
    <outdir>/<model>/sample_<idx>_V_and_err.npy and ErrL2_relative_<model>_Nsamples_<n>.npy as the
    2D function does (x, y and z in the dict).

    With ``record_free=True`` no |psi| record exists: the trajectories go through
    blindno.gpe.solve_error_batch_3d with group = 1 + len(models), in chunks of whole groups whose
    scratch (three doubles per cell and trajectory, whatever the number of frames) stays under
    gpe.MAX_RECORD_BYTES, and the two integrals per frame come back from the device.  The same
    integrator and the same per-cell terms, summed in another order: the errors agree with the
    recorded path's to 4 N 2^-53 relative (N cells), and grids whose record the recorded path refuses
    can be evaluated.  The returned dict and the files are the same."""
    from . import gpe
    sc = evaluate.compute_train_scalers_gpe(train)
    tn = evaluate.normalize_gpe(test, sc)
    yy = np.asarray(tn["y"])
    idx = [int(i) for i in indices if 0 <= int(i) < yy.shape[0]]
    if not idx:
        return {name: np.zeros(0) for name in models}
    nx, ny, nz = yy.shape[2:5]
    xin = torch.tensor(np.stack([yy[i] for i in idx]), dtype=torch.float32, device=device)
    grid_n = grid3d(nx, ny, nz, device)
    preds = {}
    for name, m in models.items():
        p = evaluate.predict(m, xin, grid_n, batch).cpu().numpy()
        preds[name] = (p[..., 0] if p.ndim == 5 else p) * sc["V_max"]
    x, y, z = (np.linspace(-10, 10, n) for n in (nx, ny, nz))
    V, g, kappa = [], [], []
    for k, i in enumerate(idx):
        gi = float(np.atleast_1d(test["g"][i])[0])
        ki = float(np.atleast_1d(test["kappa"][i])[0])
        for Vi in [tn["V"][i] * sc["V_max"]] + [preds[name][k] for name in models]:
            V.append(Vi)
            g.append(gi)
            kappa.append(ki)
    psi0 = (gpe.initial_condition(init_ic, x)[:, None, None] * gpe.initial_condition(init_ic, y)[None, :, None] *
            gpe.initial_condition(init_ic, z)[None, None, :])
    per = 1 + len(models)
    errs = {name: [] for name in models}
    t, rho, base = None, None, 0
    if record_free:
        free = _gpe_errors_record_free(psi0, (x, y, z), dt, t_final, order, g, kappa, V, per, rec_every, device)
    else:
        nrec = (int(t_final / dt)) // int(rec_every) + 1
        traj_bytes = nrec * nx * ny * nz * 8
        fit = int(gpe.MAX_RECORD_BYTES // traj_bytes)             # trajectories per call
        if fit < 1:
            raise gpe.BlindnoError(
                f"one trajectory's record ({traj_bytes} bytes) is above MAX_RECORD_BYTES = {gpe.MAX_RECORD_BYTES}; "
                "raise rec_every")
        chunk = fit // per * per if fit >= per else fit           # whole indices where one fits

    def traj(n):
        """|psi| record of trajectory n: its chunk is solved when first needed, one chunk resident."""
        nonlocal t, rho, base
        if rho is None or not base <= n < base + rho.shape[0]:
            rho = None                                        # free the previous chunk first
            base = n // chunk * chunk
            s = slice(base, base + chunk)
            r = gpe.solve_batch_3d(psi0, x, y, z, dt, t_final, order, np.array(g[s]), np.array(kappa[s]),
                                   np.array(V[s]), rec_every=rec_every, device=device)
            t, rho = r["t"], r["abs"]
        return rho[n - base]

    for k, i in enumerate(idx):
        if not record_free:
            ref = traj(k * per).clone() if chunk % per else traj(k * per)
        for j, name in enumerate(models):
            if record_free:
                e = free[k * per + 1 + j]
            else:
                e = gpe.time_averaged_L2_error_3d(t, ref, t, traj(k * per + 1 + j), (x, y, z))
            errs[name].append(e)
            if outdir is not None:
                d = os.path.join(outdir, name)
                os.makedirs(d, exist_ok=True)
                np.save(os.path.join(d, f"sample_{i}_V_and_err.npy"),
                        {"x": x, "y": y, "z": z, "true_V": V[k * per], "pred_V": V[k * per + 1 + j],
                         "g": g[k * per], "kappa": kappa[k * per], "Err_L2_rel": e})
    out = {name: np.array(v, dtype=float) for name, v in errs.items()}
    if outdir is not None:
        for name, arr in out.items():
            np.save(os.path.join(outdir, f"ErrL2_relative_{name}_Nsamples_{len(idx)}.npy"), arr)
    return out


# ------------------------------------------------------------------------------- 1D FPE
def compute_time_error_1d(models: Dict[str, torch.nn.Module], train, test, indices: Iterable[int],
                          outdir: Optional[str] = None, nsteps: int = 400, dt: float = 2e-3,
                          batch: int = 32, device="cuda", temperature: float = 300.0,
                          extent_nm: float = 800.0, resolution_nm: float = 10.0,
                          init_width_nm: float = 50.0) -> Dict[str, np.ndarray]:
    """1d_FPE/compute_time_error.py:215-420: per test index, (potential, drag) predicted by each
    model (de-normalised with the train statistics, drag = x-mean of the per-point drag), the
    density from a centred Gaussian (width 50 nm) propagated under the true and under each
    predicted (U, drag) (``simulate_density_trajectory``, :215-238), and
    time_averaged_L2_error (:240-295).  All trajectories go into ONE blindno_fp_propagate
    launch.  Returns {model: errors in index order}; with ``outdir`` writes
    <outdir>/<model>/pred_sample_<idx>.npy (Nx, 2) and ErrL2_<model>_Nsamples_<n>.npy."""
    from . import gpe
    stats = evaluate.compute_train_stats_1d(train)
    data = np.load(test) if isinstance(test, str) else test
    traj = np.asarray(data["trajectories"])
    idx = [int(i) for i in indices if 0 <= int(i) < traj.shape[0]]
    if not idx:
        return {name: np.zeros(0) for name in models}
    nx = traj.shape[2]
    xin = torch.tensor(np.stack([evaluate.normalize_input_1d(np.array(traj[i], dtype=np.float32), stats)
                                 for i in idx]), device=device)
    grid_n = torch.linspace(0, 1, nx, device=device).unsqueeze(-1)
    preds = {name: evaluate.predict(m, xin, grid_n, batch).cpu().numpy() for name, m in models.items()}

    def sim(U, drag):
        proto = fpe.fokker_planck(temperature=temperature, drag=drag, extent=extent_nm * NM,
                                  resolution=resolution_nm * NM, boundary=fpe.boundary.reflecting)
        return fpe.fokker_planck(temperature=temperature, drag=drag, extent=extent_nm * NM,
                                 resolution=resolution_nm * NM, boundary=fpe.boundary.reflecting,
                                 potential=fpe.potential_from_data(proto.grid[0], U))
    sims, saved = [], []
    for k, i in enumerate(idx):
        # the reference reads potential / drag as float32 (1d_FPE/compute_time_error.py:112-117)
        sims.append(sim(np.asarray(data["potential"][i], dtype=np.float32).astype(np.float64),
                        float(np.asarray(data["drag"], dtype=np.float32)[i])))
        for name in models:
            pot, drg = evaluate.denormalize_1d(preds[name][k], stats)
            saved.append((name, i, np.stack([pot, drg], axis=1)))
            sims.append(sim(pot, float(drg.mean())))
    pdf = fpe.gaussian_pdf(center=(0 * NM), width=init_width_nm * NM)
    res = fpe.propagate_many(sims, [pdf] * len(sims), dt, Nsteps=nsteps, device=device)
    grid = sims[0].grid
    per = 1 + len(models)
    errs = {name: [] for name in models}
    for k in range(len(idx)):
        t_ref, P_ref = res[k * per]
        for j, name in enumerate(models):
            t_p, P_p = res[k * per + 1 + j]
            errs[name].append(gpe.time_averaged_L2_error(t_ref, P_ref, t_p, P_p, grid))
    if outdir is not None:
        for name, i, arr in saved:
            d = os.path.join(outdir, name)
            os.makedirs(d, exist_ok=True)
            np.save(os.path.join(d, f"pred_sample_{i}.npy"), arr)
    out = {name: np.array(v, dtype=float) for name, v in errs.items()}
    if outdir is not None:
        for name, arr in out.items():
            np.save(os.path.join(outdir, f"ErrL2_{name}_Nsamples_{len(idx)}.npy"), arr)
    return out


# ------------------------------------------------------------------------------- 3D FPE
KIND_3D = "3d_FPE"


def compute_time_error_3d(models: Dict[str, torch.nn.Module], train, test, indices: Iterable[int],
                          outdir: Optional[str] = None, nsteps: int = 400, tf: float = 2e-4, batch: int = 2,
                          device="cuda", temperature: float = 300.0, extent_nm: float = 400.0,
                          resolution_nm: float = 10.0, init_width_nm: float = 50.0) -> List[list]:
    """The density-trajectory error of the 3d_FPE experiment (the project's own; ``train`` / ``test``
    are datagen.fpe_3d_dataset npz files or dicts, the defaults its physics): per test index each
    model predicts (potential, drag field), de-normalised with the train statistics
    (evaluate.denormalize, kind 3d_FPE); a Gaussian at the origin (width 50 nm) is propagated between
    reflecting walls under the true fields and under each prediction, the drag as the per-cell field
    the dataset stores (not its mean).  Every propagation -- the reference and one per model, for
    every index -- goes through fpe.propagate_error_many with group = 1 + len(models): no density
    record exists anywhere (at 40^3 x 400 frames it would be 204.8 MB per trajectory), the two sums
    per frame come back from the device, and ErrL2_density = mean_o sqrt(num_o) / (sqrt(den_o) +
    1e-12) is ``time_averaged_relative_l2`` of ``compute_time_error``.  A prediction whose drag has
    a non-positive or non-finite cell cannot be propagated: its ErrL2_density is NaN (its trajectory
    in the batch is a copy of the reference, so the layout stays whole) and its field errors are
    still reported (evaluate.rel_l2 against the raw float32 fields, as blindno.evaluate reports
    them).  Rows [index, model, rel_l2_potential, rel_l2_drag, ErrL2_density] per index, the models
    in the given order; with ``outdir`` appended to metrics_all.csv."""
    stats = evaluate.compute_train_stats(KIND_3D, train)
    data = np.load(test) if isinstance(test, str) else test
    traj = np.asarray(data["trajectories"])
    idx = [int(i) for i in indices if 0 <= int(i) < traj.shape[0]]
    if not idx:
        return []
    ngrid = (int(np.ceil(extent_nm / resolution_nm)),) * 3
    if ngrid != tuple(traj.shape[2:5]):
        raise fpe.BlindnoError(f"compute_time_error_3d: extent_nm / resolution_nm give a {ngrid} grid, "
                               f"the data is {tuple(traj.shape[2:5])}")
    x = torch.tensor(np.stack([evaluate.normalize_input(np.array(traj[i], dtype=np.float32), stats)
                               for i in idx]), dtype=torch.float32, device=device)
    grid_t = grid3d(*traj.shape[2:5], device)
    preds = {name: evaluate.predict(m, x, grid_t, batch).cpu().numpy() for name, m in models.items()}

    def sim(U, drag):
        U = np.asarray(U, dtype=np.float64)
        return fpe.fokker_planck(temperature=temperature, drag=np.asarray(drag, dtype=np.float64),
                                 extent=[extent_nm * NM] * 3, resolution=resolution_nm * NM,
                                 boundary=fpe.boundary.reflecting, potential=lambda *g: U)
    sims, fields = [], []
    for k, i in enumerate(idx):
        U = np.array(data["potential"][i], dtype=np.float32)
        drag = np.array(data["drag"][i], dtype=np.float32)
        ref = sim(U, drag)
        sims.append(ref)
        for name in models:
            pa, pb = evaluate.denormalize(KIND_3D, preds[name][k], stats)
            ok = bool(np.all(np.isfinite(pb)) and np.all(pb > 0))
            fields.append((i, name, evaluate.rel_l2(pa, U), evaluate.rel_l2(pb, drag), ok))
            sims.append(sim(pa, pb) if ok else ref)
    pdf = fpe.gaussian_pdf(center=(0 * NM, 0 * NM, 0 * NM), width=init_width_nm * NM)
    per = 1 + len(models)
    _, num, den = fpe.propagate_error_many(sims, [pdf] * len(sims), tf, Nsteps=nsteps, group=per, device=device)
    rows = []
    for k in range(len(idx)):
        for j in range(len(models)):
            i, name, rp, rd, ok = fields[k * len(models) + j]
            b = k * per + 1 + j
            e = float(np.mean(np.sqrt(num[b]) / (np.sqrt(den[b]) + 1e-12))) if ok else float("nan")
            rows.append([i, name, rp, rd, e])
    if outdir is not None:
        os.makedirs(outdir, exist_ok=True)
        path = os.path.join(outdir, "metrics_all.csv")
        header = not os.path.exists(path)
        with open(path, "a", newline="") as f:
            w = csv.writer(f)
            if header:
                w.writerow(["index", "model", "rel_l2_potential", "rel_l2_drag", "ErrL2_density"])
            w.writerows(rows)
    return rows
