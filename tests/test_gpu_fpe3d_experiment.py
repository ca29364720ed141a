"""The 3d_FPE experiment end to end on the HIP device (needs a GPU): timeerror.compute_time_error_3d
against the record path (blindno_fp_propagate_nd's frames, numpy norms) on an 8^3 grid with stub
models, and blindno.trainer's eager 3d_FPE experiment for two epochs.
"""
import csv
import math
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

NM = 1e-9
PHYS = dict(extent_nm=80, resolution_nm=10)
NSTEPS, TF = 5, 4e-5


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")


def _dict3d(M, T, seed):
    """A dataset dict on the 8^3 grid of extent 80 nm: fpe_3d_dataset's field shapes (Gaussian wells
    of 1e-20 .. 2e-20 J, a quadratic drag field around 7.5e-10 kg/s) without its propagation."""
    from blindno import datagen
    rs = np.random.RandomState(seed)
    ax = (np.arange(8) - 3.5) * 10 * NM
    g = np.meshgrid(ax, ax, ax, indexing="ij")
    pot, drag = [], []
    for _ in range(M):
        c = rs.uniform(-30 * NM, 30 * NM, size=(2, 3))
        w = rs.uniform(20 * NM, 60 * NM, size=2)
        a = rs.uniform(1e-20, 2e-20, size=2)
        pot.append(sum(-a[j] * np.exp(-sum(((g[d] - c[j, d]) / w[j]) ** 2 for d in range(3))) for j in range(2)))
        dc, vf = rs.uniform(-30 * NM, 30 * NM, size=3), rs.uniform(0, 2)
        drag.append(datagen.DRAG * (1 + vf * sum(((g[d] - dc[d]) / (250 * NM)) ** 2 for d in range(3))))
    traj = rs.rand(M, T, 8, 8, 8)
    traj /= traj.sum(axis=(2, 3, 4), keepdims=True)
    return dict(trajectories=traj, potential=np.array(pot), drag=np.array(drag))


class _Stub(torch.nn.Module):
    """Returns the rows of a fixed (n, 8, 8, 8, 2) prediction in call order."""

    def __init__(self, y):
        super().__init__()
        self.y, self.at = torch.as_tensor(y, dtype=torch.float32), 0

    def forward(self, x, grid):
        assert x.dim() == 5 and tuple(grid.shape) == (8, 8, 8, 3)
        out = self.y[self.at:self.at + x.shape[0]].to(x.device)
        self.at += x.shape[0]
        return out


def _sim(U, drag):
    from blindno import fpe
    U = np.asarray(U, dtype=np.float64)
    return fpe.fokker_planck(temperature=300.0, drag=np.asarray(drag, dtype=np.float64), extent=[80 * NM] * 3,
                             resolution=10 * NM, boundary=fpe.boundary.reflecting, potential=lambda *g: U)


def _record_metric(ref, others):
    """ErrL2_density of each of ``others`` against ``ref`` from blindno_fp_propagate_nd's record, the
    whole group at the largest substep count of its members (what propagate_error_many runs), the
    norms in numpy as compute_time_error takes them."""
    from blindno import fpe, timeerror
    from blindno._lib import call, ptr, query, stream_ptr
    sims = [ref] + list(others)
    pdf = fpe.gaussian_pdf(center=(0.0, 0.0, 0.0), width=50 * NM)
    p0 = np.stack([pdf(*s.grid).reshape(-1) for s in sims])
    p0 /= p0.sum(axis=1, keepdims=True)
    coef = np.stack([s.coefficients_nd() for s in sims])
    dt_out = TF / (NSTEPS - 1)
    s = max(fpe.substeps_for(c, dt_out) for c in coef)
    out = torch.empty(len(sims), NSTEPS, 512, dtype=torch.float64, device="cuda")
    scratch = torch.empty(query("blindno_fp_propagate_nd_scratch_doubles", len(sims), 8, 8, 8), dtype=torch.float64,
                          device="cuda")
    call("blindno_fp_propagate_nd", ptr(torch.from_numpy(p0).cuda()), ptr(torch.from_numpy(coef).cuda()), ptr(out),
         ptr(scratch), len(sims), 8, 8, 8, NSTEPS, s, fpe.TAYLOR_DEGREE, float(dt_out), stream_ptr())
    rec = out.cpu().numpy()
    return [timeerror.time_averaged_relative_l2(rec[k], rec[0]) for k in range(1, len(sims))]


def test_compute_time_error_3d_against_the_record_path(tmp_path):
    _need_gpu()
    from blindno import data, evaluate, fpe, timeerror
    d = _dict3d(4, 6, seed=21)
    idx = [2, 0, 9, 3]                                       # 9 is out of range and skipped
    kept = [2, 0, 3]
    Y = data.TrajectoryDataset3D(arrays=d).targets()[kept]   # the normalised truth (3, 8, 8, 8, 2)
    stats = evaluate.compute_train_stats("3d_FPE", d)
    pert = Y.copy()
    pert[..., 0] *= 1.05
    neg = Y.copy()
    neg[..., 1] = -(stats["diff_mean"] / stats["diff_std"]) - 10.0          # de-normalises to -10 std / 1e6 < 0
    models = {"truth": _Stub(Y), "pert": _Stub(pert), "neg": _Stub(neg)}
    rows = timeerror.compute_time_error_3d(models, d, d, idx, outdir=str(tmp_path), nsteps=NSTEPS, tf=TF, batch=2,
                                           **PHYS)
    assert [(r[0], r[1]) for r in rows] == [(i, m) for i in kept for m in ("truth", "pert", "neg")]
    for k, i in enumerate(kept):
        U = np.array(d["potential"][i], dtype=np.float32)
        drag = np.array(d["drag"][i], dtype=np.float32)
        ta, tb = evaluate.denormalize("3d_FPE", Y[k], stats)
        pa, pb = evaluate.denormalize("3d_FPE", pert[k], stats)
        na, nb = evaluate.denormalize("3d_FPE", neg[k], stats)
        assert (tb > 0).all() and (pb > 0).all() and (nb < 0).all()
        bar_t, bar_p = _record_metric(_sim(U, drag), [_sim(ta, tb), _sim(pa, pb)])
        rt, rp, rn = rows[3 * k:3 * k + 3]
        print(f"index {i}: truth {rt[4]!r} (record {bar_t!r}), perturbed {rp[4]!r} (record {bar_p!r}), "
              f"field errors {rt[2:4]} {rp[2:4]} {rn[2:4]}")
        # the field errors are evaluate.rel_l2 of the de-normalised prediction against the raw fields
        assert rt[2:4] == [evaluate.rel_l2(ta, U), evaluate.rel_l2(tb, drag)]
        assert rp[2:4] == [evaluate.rel_l2(pa, U), evaluate.rel_l2(pb, drag)]
        assert rn[2:4] == [evaluate.rel_l2(na, U), evaluate.rel_l2(nb, drag)]
        # (rel_l2 carries evaluate's eps = 1e-12 in the denominator, far above a potential's norm in
        # joules, so the potential column is small in absolute terms; the order is what is checked)
        assert rt[2] < rp[2] and rt[3] < 1e-6 and rp[3] == rt[3] and rn[2] == rt[2]
        # truth: no more than the float32 round trip of the fields costs on the record path
        assert 0.0 <= rt[4] <= bar_t * (1 + 1e-12) and bar_t < 1e-3 * bar_p
        # perturbed: the record path's value
        assert bar_p > 1e-4 and abs(rp[4] - bar_p) <= 1e-12 * bar_p
        # a negative drag cannot be propagated: NaN, finite field errors
        assert math.isnan(rn[4]) and all(math.isfinite(v) for v in rn[2:4]) and rn[3] > 1
    with open(tmp_path / "metrics_all.csv") as f:
        got = list(csv.reader(f))
    assert got[0] == ["index", "model", "rel_l2_potential", "rel_l2_drag", "ErrL2_density"] and len(got) == 10
    assert [(int(r[0]), r[1]) for r in got[1:]] == [(r[0], r[1]) for r in rows]
    assert [float(r[4]) for r in got[1:] if r[1] != "neg"] == [r[4] for r in rows if r[1] != "neg"]
    # a second call appends without a second header
    for m in models.values():
        m.at = 0
    again = timeerror.compute_time_error_3d(models, d, d, [0], outdir=str(tmp_path), nsteps=NSTEPS, tf=TF, **PHYS)
    assert len(again) == 3 and len(open(tmp_path / "metrics_all.csv").readlines()) == 13
    # a grid that is not the data's is refused
    with pytest.raises(fpe.BlindnoError, match="grid"):
        timeerror.compute_time_error_3d({}, d, d, [0], nsteps=NSTEPS, tf=TF)


def test_propagate_error_many_groups_by_substeps():
    """Groups of different stiffness run in separate launches and land in the caller's order; the
    sums are those of one launch per group at that group's own count."""
    _need_gpu()
    from blindno import fpe
    d = _dict3d(2, 2, seed=4)
    soft = [_sim(d["potential"][0], d["drag"][0]), _sim(1.02 * d["potential"][0], d["drag"][0])]
    stiff = [_sim(d["potential"][1], 0.25 * d["drag"][1]), _sim(d["potential"][1], 0.26 * d["drag"][1])]
    pdf = fpe.gaussian_pdf(center=(0.0, 0.0, 0.0), width=50 * NM)
    dt_out = TF / (NSTEPS - 1)
    s_soft, s_stiff = (max(fpe.substeps_for(s.coefficients_nd(), dt_out) for s in g) for g in (soft, stiff))
    assert s_stiff > 2 * s_soft
    sims = stiff + soft + stiff
    t, num, den = fpe.propagate_error_many(sims, [pdf] * 6, TF, Nsteps=NSTEPS, group=2)
    assert np.array_equal(t, np.linspace(0, TF, NSTEPS)) and num.shape == den.shape == (6, NSTEPS)
    assert (num[0::2] == 0.0).all() and (num[1::2, 1:] > 0).all() and (den > 0).all()
    assert num[:2].tobytes() == num[4:].tobytes() and den[:2].tobytes() == den[4:].tobytes()
    _, n1, d1 = fpe.propagate_error_many(soft, [pdf] * 2, TF, Nsteps=NSTEPS)          # one group: the batch
    assert n1.tobytes() == num[2:4].tobytes() and d1.tobytes() == den[2:4].tobytes()
    assert num[1, 0] == 0.0                                   # the same initial density at t = 0


def test_trainer_3d_fpe_end_to_end(tmp_path):
    """Five 8^3 samples of T = 52 snapshots (draw_bag needs T > 50): the 3d_FPE experiment for two
    epochs at batch 2, evaluating every epoch."""
    _need_gpu()
    from blindno import evaluate, nio, trainer
    from blindno.train import GraphedBagStep, trained_parameters
    d = _dict3d(5, 52, seed=8)
    path = str(tmp_path / "fpe3d.npz")
    np.savez(path, **d)
    out = str(tmp_path / "results_3d_FPE_fno")
    exp = trainer._experiments()["3d_FPE"]
    dev = torch.device("cuda")
    t = trainer.Trainer(exp, path, out, dev, epochs=2, save_interval=1, batch=2, log=lambda s: None)
    assert t.graphed is None and tuple(t.grid.shape) == (8, 8, 8, 3) and isinstance(t.model, nio.NIOFP3D_FNO)
    assert len(t.train_idx) == 4 and len(t.test_idx) == 1
    names = {id(p): k for k, p in t.model.named_parameters()}
    trained = [names[id(p)] for p in trained_parameters(t.model, exclude_prefixes=exp.exclude_prefixes)]
    before = {k: v.detach().clone() for k, v in t.model.state_dict().items()}
    hist = t.fit()
    assert [len(hist[k]) for k in exp.loss_files] == [2, 2, 2, 2]
    assert all(math.isfinite(v) for k in exp.loss_files for v in hist[k])
    assert hist["train_losses"][0] > 0 and hist["train_losses"][1] != hist["train_losses"][0]
    after = t.model.state_dict()
    assert all(k.startswith(("FNO_input.", "fno.")) for k in trained) and len(trained) > 8
    assert all(k in trained for k in before if k.endswith(".weight") and not k.startswith("fc0."))
    moved = [k for k in trained if not torch.equal(before[k], after[k])]
    assert {k.split(".")[0] for k in moved} == {"FNO_input", "fno"}
    assert all(k in moved for k in trained if "weight" in k), sorted(set(trained) - set(moved))
    assert all(torch.equal(before[k], after[k]) for k in before if k.startswith("fc0."))
    best = min(hist["test_losses"])
    ck = f"model_checkpoint_best_{best:.6f}.pt"
    assert sorted(os.listdir(out)) == sorted([ck] + [k + ".npy" for k in exp.loss_files])
    for k in exp.loss_files:
        assert np.array_equal(np.load(os.path.join(out, k + ".npy")), np.array(hist[k]))
    # the checkpoint in a fresh model reproduces the recorded test loss through Trainer.evaluate
    fresh = nio.NIOFP3D_FNO(2, 8, 4, 2, dev, input_modes=4)
    fresh.load_state_dict(evaluate.load_checkpoint_robust(os.path.join(out, ck)), strict=True)
    t.model = fresh.to(dev)
    loss, dr, df = t.evaluate()
    e = int(np.argmin(hist["test_losses"]))
    print(f"test losses {hist['test_losses']}, the checkpoint in a fresh model {loss!r}")
    # the same fp32 forward on the same weights; 1e-6 allows for a different sum order, nothing more
    assert abs(loss - hist["test_losses"][e]) <= 1e-6 * loss and loss == dr + df
    assert abs(dr - hist["test_losses_drift"][e]) <= 1e-6 * dr
    # predict on 5-D outputs
    pred = evaluate.predict(t.model, t.Xte, t.grid, 2)
    assert pred.shape == (1, 8, 8, 8, 2) and bool(torch.isfinite(pred).all())
    # an existing 2D experiment still owns its graphed step
    rs = np.random.RandomState(1)
    d2 = dict(trajectories=rs.rand(5, 52, 61, 61) * 1e-10, potential=rs.randn(5, 61, 61) * 1e-21,
              drag=rs.rand(5, 61, 61) * 1e-6 + 1e-6)
    p2 = str(tmp_path / "fpe2d.npz")
    np.savez(p2, **d2)
    e2 = trainer._experiments()["2d_FPE"]
    t2 = trainer.Trainer(e2, p2, str(tmp_path / "r2"), dev, epochs=1, batch=2, log=lambda s: None)
    assert not e2.eager and isinstance(t2.graphed, GraphedBagStep)

