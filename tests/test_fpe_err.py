"""The record-free Fokker-Planck error path without a GPU: the scratch query of
include/blindno_fpe_err.h, the launch plan and budgets of blindno.fpe.propagate_error_many, the 3d_FPE kind of blindno.evaluate
against data.TrajectoryDataset3D, and the 3d_FPE trainer experiment's configuration.
"""

import numpy as np
import pytest

from fpe3d_ref import initial, make_sim


def test_fpe_err_scratch_query_without_a_device():
    """The host-only size query: the density, two iterates and two partials per tile; -1 when
    refused."""
    from blindno import _lib
    q = lambda *a: _lib.query("blindno_fp_error_nd_scratch_doubles", *a)   # noqa: E731
    assert q(6, 40, 40, 40) == 3 * 6 * 64000 + 2 * 6 * 250
    assert q(1, 5, 4, 3) == 3 * 60 + 2 and q(2, 7, 6, 7) == 2 * (3 * 294 + 2 * 2)
    assert q(600, 2048, 2048, 1) == 600 * (3 * 2048 * 2048 + 2 * 16384) > 2 ** 32
    for bad in [(0, 4, 4, 4), (1, 0, 4, 4), (1, 4, 0, 4), (1, 4, 4, 0), (1, 1 << 20, 1 << 20, 1 << 20),
                (1, 2 ** 31 - 1, 2 ** 31 - 1, 2 ** 31 - 1)]:
        assert q(*bad) == -1, bad


def test_launch_plan_keeps_groups_whole_and_merges_equal_counts():
    from blindno import fpe
    plan = fpe.error_launch_plan([2, 5, 3, 1, 1, 1, 4, 5, 5, 2, 2, 2], 3, 10)
    # groups 0 and 2 need 5 (their members' maximum), group 1 needs 1, group 3 needs 2
    assert plan == [(1, [1]), (2, [3]), (5, [0, 2])]
    assert sorted(g for _, gs in plan for g in gs) == [0, 1, 2, 3]           # every group exactly once
    assert fpe.error_launch_plan([7, 7, 7, 7], 1, 4) == [(7, [0, 1, 2, 3])]    # equal counts: one launch
    assert fpe.error_launch_plan([1, 9, 2, 3], 4, 4) == [(9, [0])]             # one group of the whole batch
    assert fpe.error_launch_plan([3, 1, 2, 2], 2, 1) == [(2, [1]), (3, [0])]   # no interval: still planned
    for steps, group in [([1, 2, 3], 2), ([1, 2], 0), ([], 1), ([1, 2, 3, 4], 3)]:
        with pytest.raises(fpe.BlindnoError, match="whole groups"):
            fpe.error_launch_plan(steps, group, 4)


def test_launch_plan_budgets():
    """MAX_TOTAL_SUBSTEPS on the stiffest trajectory; MAX_TOTAL_PASSES_ND over the DISTINCT group
    substep counts (members below their group's maximum add no launch)."""
    from blindno import fpe
    n = 11                                                         # 10 intervals
    with pytest.raises(fpe.BlindnoError, match=r"Taylor substeps.*refusing to launch"):
        fpe.error_launch_plan([1, fpe.MAX_TOTAL_SUBSTEPS // 10 + 1], 2, n)
    cap = fpe.MAX_TOTAL_PASSES_ND // (10 * fpe.TAYLOR_DEGREE)      # substeps per interval inside the budget
    assert fpe.error_launch_plan([cap, 1, cap, cap - 1], 2, n) == [(cap, [0, 1])]
    with pytest.raises(fpe.BlindnoError, match=r"passes.*refusing to launch"):
        fpe.error_launch_plan([cap + 1, 1], 2, n)
    with pytest.raises(fpe.BlindnoError, match=r"passes.*refusing to launch"):
        fpe.error_launch_plan([cap, 1, 1, 1], 2, n)                # two distinct counts: cap + 1
    assert fpe.error_launch_plan([cap + 1, 1], 2, n, degree=1) == [(cap + 1, [0])]


def test_over_budget_requests_are_refused_without_a_device():
    """propagate_error_many raises both refusals before anything touches the device (device='cpu'
    raises the no-CPU-path error next) -- on a 2D grid too, which propagate_many would hand to the
    one-launch LDS kernel: the error path is always grid-resident."""
    from blindno import fpe
    for dims in [(5, 4, 3), (5, 4, 1)]:
        sims = [make_sim(dims, (False, False, False), k) for k in range(2)]
        p0 = [initial(s, k) for k, s in enumerate(sims)]
        per = max(fpe.substeps_for(s.coefficients_nd(), 1.0) for s in sims)    # substeps per second
        want = fpe.MAX_TOTAL_PASSES_ND // (2 * fpe.TAYLOR_DEGREE) + 2          # per interval, 2 intervals
        tf = 2 * want / per
        with pytest.raises(fpe.BlindnoError, match=r"passes.*refusing to launch"):
            fpe.propagate_error_many(sims, p0, tf, Nsteps=3, group=2, device="cpu")
        with pytest.raises(fpe.BlindnoError, match="no CPU path"):             # just inside the budget
            fpe.propagate_error_many(sims, p0, tf / 2.2, Nsteps=3, group=2, device="cpu")
        with pytest.raises(fpe.BlindnoError, match=r"Taylor substeps.*refusing to launch"):
            fpe.propagate_error_many(sims, p0, 2.0 * fpe.MAX_TOTAL_SUBSTEPS / per, Nsteps=3, group=2, device="cpu")
        with pytest.raises(fpe.BlindnoError, match="whole groups"):
            fpe.propagate_error_many(sims + sims[:1], p0 + p0[:1], tf / 2.2, Nsteps=3, group=2, device="cpu")


def _dict3d(M=3, T=5, S=(4, 4, 4), seed=5):
    rs = np.random.RandomState(seed)
    return dict(trajectories=rs.rand(M, T, *S) * 1e-10, potential=rs.randn(M, *S) * 1e-21,
                drag=rs.rand(M, *S) * 1e-6 + 1e-6)


def test_evaluate_3d_fpe_matches_trajectory_dataset_3d():
    """Kind 3d_FPE: the statistics, the input normalisation and the de-normalisation of the targets
    are data.TrajectoryDataset3D's (trajectories x 1e10, potential x 1e21, drag x 1e6, z-scored
    over axis 0), on a 3-sample 4^3 dict."""
    from blindno import data, evaluate as ev
    d = _dict3d()
    ds = data.TrajectoryDataset3D(arrays=d)
    st = ev.compute_train_stats("3d_FPE", d)
    assert ev.KINDS["3d_FPE"]["fields"] == ("drift", "diffusion")
    assert np.array_equal(st["traj_mean"], ds.trajectories_mean) and np.array_equal(st["traj_std"], ds.trajectories_std)
    assert np.array_equal(st["drift_mean"], ds.potential_mean) and np.array_equal(st["drift_std"], ds.potential_std)
    assert np.array_equal(st["diff_mean"], ds.drag_mean) and np.array_equal(st["diff_std"], ds.drag_std)
    for i in range(3):
        x = ev.normalize_input(np.array(d["trajectories"][i], dtype=np.float32), st)
        assert x.shape == (5, 4, 4, 4) and np.array_equal(x, ds.trajectories[i])
        y = ds[i][1].numpy()                                       # the normalised targets (4, 4, 4, 2)
        pa, pb = ev.denormalize("3d_FPE", y, st)
        ta, tb = ev.true_fields("3d_FPE", d, i, st)
        assert pa.shape == pb.shape == (4, 4, 4)
        assert np.array_equal(pa, ta) and np.array_equal(pb, tb)   # the same float32 sequence
        # the round trip returns the raw fields to float32 rounding: with m the largest |value| of
        # the field, |raw s - mu| <= 2 m s, and the six float32 operations (x s, - mu, / sd, x sd,
        # + mu, / s) each round a value of at most 2 m s: 1 + 2 + 2 + 2 + 1 <= 8 eps m
        for got, key in ((pa, "potential"), (pb, "drag")):
            raw = np.array(d[key][i], dtype=np.float32)
            assert np.abs(got - raw).max() <= 8 * np.finfo(np.float32).eps * np.abs(np.array(d[key], np.float32)).max()


def test_trainer_3d_fpe_experiment_configuration():
    from blindno import data, trainer
    exps = trainer._experiments("fno")
    e = exps["3d_FPE"]
    assert "3d_FPE" not in trainer._experiments("unet") and "3d_FPE" not in trainer._experiments("nio")
    assert (e.dim, e.dataset, e.lr, e.batch, e.save_interval, e.result_dir) == \
        (3, data.TrajectoryDataset3D, 5e-4, 4, 5, "results_3d_FPE_fno")
    assert e.two_channel_metric and e.eager
    assert tuple(e.loss_files) == ("train_losses", "test_losses", "test_losses_drift", "test_losses_diffusion")
    # every other experiment keeps the graphed step
    for m in ("fno", "unet", "nio"):
        assert all(not x.eager for k, x in trainer._experiments(m).items() if k != "3d_FPE")
    assert trainer.Experiment.__dataclass_fields__["eager"].default is False


def test_eager_experiment_refuses_a_world_above_one(tmp_path, monkeypatch):
    """An eager experiment has no data-parallel path: the Trainer raises before any collective (the
    world size is read first; nothing else of torch.distributed is touched)."""
    import torch
    import torch.distributed as dist
    from blindno import trainer
    monkeypatch.setattr(dist, "is_initialized", lambda: True)
    monkeypatch.setattr(dist, "get_world_size", lambda *a: 2)
    monkeypatch.setattr(dist, "get_rank", lambda *a: 1)
    for name in ("broadcast", "all_reduce", "barrier"):
        monkeypatch.setattr(dist, name, lambda *a, **k: pytest.fail("a collective ran"))
    with pytest.raises(ValueError, match="one process"):
        trainer.Trainer(trainer._experiments()["3d_FPE"], str(tmp_path / "absent.npz"), str(tmp_path / "o"),
                        torch.device("cpu"), epochs=1)
