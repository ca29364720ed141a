"""NIOFP3D_FNO on the HIP device (needs a GPU) against the float64 checker tests/nio3d_fno_ref.py,
which encodes every drawn snapshot (repeats included) and writes the bag mean literally, while the
device runs each distinct snapshot once, weighted by multiplicity / L, with the projection and the
mean at bag level (ops.BagEncoder3dFn) or, with ops.BAG3D_STATS off, as FNO3dFn + BagMeanFn.

Bars (those of tests/test_gpu_nio3d.py): output <= 1e-5, every gradient <= 1e-4.
"""
import numpy as np
import pytest
import torch

from conftest import load_golden, rel_l2

import nio3d_fno_ref
from test_nio3d_fno_golden import golden_ctor, golden_state

pytestmark = pytest.mark.gpu

FWD_BAR, GRAD_BAR = 1e-5, 1e-4


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    import blindno
    blindno.load_library()


def _grid(shape):
    ax = [torch.linspace(-1, 1, n) for n in shape]
    return torch.stack(torch.meshgrid(*ax, indexing="ij"), -1).contiguous()


def _golden_case():
    g = load_golden("nio3d_fno_train")
    st, x = golden_state(g)
    return dict(ctor=golden_ctor(g), kw={}, st=st, x=torch.from_numpy(x), grid=torch.from_numpy(g["in.grid"]),
                idx=g["idx"], cot=torch.from_numpy(g["cot"]))


def _repeats_case():
    """51 draws out of 12 distinct snapshots on an odd grid, other widths and a one-channel head."""
    import blindno
    torch.manual_seed(5)
    ctor, kw = (2, 5, 3, 1), {"input_modes": 2}
    m = blindno.NIOFP3D_FNO(*ctor, "cpu", **kw)
    st = {k: v.detach().numpy() for k, v in m.state_dict().items()}
    x = torch.randn(1, 60, 5, 9, 6)
    idx = np.random.RandomState(4).choice(12, 51)
    assert len(np.unique(idx)) < len(idx)
    return dict(ctor=ctor, kw=kw, st=st, x=x, grid=_grid((5, 9, 6)), idx=idx, cot=torch.randn(1, 5, 9, 6, 1))


_CASES = {"golden": _golden_case, "repeats": _repeats_case}
_REF = {}


def reference(name):
    """(case, float64 output, {name: float64 gradient}) -- computed once per case, never changed."""
    if name not in _REF:
        c = _CASES[name]()
        p = nio3d_fno_ref.leaves(c["st"])
        y = nio3d_fno_ref.niofp3d_fno(p, c["x"].double(), c["grid"].double(), idx=c["idx"].tolist())
        (y * c["cot"].double()).sum().backward()
        _REF[name] = (c, y.detach(), {k: v.grad for k, v in p.items()})
    return _REF[name]


def device_run(c, bag_level):
    import blindno
    from blindno import ops
    m = blindno.NIOFP3D_FNO(*c["ctor"], "cuda", **c["kw"])
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in c["st"].items()}, strict=True)
    m = m.cuda().train()
    old = ops.BAG3D_STATS
    ops.BAG3D_STATS = bag_level
    try:
        out = m(c["x"].cuda(), c["grid"].cuda(), bag_idx=c["idx"])
        (out * c["cot"].cuda()).sum().backward()
        torch.cuda.synchronize()
    finally:
        ops.BAG3D_STATS = old
    return m, out


@pytest.mark.parametrize("bag_level", [True, False], ids=["bag_level", "fallback"])
@pytest.mark.parametrize("name", ["golden", "repeats"])
def test_matches_fp64_checker(name, bag_level, monkeypatch):
    from blindno import ops
    c, y, grads = reference(name)
    calls = []
    real = ops.call
    monkeypatch.setattr(ops, "call", lambda n, *a: (calls.append(n), real(n, *a))[1])
    m, out = device_run(c, bag_level)
    # the path asked for is the path taken
    assert ("blindno_project_bag3d_fwd" in calls) == bag_level
    assert ("blindno_project_bag3d_bwd" in calls) == bag_level
    assert tuple(out.shape) == tuple(y.shape)
    e = rel_l2(out.detach().cpu().numpy(), y.numpy())
    worst = (0.0, "")
    for k, p in m.named_parameters():
        if k.startswith("fc0."):
            assert p.grad is None, k                      # fc0 enters as .data
            assert grads[k] is None
            continue
        got, ref = p.grad, grads[k]
        if got.is_complex():
            got, ref = torch.view_as_real(got), torch.view_as_real(ref)
        worst = max(worst, (rel_l2(got.cpu().numpy(), ref.numpy()), k))
    print(f"{name} bag_level={bag_level}: fwd {e:.2e}, worst gradient {worst[0]:.2e} ({worst[1]})")
    assert e <= FWD_BAR, e
    assert worst[0] <= GRAD_BAR, worst


def test_train_draw_is_the_references():
    """Without bag_idx, train mode draws the bag from numpy's global RNG as the reference does:
    seeded as the golden was, the draw is the golden's (L, idx)."""
    import blindno
    g = load_golden("nio3d_fno_train")
    c, _, _ = reference("golden")
    np.random.seed(int(g["bag_seed"]))
    L, idx = blindno.draw_bag(c["x"].shape[1])
    assert L == int(g["L"]) and np.array_equal(idx, g["idx"])
    m, _ = device_run(c, True)
    x, grid = c["x"].cuda(), c["grid"].cuda()
    with torch.no_grad():
        np.random.seed(int(g["bag_seed"]))
        a = m(x, grid)
        b = m(x, grid, bag_idx=g["idx"])
        b2 = m(x, grid, bag_idx=g["idx"])
    assert torch.equal(a, b)
    assert torch.equal(b, b2)                             # bag_idx= reproduces a run


def test_eval_uses_every_snapshot_and_shapes_are_validated():
    c, _, _ = reference("golden")
    m, _ = device_run(c, True)
    m.eval()
    x, grid = c["x"].cuda(), c["grid"].cuda()
    with torch.no_grad():
        a = m(x, grid)
        b = m(x, grid, bag_idx=np.arange(x.shape[1]))
        part = m(x, grid, bag_idx=np.arange(x.shape[1] - 1))
    assert a.shape == (2, 7, 6, 5, 2) and torch.isfinite(a).all()
    assert torch.equal(a, b)                              # L = T
    assert not torch.equal(a, part)
    with pytest.raises(ValueError, match="expected x"):
        m(x, grid[..., :2])
    with pytest.raises(ValueError, match="expected x"):
        m(x[:, :, 0], grid)


def test_fpe_3d_dataset_trains_niofp3d_fno():
    """End to end on a 10^3 grid, which Encoder3D (depth 33-64) cannot take: fpe_3d_dataset ->
    TrajectoryDataset3D -> a few FlatAdam steps with the train-mode bag draw."""
    import blindno
    from blindno import data, datagen, ops
    from blindno.train import FlatAdam, trained_parameters
    NM = 1e-9
    np.random.seed(21)
    d = datagen.fpe_3d_dataset(M=2, nsteps=60, extent=100 * NM)
    assert d["trajectories"].shape == (2, 60, 10, 10, 10)
    X, Y = data.device_tensors(data.TrajectoryDataset3D(arrays=d))
    assert X.shape == (2, 60, 10, 10, 10) and Y.shape == (2, 10, 10, 10, 2)
    with pytest.raises(ValueError, match="does not reduce to one voxel"):
        blindno.Encoder3D(25)(torch.zeros(1, 2, 1, 10, 10, 10))
    torch.manual_seed(0)
    m = blindno.NIOFP3D_FNO(2, 6, 3, 2, "cuda", input_modes=2).cuda().train()
    grid = _grid((10, 10, 10)).cuda()
    opt = FlatAdam(trained_parameters(m, exclude_prefixes=("fc0.",)), lr=2e-3)
    fixed = np.arange(60)

    def loss_on_fixed_bag():
        with torch.no_grad():
            return float(ops.MSEFn.apply(m(X, grid, bag_idx=fixed), Y, None))

    before = loss_on_fixed_bag()
    fc0 = m.fc0.weight.detach().clone()
    for _ in range(8):
        opt.zero_grad()
        loss = ops.MSEFn.apply(m(X, grid), Y, None)       # the train-mode draw, deduplicated
        loss.backward()
        assert bool(torch.isfinite(loss))
        opt.step()
    after = loss_on_fixed_bag()
    print(f"NIOFP3D_FNO on fpe_3d_dataset 10^3: loss {before:.5f} -> {after:.5f}")
    assert np.isfinite(before) and np.isfinite(after) and after < before
    assert torch.equal(fc0, m.fc0.weight.detach()) and m.fc0.weight.grad is None
