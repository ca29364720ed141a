"""Transolver2D and NIOFP2D_Trans on the GPU against the float64 restatement
tests/transolver_ref.py, the deduplicated bag against the bag with its duplicates kept, and two
steps of the trainer's ``2d_FPE --model trans`` experiment.

Bar of the comparisons with float64: rel-L2 <= max(1e-5, 3 x e32), e32 the error of the same
restatement run in fp32 on the CPU against float64 on the same inputs and parameters.
"""
import os

import numpy as np
import pytest
import torch

import transolver_ref as tr

pytestmark = pytest.mark.gpu


def rel(a, b):
    a, b = a.detach().double().cpu().reshape(-1), b.detach().double().cpu().reshape(-1)
    den = float(torch.linalg.vector_norm(b))
    return float(torch.linalg.vector_norm(a - b)) / (den if den > 0 else 1.0)


def _spread_parameters(module, seed):
    """Parameters at which every path of the model matters (the reference's initialisation, std
    0.02, leaves the attention's contribution far below the bars): fan-in scaled weights, LayerNorm
    gains around 1, small biases, four different temperatures."""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for name, p in module.named_parameters():
            if name.endswith("temperature"):
                p.copy_(torch.tensor([0.5, 0.3, 0.8, 1.2]).view(1, 4, 1, 1))
            elif p.dim() >= 2:
                p.copy_(torch.randn(p.shape, generator=g) * (1.5 / (p[0].numel() ** 0.5)))
            elif ".ln_" in name and name.endswith("weight"):
                p.copy_(1.0 + 0.3 * torch.randn(p.shape, generator=g))
            else:
                p.copy_(0.1 * torch.randn(p.shape, generator=g))


def _ref_transolver(sd, inp, H, W, dy, dt):
    p = {k: v.detach().to(dt).clone().requires_grad_(True) for k, v in sd.items()}
    y = tr.transolver(p, inp.to(dt), H, W)
    (y * dy.to(dt)).sum().backward()
    return y.detach(), {k: v.grad for k, v in p.items() if v.grad is not None}


@pytest.mark.parametrize("H,W", [(9, 13), (61, 61)])
def test_transolver_against_float64(H, W):
    import blindno
    S, N = 3, H * W
    torch.manual_seed(5)
    m = blindno.Transolver2D(H=H, W=W)
    _spread_parameters(m, 11)
    g = torch.Generator().manual_seed(H)
    inp = torch.randn(S, 3, N, generator=g)
    dy = torch.randn(S, 1, N, generator=g)
    sd = {k: v for k, v in m.state_dict().items()}
    y64, g64 = _ref_transolver(sd, inp, H, W, dy, torch.float64)
    y32, g32 = _ref_transolver(sd, inp, H, W, dy, torch.float32)
    assert "placeholder" not in g64 and len(g64) == 68
    m = m.cuda()
    y = m.forward_planes(inp.view(S, 3, H, W).cuda())
    (y * dy.view(S, 1, H, W).cuda()).sum().backward()
    e, bar = rel(y.reshape(S, 1, N), y64), max(1e-5, 3 * rel(y32, y64))
    print(f"{H}x{W} forward rel-L2 {e:.2e} bar {bar:.2e}")
    bad = [("y", e, bar)] if e > bar else []
    for k, p in m.named_parameters():
        if k == "placeholder":
            assert p.grad is None
            continue
        e, bar = rel(p.grad, g64[k]), max(1e-5, 3 * rel(g32[k], g64[k]))
        print(f"{H}x{W} {k:40s} rel-L2 {e:.2e} bar {bar:.2e}")
        if e > bar:
            bad.append((k, e, bar))
    assert not bad, bad
    # the reference's (S, N, C) signature gives the same numbers
    x_pts, fx_pts = inp[:, :1].transpose(1, 2).cuda(), inp[:, 1:].transpose(1, 2).cuda()
    with torch.no_grad():
        y2 = m(x_pts, fx_pts)
    assert torch.equal(y2.reshape(-1), y.detach().reshape(-1))


def _grid():
    ax = np.linspace(-1, 1, 61, dtype=np.float32)
    gx, gy = np.meshgrid(ax, ax, indexing="ij")
    return torch.from_numpy(np.stack([gx, gy], 2))


def test_model_against_float64_and_dedup():
    """NIOFP2D_Trans on a draw with duplicates: against the float64 restatement, and the
    deduplicated path against the same model run with the duplicates kept (equal up to the order
    of the bag sum, so the same bar)."""
    import blindno
    from blindno import nio
    torch.manual_seed(2)
    m = blindno.NIOFP2D_Trans(2, 3, 100, 25, 2, 6, 8, 2)
    _spread_parameters(m.trans_input, 21)
    g = torch.Generator().manual_seed(9)
    x = torch.randn(1, 12, 61, 61, generator=g)
    cot = torch.randn(1, 61, 61, 2, generator=g)
    grid = _grid()
    idx = [3, 7, 3, 0, 11, 7, 3, 5]
    sd = {k: v.detach().clone() for k, v in m.state_dict().items()}

    def reference(dt):
        p = {k: (v.to(dt) if v.is_floating_point() else v).clone().requires_grad_(v.is_floating_point())
             for k, v in sd.items()}
        h = tr.trans_bag_field(p, x, grid, idx, dt=dt)
        (h * hcot.to(dt)).sum().backward()
        return h.detach(), {k: v.grad for k, v in p.items() if v.grad is not None}

    m = m.cuda().train()
    xd, gd = x.cuda(), grid.cuda()
    # the encoder's field (what the heads read) is compared with float64; the heads have their own tests
    hcot = torch.randn(1, 61, 61, 6, generator=g)
    h64, g64 = reference(torch.float64)
    h32, g32 = reference(torch.float32)

    def encoder(dedup):
        nio.DEDUP_BAGS = dedup
        try:
            m.zero_grad(set_to_none=True)
            xs, L, lw = nio._select(m, xd, idx, dedup=True)
            assert (L, lw is not None) == ((5, True) if dedup else (8, False))
            B = xs.shape[0]
            gp = gd.permute(2, 0, 1).unsqueeze(0).expand(B * L, 2, 61, 61)
            u = m.trans_input.forward_planes(torch.cat((xs.reshape(B * L, 1, 61, 61), gp), 1))
            h = nio._bag_mean_2d(m, u, gd, B, L, 61, 61, lw)
            (h * hcot.cuda()).sum().backward()
            return h.detach(), {k: p.grad.clone() for k, p in m.named_parameters() if p.grad is not None}
        finally:
            nio.DEDUP_BAGS = True
    hd, gdd = encoder(True)
    hk, gk = encoder(False)
    bad = []
    for name, got, want, fp32 in [("h", hd, h64, h32)] + [(k, gdd[k], g64[k], g32[k]) for k in sorted(gdd)]:
        e, bar = rel(got, want), max(1e-5, 3 * rel(fp32, want))
        print(f"dedup vs float64 {name:50s} rel-L2 {e:.2e} bar {bar:.2e}")
        if e > bar:
            bad.append((name, e, bar))
    assert sorted(gdd) == sorted(gk) == sorted(g64) and len(gdd) == 68
    for name, got, want, fp32 in [("h", hd, hk, h32)] + [(k, gdd[k], gk[k], g32[k]) for k in sorted(gdd)]:
        ref64 = h64 if name == "h" else g64[name]
        e, bar = rel(got, want), max(1e-5, 3 * rel(fp32, ref64))
        print(f"dedup vs kept    {name:50s} rel-L2 {e:.2e} bar {bar:.2e}")
        if e > bar:
            bad.append(("kept:" + name, e, bar))
    assert not bad, bad
    # the module's own forward, deduplicated against duplicates kept: output and every gradient,
    # under the bars of the encoder comparison above (the heads are the same launches in both)
    def whole(dedup):
        nio.DEDUP_BAGS = dedup
        try:
            m.zero_grad(set_to_none=True)
            out = m(xd, gd, bag_idx=idx)
            (out * cot.cuda()).sum().backward()
            return out.detach(), {k: p.grad.clone() for k, p in m.named_parameters() if p.grad is not None}
        finally:
            nio.DEDUP_BAGS = True
    od, wd = whole(True)
    ok, wk = whole(False)
    assert tuple(od.shape) == (1, 61, 61, 2) and torch.isfinite(od).all()
    assert sorted(wd) == sorted(wk)
    e = rel(od, ok)
    print(f"model dedup vs kept: out rel-L2 {e:.2e}")
    assert e <= max(1e-5, 3 * rel(h32, h64)), e
    for k in sorted(wd):
        e = rel(wd[k], wk[k])
        bar = max(1e-5, 3 * rel(g32[k], g64[k])) if k in g64 else 1e-5
        print(f"model dedup vs kept {k:50s} rel-L2 {e:.2e} bar {bar:.2e}")
        if e > bar:
            bad.append(("model:" + k, e, bar))
    assert not bad, bad
    for k, p in m.named_parameters():
        unused = k.startswith(("branch.", "fc0.")) or k == "trans_input.placeholder"
        assert (k not in wd) == unused, k
    with pytest.raises(ValueError, match="61 x 61"):
        m(torch.zeros(1, 60, 24, 24, device="cuda"), torch.zeros(24, 24, 2, device="cuda"))


def test_model_against_reference_golden():
    """NIOFP2D_Trans on the GPU against the reference's own fp32 run (nio2d_trans_train.npz), under
    the bars of tests/test_transolver_ref.py::test_golden_model_restatement."""
    import blindno
    from test_transolver_ref import G_TOL, OUT_TOL, golden_case
    from conftest import rel_l2
    g, st, x = golden_case()
    m = blindno.NIOFP2D_Trans(2, 3, 100, 25, 2, 6, 8, 2)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in st.items()}, strict=True)
    m = m.cuda().train()
    out = m(torch.from_numpy(x).cuda(), torch.from_numpy(g["in.grid"]).cuda(), bag_idx=g["idx"])
    (out * torch.from_numpy(g["cot"]).cuda()).sum().backward()
    e = rel_l2(out.detach().cpu().numpy(), g["out"])
    print(f"output rel-L2 {e:.2e} (bar {OUT_TOL})")
    assert e <= OUT_TOL
    grads = {k: p.grad for k, p in m.named_parameters()}
    worst = (None, 0.0)
    for k, v in g.items():
        if k.startswith("g."):
            assert grads[k[2:]] is not None, k
            e = rel_l2(grads[k[2:]].cpu().numpy(), v)
            worst = max(worst, (k, e), key=lambda t: t[1])
            assert e <= G_TOL, (k, e)
    print(f"worst gradient {worst[0]} rel-L2 {worst[1]:.2e} (bar {G_TOL})")
    for k, gr in grads.items():
        assert (gr is None) == ("g." + k not in g), k


def test_trainer_two_steps(tmp_path):
    from blindno import trainer
    rs = np.random.RandomState(0)
    n, T = 5, 52
    path = os.path.join(tmp_path, "tiny.npz")
    np.savez(path, trajectories=(1e-10 * rs.rand(n, T, 61, 61)).astype(np.float32),
             potential=(1e-21 * rs.randn(n, 61, 61)).astype(np.float32),
             drag=(1e-6 * rs.rand(n, 61, 61)).astype(np.float32))
    exp = trainer.experiments_for("trans")["2d_FPE"]
    t = trainer.Trainer(exp, path, os.path.join(tmp_path, "out"), torch.device("cuda", 0), epochs=1, batch=2,
                        log=lambda s: None)
    before = {k: v.detach().clone() for k, v in t.model.state_dict().items()}
    loss = t.train_epoch(1)                   # 4 train samples, batch 2: two eager steps
    assert np.isfinite(loss)
    after = t.model.state_dict()
    changed = 0
    for k, v in before.items():
        frozen = k.startswith(("branch.", "fc0.")) or k == "trans_input.placeholder"
        if frozen:
            assert torch.equal(v, after[k]), k
        elif v.is_floating_point() and not torch.equal(v, after[k]):
            changed += 1
    assert changed >= 68, changed
