"""NIOFP2D_Trans_attn on the GPU: against the reference's own fp32 run (nio2d_trans_attn_train.npz),
against the float64 restatement tests/trans_attn_ref.py in train and eval mode, the deduplicated bag
against the bag with its duplicates kept, the numpy draw, and one epoch of the trainer's
``2d_FPE --model trans_attn`` experiment.

Bars: OUT_TOL = 1e-4 / G_TOL = 1e-3 for the model (tests/test_transolver_ref.py: the bars under
which the reference's fp32 run sits against float64, which a second fp32 implementation of the same
model can be held to), FWD_TOL = 1e-5 / GRAD_TOL = 1e-4 (tests/test_gpu_parity.py) for the
deduplicated run against the run with duplicates kept, whose encoder launches compute the same
numbers and whose attention differs only in the order of its sums.
"""
import os

import numpy as np
import pytest
import torch

import trans_attn_ref as R
from conftest import rel_l2
from test_gpu_parity import FWD_TOL, GRAD_TOL
from test_gpu_trans import _grid, _spread_parameters
from test_trans_attn_ref import G_TOL, OUT_TOL, golden_case

pytestmark = pytest.mark.gpu

UNUSED = ("branch.", "fc0.")


def _unused(k):
    return k.startswith(UNUSED) or k == "trans_input.placeholder"


def _golden_model():
    import blindno
    g, st, x = golden_case()
    m = blindno.NIOFP2D_Trans_attn(2, 3, 100, 25, 2, 6, 8, 2, 61, 61)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in st.items()}, strict=True)
    return g, m.cuda().train(), torch.from_numpy(x).cuda(), torch.from_numpy(g["in.grid"]).cuda()


def test_model_against_reference_golden():
    g, m, x, grid = _golden_model()
    out = m(x, grid, bag_idx=g["idx"])
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


def test_numpy_draw_matches_reference():
    """Without bag_idx the train-mode draw consumes numpy's global RNG like the reference
    (randint(50, T), choice(T, L) with replacement): the golden's seed gives the golden's output."""
    g, m, x, grid = _golden_model()
    np.random.seed(int(g["bag_seed"]))
    with torch.no_grad():
        out = m(x, grid)
    assert rel_l2(out.cpu().numpy(), g["out"]) <= OUT_TOL
    with pytest.raises(ValueError, match="host index list"):
        m(x, grid, bag_idx=torch.as_tensor(g["idx"]).cuda())


def _model_and_ref(train, T, idx, B, seed):
    """(model on the GPU, outputs and gradients of the GPU run and of the float64 restatement)."""
    import blindno
    torch.manual_seed(seed)
    m = blindno.NIOFP2D_Trans_attn(2, 3, 100, 25, 2, 6, 8, 2, 61, 61)
    _spread_parameters(m.trans_input, 21)
    gen = torch.Generator().manual_seed(seed + 1)
    x = torch.randn(B, T, 61, 61, generator=gen)
    cot = torch.randn(B, 61, 61, 2, generator=gen)
    grid = _grid()
    p = {k: (v.detach().double() if v.is_floating_point() else v.detach()).clone()
         .requires_grad_(v.is_floating_point()) for k, v in m.state_dict().items()}
    gref = grid.double().requires_grad_(True)
    ref = R.niofp2d_trans_attn(p, x, gref, idx=idx)
    (ref * cot.double()).sum().backward()
    m = m.cuda().train(train)
    gd = grid.cuda().requires_grad_(True)
    return m, x.cuda(), gd, cot.cuda(), ref.detach(), p, gref


def _check(m, out, gd, ref, p, gref):
    e = rel_l2(out.detach().cpu().numpy(), ref.numpy())
    print(f"output rel-L2 {e:.2e} (bar {OUT_TOL})")
    assert e <= OUT_TOL
    n = 0
    for k, prm in m.named_parameters():
        if _unused(k):
            assert prm.grad is None and p[k].grad is None, k
            continue
        assert p[k].grad is not None and prm.grad is not None, k
        e = rel_l2(prm.grad.cpu().numpy(), p[k].grad.numpy())
        assert e <= G_TOL, (k, e)
        n += 1
    assert n == 96
    e = rel_l2(gd.grad.cpu().numpy(), gref.grad.numpy())
    print(f"grid gradient rel-L2 {e:.2e} (bar {G_TOL})")
    assert e <= G_TOL


def test_train_mode_against_float64_and_duplicates_kept(monkeypatch):
    from blindno import nio
    idx = np.random.RandomState(3).choice(52, 51)
    assert len(set(idx.tolist())) < 51
    m, x, gd, cot, ref, p, gref = _model_and_ref(True, 52, idx.tolist(), 2, 4)
    out = m(x, gd, bag_idx=idx)
    (out * cot).sum().backward()
    _check(m, out, gd, ref, p, gref)
    dedup = {k: q.grad.clone() for k, q in m.named_parameters() if q.grad is not None}
    dedup["grid"] = gd.grad.clone()
    # the same step with every duplicate kept as a token of its own
    monkeypatch.setattr(nio, "DEDUP_BAGS", False)
    m.zero_grad(set_to_none=True)
    gd.grad = None
    out2 = m(x, gd, bag_idx=idx)
    (out2 * cot).sum().backward()
    e = rel_l2(out.detach().cpu().numpy(), out2.detach().cpu().numpy())
    print(f"dedup vs kept: out rel-L2 {e:.2e}")
    assert e <= FWD_TOL
    kept = {k: q.grad for k, q in m.named_parameters() if q.grad is not None}
    kept["grid"] = gd.grad
    assert sorted(kept) == sorted(dedup)
    for k in sorted(kept):
        e = rel_l2(dedup[k].cpu().numpy(), kept[k].cpu().numpy())
        assert e <= GRAD_TOL, (k, e)


def test_eval_mode_against_float64():
    m, x, gd, cot, ref, p, gref = _model_and_ref(False, 5, None, 2, 6)
    out = m(x, gd)
    (out * cot).sum().backward()
    _check(m, out, gd, ref, p, gref)


def test_trainer_one_epoch(tmp_path):
    from blindno import trainer
    rs = np.random.RandomState(0)
    n, T = 5, 52
    path = os.path.join(tmp_path, "tiny.npz")
    np.savez(path, trajectories=(1e-10 * rs.rand(n, T, 61, 61)).astype(np.float32),
             potential=(1e-21 * rs.randn(n, 61, 61)).astype(np.float32),
             drag=(1e-6 * rs.rand(n, 61, 61)).astype(np.float32))
    exp = trainer.experiments_for("trans_attn")["2d_FPE"]
    t = trainer.Trainer(exp, path, os.path.join(tmp_path, "out"), torch.device("cuda", 0), epochs=1, batch=2,
                        log=lambda s: None)
    assert type(t.model).__name__ == "NIOFP2D_Trans_attn"
    before = {k: v.detach().clone() for k, v in t.model.state_dict().items()}
    loss = t.train_epoch(1)                   # 4 train samples, batch 2: two eager steps
    assert np.isfinite(loss)
    after = t.model.state_dict()
    changed = 0
    for k, v in before.items():
        if _unused(k):
            assert torch.equal(v, after[k]), k
        elif v.is_floating_point() and not torch.equal(v, after[k]):
            changed += 1
    assert changed >= 68, changed
