"""NIOFP2D_Trans (2d_FPE/NIOModules.py:85-166) without a GPU: the state_dict layout against the
reference's (tests/golden/layouts_trans.json, written by make_golden_trans.py), the float64
restatement tests/transolver_ref.py against torch.nn.functional's own layers, both drop-in shims,
the trainer's table and the C ABI binding of include/blindno_physattn.h.

The kernels themselves are compared with the restatement on the GPU (tests/test_gpu_physattn.py,
tests/test_gpu_trans.py).
"""
import json
import os
import subprocess
import sys

import pytest
import torch
import torch.nn.functional as F

import numpy as np

import transolver_ref as tr
from conftest import GOLDEN, ROOT, load_golden, rel_l2
from recipe import make_array

OUT_TOL, G_TOL = 1e-4, 1e-3          # the bars of tests/test_nio2d_attn.py

DROPIN = os.path.join(ROOT, "dropin")
CTOR = (2, 3, 100, 25, 3, 12, 32, 2)


def golden_case():
    """(golden arrays, recipe state with the generator's rescaling, x) of nio2d_trans_train."""
    g = load_golden("nio2d_trans_train")
    shapes = [(k, tuple(sh)) for k, sh in json.loads(str(g["layout_json"]))]
    st = tr.rescaled_state(shapes, int(g["recipe_seed"]), json.loads(str(g["rescale_json"])))
    x = make_array(tuple(int(n) for n in g["x_shape"]), int(g["recipe_seed"]), "nio2d_trans.x")
    return g, st, x


def test_golden_model_restatement():
    """transolver_ref.niofp2d_trans against the reference's own fp32 run (61^2, one bag, 51 recorded
    draws with replacement from 52 snapshots): output and every stored gradient."""
    g, st, x = golden_case()
    idx = g["idx"].tolist()
    assert tuple(g["x_shape"]) == (1, 52, 61, 61) and len(idx) == int(g["L"]) == 51
    assert len(set(idx)) < len(idx)                       # the draw holds a duplicate
    assert os.path.getsize(os.path.join(GOLDEN, "nio2d_trans_train.npz")) <= \
        os.path.getsize(os.path.join(GOLDEN, "nio2d_fno_attn_train.npz"))
    p = {k: torch.from_numpy(v).double().requires_grad_(v.dtype.kind == "f") for k, v in st.items()}
    grid = torch.from_numpy(g["in.grid"]).double()
    rec = []
    y = tr.niofp2d_trans(p, torch.from_numpy(x), grid, idx=idx, record=rec)
    e = rel_l2(y.detach().numpy(), g["out"])
    print(f"output rel-L2 {e:.2e}")
    assert e <= OUT_TOL
    (y * torch.from_numpy(g["cot"]).double()).sum().backward()
    n = 0
    for k, v in g.items():
        if k.startswith("g."):
            assert p[k[2:]].grad is not None, k
            assert rel_l2(p[k[2:]].grad.numpy(), v) <= G_TOL, k
            n += 1
    assert n == 96 and sum(k.startswith("g.trans_input.") for k in g) == 68
    assert not any(k.startswith(("g.branch.", "g.fc0.")) or k == "g.trans_input.placeholder" for k in g)
    for k, q in p.items():                                # and nothing else has a gradient
        if k.startswith(("branch.", "fc0.")) or k == "trans_input.placeholder":
            assert q.grad is None, k
    # anti-hiding: the slices are not near-uniform, and uniform slice weights move the output by
    # at least 10 x the forward bar
    rowmax = float(np.mean([float(w.max(2).values.mean()) for w in rec]))
    assert abs(rowmax - float(g["w_rowmax_mean"])) <= 1e-4 and rowmax > 2 / 16
    with torch.no_grad():
        yu = tr.niofp2d_trans(p, torch.from_numpy(x), grid, idx=idx, uniform=True)
    move = rel_l2(yu.numpy(), y.detach().numpy())
    print(f"mean row max {rowmax:.3f}; uniform slices move the output by {move:.2e}")
    assert move >= 10 * OUT_TOL


def test_state_dict_layout_matches_reference():
    import blindno
    lay = json.load(open(os.path.join(GOLDEN, "layouts_trans.json")))
    for key, kernel in (("2d_FPE", (2, 1)), ("2d_NC", (3, 2))):
        m = blindno.NIOFP2D_Trans(*CTOR, branch_last_kernel=kernel)
        got = [[k, list(v.shape), str(v.dtype).replace("torch.", "")] for k, v in m.state_dict().items()]
        want = lay[f"{key}.NIOFP2D_Trans(2,3,100,25,3,12,32,2)"]
        assert got == want
        trans = [k for k, _, _ in want if k.startswith("trans_input.")]
        assert len(trans) == 69 and trans[0] == "trans_input.placeholder"
        assert any(k.startswith("branch.") for k, _, _ in want)
        assert {"fno_drift.fc0.weight", "fno_diffusion.fc0.weight"} <= {k for k, _, _ in want}


def test_initialisation_follows_the_reference():
    import blindno
    torch.manual_seed(3)
    t = blindno.Transolver2D(H=9, W=13)
    a = t.blocks[0].Attn
    assert torch.all(a.temperature == 0.5) and tuple(a.temperature.shape) == (1, 4, 1, 1)
    for name, p in t.named_parameters():
        if name.endswith("bias") and "in_project_x" not in name and "in_project_fx" not in name:
            assert torch.all(p == 0), name
    # Model.apply's truncated normal reaches every Linear, in_project_slice included
    # (an orthogonal (16, 8) weight has unit columns; std 0.02 gives column norms near 0.08)
    assert float(a.in_project_slice.weight.detach().norm(dim=0).max()) < 0.3
    assert float(t.preprocess.linear_pre[0].weight.detach().std()) < 0.03
    assert 0 <= float(t.placeholder.detach().min()) and float(t.placeholder.detach().max()) <= 1 / 32
    with pytest.raises(ValueError):
        blindno.Transolver2D(Time_Input=True)
    with pytest.raises(ValueError):
        blindno.Transolver2D(unified_pos=1)
    with pytest.raises(ValueError):
        t(torch.zeros(1, 117, 1), None)
    with pytest.raises(ValueError, match="heads = 4"):
        blindno.Transolver2D(n_head=8)
    with pytest.raises(ValueError, match="heads = 4"):
        blindno.Transolver2D(slice_num=32)


def test_restatement_against_torch_layers():
    """transolver_ref's pieces against torch.nn.functional in float64: the LayerNorm, the GELU and
    the physics attention written as the reference composes it (softmax / einsum / matmul on
    (S, heads, N, C) tensors)."""
    g = torch.Generator().manual_seed(2)
    S, H, W = 2, 5, 7
    N = H * W
    r = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)  # noqa: E731
    x = r(S, 32, N)
    ga, be = r(32), r(32)
    want = F.layer_norm(x.transpose(1, 2), (32,), ga, be, 1e-5).transpose(1, 2)
    assert float((tr.layer_norm(x, ga, be) - want).abs().max()) < 1e-12
    assert float((tr._gelu(x) - F.gelu(x)).abs().max()) < 1e-13
    xm, fm = r(S, 32, N), r(S, 32, N)
    T = torch.tensor([0.05, 0.4, 0.7, 7.0], dtype=torch.float64)
    Ws, bs, Wq, Wk, Wv, Wo, bo = r(16, 8), r(16), r(8, 8), r(8, 8), r(8, 8), r(32, 32), r(32)
    got = tr.phys_attn(xm, fm, T, Ws, bs, Wq, Wk, Wv, Wo, bo)["y"]
    x_mid = xm.transpose(1, 2).reshape(S, N, 4, 8).permute(0, 2, 1, 3)
    fx_mid = fm.transpose(1, 2).reshape(S, N, 4, 8).permute(0, 2, 1, 3)
    sw = torch.softmax(F.linear(x_mid, Ws, bs) / torch.clamp(T.view(1, 4, 1, 1), min=0.1, max=5), -1)
    tok = torch.einsum("bhnc,bhng->bhgc", fx_mid, sw) / (sw.sum(2) + 1e-5)[:, :, :, None]
    q, k, v = F.linear(tok, Wq), F.linear(tok, Wk), F.linear(tok, Wv)
    ot = torch.softmax(q @ k.transpose(-1, -2) * 8 ** -0.5, -1) @ v
    ox = torch.einsum("bhgc,bhng->bhnc", ot, sw).permute(0, 2, 1, 3).reshape(S, N, 32)
    want = F.linear(ox, Wo, bo).transpose(1, 2)
    assert float((got - want).abs().max()) < 1e-11


def _run(code, exp):
    env = dict(os.environ, PYTHONDONTWRITEBYTECODE="1")
    return subprocess.run([sys.executable, "-c",
                           f"import sys; sys.path.insert(0, {os.path.join(DROPIN, exp)!r})\n" + code],
                          capture_output=True, text=True, env=env, timeout=240)


@pytest.mark.parametrize("exp,kernel", [("2d_FPE", [2, 1]), ("2d_Non_conservative_FPE", [3, 2])])
def test_dropin_shims_serve_the_class(exp, kernel):
    r = _run("from NIOModules import NIOFP2D_Trans, NIOFP2D_Trans_attn\n"
             "m = NIOFP2D_Trans(2,3,100,25,3,12,32,2)\n"
             "print(type(m).__mro__[1].__name__, sorted(n for n, _ in m.named_children()),"
             " list(m.branch.convblock7_3.layers[0].kernel_size))\n"
             "try:\n    NIOFP2D_Trans_attn(2,3,100,25,3,12,32,2)\n"
             "except NotImplementedError as e:\n    print('RAISES', 'SURVEY' in str(e))\n", exp)
    assert r.returncode == 0, r.stderr
    names = sorted(["branch", "fc0", "trans_input", "fno_drift", "fno_diffusion"])
    assert r.stdout.strip().splitlines() == [f"NIOFP2D_Trans {names} {kernel}", "RAISES True"], (r.stdout, r.stderr)


def test_trainer_lists_the_experiment():
    from blindno import trainer
    exps = trainer.experiments_for("trans")
    assert "2d_FPE" in exps and "2d_FPE" in trainer._experiments("unet")
    e, u = exps["2d_FPE"], trainer._experiments("unet")["2d_FPE"]
    assert e.eager and (e.lr, e.batch, e.save_interval) == (u.lr, u.batch, u.save_interval)
    assert e.result_dir == "results_2d_FPE_trans"
    # _experiments keeps its tables: it does not know "trans" (an unknown model name falls through
    # to the NIO-FNO table), and the new entry is reachable through _own_experiments alone
    keys = {"fno": ["1d_FPE", "1d_GPE", "2d_FPE", "2d_GPE", "2d_Non_conservative_FPE", "3d_FPE"],
            "unet": ["1d_FPE", "1d_GPE", "2d_FPE", "2d_Non_conservative_FPE"],
            "nio": ["1d_FPE", "1d_GPE", "2d_FPE", "2d_Non_conservative_FPE"]}
    for model, want in keys.items():
        assert sorted(trainer._experiments(model)) == want, model
    assert trainer._experiments("trans")["2d_FPE"].result_dir == "result_2d_fno"
    assert sorted(trainer._own_experiments("trans")) == ["2d_FPE"]
    assert trainer._own_experiments("trans")["2d_FPE"] is not None and trainer._own_experiments("fno") == {}
    assert sorted(trainer._own_experiments("unet")) == ["3d_FPE"]


def test_grid_other_than_61_is_refused(monkeypatch):
    import blindno
    from blindno import ops
    monkeypatch.setattr(ops, "require_device", lambda *a: None)
    m = blindno.NIOFP2D_Trans(2, 2, 8, 3, 1, 2, 2, 2)
    with pytest.raises(ValueError, match="61 x 61"):
        m(torch.zeros(1, 60, 24, 24), torch.zeros(24, 24, 2))


def test_physattn_queries_without_a_device():
    from blindno import _lib
    q = _lib.query
    assert q("blindno_physattn_ok", 300, 61, 61, 4, 8, 16) == 1
    assert q("blindno_physattn_ok", 300, 61, 61, 8, 8, 16) == 0
    assert q("blindno_physattn_nblk", 61, 61) == 15 and q("blindno_ln_planes_nblk", 3721) == 15
    assert q("blindno_physattn_fwd_scratch_floats", 300, 61, 61) == 300 * 4 * 15 * 144
    assert q("blindno_physattn_bwd_scratch_floats", 2, 61, 61) == \
        2 * 32 * 3721 + 2 * 4 * 15 * 144 + 2 * 15 * 1056 + 2 * 4 * (128 + 16 + 192) + 2 * 15 * 148
    assert q("blindno_physattn_fwd_scratch_floats", 0, 61, 61) == -1
