"""Transolver3D and NIOFP3D_Trans without a GPU: the float64 restatement tests/transolver3d_ref.py
against the reference's own fp32 runs (tests/golden/trans3d_model.npz, nio3d_trans_train.npz,
written by make_golden_trans3d.py), the state_dict layout and the initialisation against the
reference's, the refusals, and the C ABI binding of include/blindno_planemlp.h.

The kernels themselves are compared with the restatement on the GPU (tests/test_gpu_planemlp.py,
tests/test_gpu_trans3d.py).
"""
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import nio3d_ref
import transolver3d_ref as t3
import transolver_ref as tr
from conftest import GOLDEN, load_golden, rel_l2
from recipe import make_array

OUT_TOL, G_TOL = 1e-4, 1e-3          # the bars of tests/test_transolver_ref.py

LAYOUT_KEY = "2d_FPE.Transolver_Structured_Mesh_3D.Model(5,6,7)"


def model_case():
    """(golden arrays, recipe state with the generator's rescaling) of trans3d_model."""
    g = load_golden("trans3d_model")
    shapes = [(k, tuple(sh)) for k, sh in json.loads(str(g["layout_json"]))]
    return g, tr.rescaled_state(shapes, int(g["recipe_seed"]), json.loads(str(g["rescale_json"])))


def nio_case():
    """(golden arrays, recipe state, x) of nio3d_trans_train."""
    g = load_golden("nio3d_trans_train")
    shapes = [(k, tuple(sh)) for k, sh in json.loads(str(g["layout_json"]))]
    st = nio3d_ref.make_state3d(shapes, int(g["recipe_seed"]), json.loads(str(g["complex_json"])))
    for name in st:
        if name.startswith("trans_input."):
            for suffix, f in json.loads(str(g["rescale_json"])).items():
                if name.endswith(suffix):
                    st[name] = (st[name] * np.float32(f)).astype(st[name].dtype)
    x = make_array(tuple(int(n) for n in g["x_shape"]), int(g["recipe_seed"]), "nio3d_trans.x")
    return g, st, x


def test_golden_transolver_restatement():
    """transolver3d_ref.transolver3d against the reference Model's fp32 run on the (5, 6, 7) mesh,
    S = 3: output, both input gradients and one parameter gradient of each kind."""
    g, st = model_case()
    mesh = tuple(int(n) for n in g["mesh"])
    assert mesh == (5, 6, 7) and tuple(g["in.x"].shape) == (3, 210, 3)
    p = {k: torch.from_numpy(v).double().requires_grad_(True) for k, v in st.items()}
    inp = torch.from_numpy(np.concatenate((g["in.x"], g["in.fx"]), -1)).transpose(1, 2).double()
    inp.requires_grad_(True)
    rec = []
    y = t3.transolver3d(p, inp, mesh, record=rec)
    e = rel_l2(y.detach().transpose(1, 2).numpy(), g["out"])
    print(f"output rel-L2 {e:.2e}")
    assert e <= OUT_TOL
    (y * torch.from_numpy(g["cot"]).transpose(1, 2).double()).sum().backward()
    gin = inp.grad.transpose(1, 2).numpy()
    assert rel_l2(gin[..., :3], g["gin.x"]) <= G_TOL and rel_l2(gin[..., 3:], g["gin.fx"]) <= G_TOL
    keys = [k for k in g if k.startswith("g.")]
    assert len(keys) == 20
    for k in keys:
        assert np.any(g[k]), k
        assert rel_l2(p[k[2:]].grad.numpy(), g[k]) <= G_TOL, k
    assert p["placeholder"].grad is None
    # anti-hiding: the slices are not near-uniform, and uniform slice weights move the output by
    # at least 10 x the forward bar
    rowmax = float(np.mean([float(w.max(2).values.mean()) for w in rec]))
    assert abs(rowmax - float(g["w_rowmax_mean"])) <= 1e-4 and rowmax > 2 / 16
    with torch.no_grad():
        yu = t3.transolver3d(p, inp, mesh, uniform=True)
    assert rel_l2(yu.numpy(), y.detach().numpy()) >= 10 * OUT_TOL
    # an axis-order slip shows: the same points read as a (7, 6, 5) mesh give another output
    with torch.no_grad():
        ys = t3.transolver3d(p, inp, mesh[::-1])
    assert rel_l2(ys.numpy(), y.detach().numpy()) >= 10 * OUT_TOL


def test_golden_model_restatement():
    """transolver3d_ref.niofp3d_trans against the composition of the reference's Model, bag-mean
    expression and FNO3d run in its fp32 (grid (7, 6, 5), B = 2, T = 6, a bag of 8 draws with
    repeats): output, loss and every stored gradient."""
    g, st, x = nio_case()
    idx = g["idx"].tolist()
    assert tuple(g["x_shape"]) == (2, 6, 7, 6, 5) and len(idx) == 8 and len(set(idx)) < len(idx)
    assert os.path.getsize(os.path.join(GOLDEN, "nio3d_trans_train.npz")) <= 1 << 20
    p = nio3d_ref.leaves(st)
    y = t3.niofp3d_trans(p, torch.from_numpy(x), torch.from_numpy(g["in.grid"]), idx=idx)
    e = rel_l2(y.detach().numpy(), g["out"])
    print(f"output rel-L2 {e:.2e}")
    assert e <= OUT_TOL
    loss = F.mse_loss(y, torch.from_numpy(g["target"]).double())
    assert abs(loss.item() - float(g["loss"])) <= OUT_TOL * float(g["loss"])
    loss.backward()
    n = 0
    for k, v in g.items():
        if k.startswith("g."):
            gr = p[k[2:]].grad
            assert gr is not None, k
            gr = (torch.view_as_real(gr) if gr.is_complex() else gr).numpy()
            assert rel_l2(gr, v) <= G_TOL, k
            n += 1
    assert sum(k.startswith("g.trans_input.") for k in g) == 68 and n > 68
    assert not any(k.startswith("g.fc0.") or k == "g.trans_input.placeholder" for k in g)
    for k, q in p.items():
        if k.startswith("fc0.") or k == "trans_input.placeholder":
            assert q.grad is None, k
    # multiplicity matters: the distinct snapshots alone miss the output bar twice over
    with torch.no_grad():
        yd = t3.niofp3d_trans(p, torch.from_numpy(x), torch.from_numpy(g["in.grid"]), idx=sorted(set(idx)))
    assert rel_l2(yd.numpy(), y.detach().numpy()) >= 2 * OUT_TOL


def test_state_dict_layout_matches_reference():
    import blindno
    want = json.load(open(os.path.join(GOLDEN, "layouts_trans3d.json")))[LAYOUT_KEY]
    m = blindno.Transolver3D(H=5, W=6, D=7)
    got = [[k, list(v.shape), str(v.dtype).replace("torch.", "")] for k, v in m.state_dict().items()]
    assert got == want
    assert len(want) == 69 and want[0][0] == "placeholder"
    assert ["blocks.0.Attn.in_project_x.weight", [32, 32, 3, 3, 3], "float32"] in want
    # and the composite: the Transolver, fc0 and one head, nothing else
    n = blindno.NIOFP3D_Trans(2, 4, 2, 2, "cpu", (7, 6, 5))
    g = load_golden("nio3d_trans_train")
    assert [[k, list(v.shape)] for k, v in n.state_dict().items()] == json.loads(str(g["layout_json"]))
    assert [k for k, _ in n.named_children()] == ["trans_input", "fc0", "fno"]
    assert n.unused_prefixes == ("trans_input.placeholder", "fc0.")
    assert blindno.NIOFP3D_Trans is blindno.nio.NIOFP3D_Trans


def test_initialisation_follows_the_reference():
    """A seeded construction reproduces the reference Model's initial weights (the ``init.*``
    arrays of trans3d_model.npz): the same draws in the same order -- orthogonal_ inside each
    attention's constructor, then the truncated normal over every Linear, then the placeholder."""
    import blindno
    g = load_golden("trans3d_model")
    torch.manual_seed(int(g["init_seed"]))
    t = blindno.Transolver3D(H=5, W=6, D=7)
    got = t.state_dict()
    keys = [k for k in g if k.startswith("init.")]
    assert len(keys) == 8
    for k in keys:
        assert np.array_equal(got[k[5:]].numpy(), g[k]), k
    a = t.blocks[0].Attn
    assert torch.all(a.temperature == 0.5) and tuple(a.temperature.shape) == (1, 4, 1, 1)
    for name, p in t.named_parameters():
        if name.endswith("bias") and "in_project_x" not in name and "in_project_fx" not in name:
            assert torch.all(p == 0), name
    assert float(a.in_project_slice.weight.detach().norm(dim=0).max()) < 0.3


def test_unsupported_configurations_are_refused(monkeypatch):
    import blindno
    from blindno import ops
    with pytest.raises(ValueError):
        blindno.Transolver3D(Time_Input=True)
    with pytest.raises(ValueError):
        blindno.Transolver3D(unified_pos=1)
    with pytest.raises(ValueError):
        blindno.Transolver3D(dropout=0.1)
    with pytest.raises(ValueError, match="heads = 4"):
        blindno.Transolver3D(n_head=8)
    with pytest.raises(ValueError, match="heads = 4"):
        blindno.Transolver3D(slice_num=32)
    with pytest.raises(ValueError, match="heads = 4"):
        blindno.Transolver3D(n_hidden=64, n_head=4)
    with pytest.raises(ValueError):
        blindno.Transolver3D(mlp_ratio=4)
    t = blindno.Transolver3D(H=3, W=4, D=5)
    assert (t.H, t.W, t.D) == (3, 4, 5)
    with pytest.raises(ValueError):
        t(torch.zeros(1, 60, 3), None)
    monkeypatch.setattr(ops, "require_device", lambda *a: None)
    with pytest.raises(ValueError, match=r"\(3, 4, 5\)"):
        t.forward_planes(torch.zeros(1, 4, 5, 4, 3))
    m = blindno.NIOFP3D_Trans(1, 2, 2, 2, "cpu", (7, 6, 5))
    with pytest.raises(ValueError, match="7 x 6 x 5"):
        m(torch.zeros(1, 6, 5, 6, 7), torch.zeros(5, 6, 7, 3))
    with pytest.raises(ValueError, match="7 x 6 x 5"):
        m(torch.zeros(1, 6, 7, 6, 5), torch.zeros(7, 6, 6, 3))
    # the op itself: unsupported channel triples, and no CPU path
    z = torch.zeros
    with pytest.raises(ValueError, match=r"\(32, 32, 32\)"):
        ops.PlaneMLPFn.apply(z(1, 16, 8), z(16, 16), z(16), z(16, 16), z(16))
    with pytest.raises(ValueError, match=r"\(32, 32, 32\)"):
        ops.PlaneMLPFn.apply(z(1, 32, 8), z(32, 32), z(32), z(32, 32), z(32))          # no LayerNorm
    with pytest.raises(ValueError, match=r"\(32, 32, 32\)"):
        ops.PlaneMLPFn.apply(z(1, 4, 8), z(64, 4), z(64), z(32, 64), z(32), None, z(4), z(4))
    monkeypatch.undo()
    with pytest.raises(blindno.BlindnoError):
        ops.PlaneMLPFn.apply(z(1, 4, 8), z(64, 4), z(64), z(32, 64), z(32))


def test_restatement_against_torch_layers():
    """transolver3d_ref.plane_mlp against torch.nn.functional in float64, both configurations."""
    g = torch.Generator().manual_seed(4)
    r = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)  # noqa: E731
    x, res, ga, be = r(2, 32, 11), r(2, 32, 11), r(32), r(32)
    W1, b1, W2, b2 = r(32, 32), r(32), r(32, 32), r(32)
    u = F.layer_norm(x.transpose(1, 2), (32,), ga, be, 1e-5)
    want = (F.linear(F.gelu(F.linear(u, W1, b1)), W2, b2) + res.transpose(1, 2)).transpose(1, 2)
    assert float((t3.plane_mlp(x, W1, b1, W2, b2, res, ga, be) - want).abs().max()) < 1e-11
    x, W1, b1, W2 = r(2, 4, 11), r(64, 4), r(64), r(32, 64)
    want = F.linear(F.gelu(F.linear(x.transpose(1, 2), W1, b1)), W2, b2).transpose(1, 2)
    assert float((t3.plane_mlp(x, W1, b1, W2, b2) - want).abs().max()) < 1e-11


def test_planemlp_queries_without_a_device():
    from blindno import _lib
    q = _lib.query
    assert q("blindno_plane_mlp_ok", 32, 32, 32, 1) == 1 and q("blindno_plane_mlp_ok", 4, 64, 32, 0) == 1
    for bad in [(32, 32, 32, 0), (4, 64, 32, 1), (32, 64, 32, 1), (3, 64, 32, 0), (32, 32, 1, 1), (0, 0, 0, 0)]:
        assert q("blindno_plane_mlp_ok", *bad) == 0, bad
    assert q("blindno_plane_mlp_nblk", 64000) == 250 and q("blindno_plane_mlp_nblk", 256) == 1
    assert q("blindno_plane_mlp_nblk", 257) == 2 and q("blindno_plane_mlp_nblk", 0) == -1
    assert q("blindno_plane_mlp_nblk", (1 << 24) + 1) == -1
    assert q("blindno_plane_mlp_bwd_scratch_floats", 300, 64000, 32, 32, 32) == 300 * 250 * (1024 + 32 + 1024 + 32 + 64)
    assert q("blindno_plane_mlp_bwd_scratch_floats", 3, 257, 4, 64, 32) == 3 * 2 * (256 + 64 + 2048 + 32 + 8)
    for bad in [(0, 8, 32, 32, 32), (65536, 8, 32, 32, 32), (1, 0, 32, 32, 32), (1, 8, 32, 32, 16)]:
        assert q("blindno_plane_mlp_bwd_scratch_floats", *bad) == -1, bad
