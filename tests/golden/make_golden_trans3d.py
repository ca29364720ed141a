#!/usr/bin/env python3
"""Capture the golden vectors of the reference's structured-mesh 3D Transolver and of the 3D
Transolver-NIO composed around it, and the Transolver's state_dict layout (CPU; run where the
reference checkout is available -- it never travels with the tests).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_trans3d.py --ref <reference checkout>

``trans3d_model.npz``: 2d_FPE's model/Transolver_Structured_Mesh_3D.Model(space_dim=3, n_layers=3,
n_hidden=32, n_head=4, mlp_ratio=1, fun_dim=1, out_dim=1, slice_num=16, H=5, W=6, D=7) on S = 3
snapshots of point features x (S, 210, 3), fx (S, 210, 1) (the recipe arrays ``trans3d.x`` /
``trans3d.fx``, stored).  The parameters come from the numpy recipe with the rescaling of
make_golden_trans.py (``layout_json`` / ``recipe_seed`` / ``rescale_json`` regenerate them through
transolver_ref.rescaled_state) and are not stored.  Stored: the output, the cotangent, the
gradients of both inputs (``gin.x``, ``gin.fx``) and of one parameter of each kind (GRAD_KEYS),
and, as ``init.*``, a few tensors of the Model's own initialisation after torch.manual_seed(3).
As in make_golden_trans.py the attention must matter in the fixture: uniform slice weights must
move the REFERENCE's own fp32 output by at least 10 x OUT_TOL and the mean row maximum of the slice
weights must exceed 2/16.  If a seed fails, take the next seed, never another bar.

``layouts_trans3d.json``: names / shapes / dtypes of that Model's state_dict.

``nio3d_trans_train.npz``: the reference has no 3D Transolver composite.  The golden model
composes what it does have, in its fp32: the Model above on the grid (7, 6, 5) (the smallest grid
make_golden_nio3d_fno.py uses for FNO3d) as ``trans_input``, its bag-mean expression
(2d_FPE/NIOModules.py:149-160) with one more grid channel, ``fc0`` = Linear(4, 4) read through
``.data``, and its ``FNO3d`` (2d_FPE/FNOModules.py:290-366) as the head ``fno`` = FNO3d(2, 4, 2, 4,
2).  That is NIOFP3D_Trans(2, 4, 2, 2, "cpu", (7, 6, 5)).  Train mode on x (2, 6, 7, 6, 5) with a
linspace(-1, 1) grid and the recorded bag BAG_IDX, which holds repeated entries, so multiplicity
matters.  Stored: ``out``, ``target``, ``loss`` (the MSE of ``out`` against ``target``), ``in.grid``,
``idx`` and the gradient of the loss with respect to every trained parameter (``fc0.*`` and the
Transolver's ``placeholder`` get none; block 2's four temperatures lie outside the clamp at this
seed, so that gradient is exactly zero).

After each capture the float64 restatement (tests/transolver3d_ref.py) runs on the same recipe
parameters and the fp32 reference must sit inside every bar tests/test_transolver3d_ref.py applies
(those of tests/test_transolver_ref.py).
"""
from __future__ import annotations

import argparse
import json
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
for _p in (HERE, TESTS, os.path.dirname(TESTS)):
    if _p not in sys.path:
        sys.path.insert(0, _p)

from make_golden_trans import RESCALE, ROWMAX_MIN, _install_timm_stub, _layout, _slice_probe  # noqa: E402

MODEL_KW = dict(space_dim=3, n_layers=3, n_hidden=32, dropout=0.0, n_head=4, Time_Input=False, mlp_ratio=1,
                fun_dim=1, out_dim=1, slice_num=16, ref=8, unified_pos=False)
MESH = (5, 6, 7)
S = 3
RECIPE_SEED = 711
COT_SEED = 71
GRAD_KEYS = ("preprocess.linear_pre.0.weight", "preprocess.linear_post.bias", "blocks.0.ln_1.weight",
             "blocks.0.ln_1.bias", "blocks.0.ln_2.weight", "blocks.1.Attn.temperature",
             "blocks.1.Attn.in_project_x.weight", "blocks.1.Attn.in_project_fx.bias",
             "blocks.1.Attn.in_project_slice.weight", "blocks.1.Attn.in_project_slice.bias",
             "blocks.1.Attn.to_q.weight", "blocks.1.Attn.to_k.weight", "blocks.1.Attn.to_v.weight",
             "blocks.1.Attn.to_out.0.weight", "blocks.1.mlp.linear_pre.0.weight",
             "blocks.1.mlp.linear_pre.0.bias", "blocks.1.mlp.linear_post.weight", "blocks.2.ln_3.weight",
             "blocks.2.mlp2.weight", "blocks.2.mlp2.bias")
# the reference's own initialisation after torch.manual_seed(INIT_SEED): a few small tensors
INIT_SEED = 3
INIT_KEYS = ("placeholder", "preprocess.linear_pre.0.weight", "preprocess.linear_post.weight",
             "blocks.0.Attn.in_project_slice.weight", "blocks.1.Attn.in_project_fx.bias",
             "blocks.1.Attn.to_v.weight", "blocks.2.mlp.linear_post.weight", "blocks.2.mlp2.weight")

NIO_CTOR = (2, 4, 2, 2)            # fno_layers, width, modes, output_dim
NIO_X_SHAPE = (2, 6, 7, 6, 5)
NIO_RECIPE_SEED = 712
NIO_COT_SEED = 72
BAG_IDX = (4, 4, 4, 4, 0, 4, 4, 1)

# the bars of tests/test_transolver3d_ref.py (those of tests/test_transolver_ref.py)
OUT_TOL, G_TOL = 1e-4, 1e-3


def grid_of(shape):
    import numpy as np
    axes = [np.linspace(-1, 1, n, dtype=np.float32) for n in shape]
    return np.stack(np.meshgrid(*axes, indexing="ij"), axis=-1)


def rel(a, b):
    import numpy as np
    den = float(np.linalg.norm(b.ravel()))
    return float(np.linalg.norm((a - b).ravel())) / (den if den > 0 else 1.0)


def _probed(blocks, n_points, uniform, run):
    """run() with every block's slice softmax probed (make_golden_trans._slice_probe)."""
    import numpy as np
    import torch
    seen = []
    saved = [(b.Attn, b.Attn.softmax) for b in blocks]
    for attn, _ in saved:
        attn.softmax = _slice_probe(n_points, uniform, seen)
    try:
        with torch.no_grad():
            out = run()
    finally:
        for attn, sm in saved:
            attn.softmax = sm
    return out, float(np.mean(seen))


def _attention_matters(blocks, n_points, run):
    out_a, rowmax = _probed(blocks, n_points, False, run)
    out_u, _ = _probed(blocks, n_points, True, run)
    move = float((out_a - out_u).norm() / out_a.norm())
    print(f"  mean row max of w {rowmax:.3f}; uniform slice weights move the reference's output by {move:.2e}")
    if move < 10 * OUT_TOL or rowmax <= ROWMAX_MIN:
        raise SystemExit("the attention does not matter at this RECIPE_SEED: take the next")
    return rowmax, move


def capture_model():
    import numpy as np
    import torch
    from model.Transolver_Structured_Mesh_3D import Model
    from recipe import make_array
    import transolver3d_ref as t3
    import transolver_ref

    H, W, D = MESH
    N = H * W * D
    torch.manual_seed(INIT_SEED)
    m = Model(H=H, W=W, D=D, **MODEL_KW)
    init = {"init." + k: m.state_dict()[k].numpy().copy() for k in INIT_KEYS}
    with open(os.path.join(HERE, "layouts_trans3d.json"), "w") as f:
        json.dump({f"2d_FPE.Transolver_Structured_Mesh_3D.Model({H},{W},{D})": _layout(m)}, f, indent=0)
    print("  wrote layouts_trans3d.json")
    shapes = [(k, tuple(v.shape)) for k, v in m.state_dict().items()]
    st = transolver_ref.rescaled_state(shapes, RECIPE_SEED, RESCALE)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in st.items()})
    m.train()
    x = torch.from_numpy(make_array((S, N, 3), RECIPE_SEED, "trans3d.x")).requires_grad_(True)
    fx = torch.from_numpy(make_array((S, N, 1), RECIPE_SEED, "trans3d.fx")).requires_grad_(True)
    rowmax, move = _attention_matters(m.blocks, N, lambda: m(x, fx))
    out = m(x, fx)
    cot = torch.from_numpy(make_array(tuple(out.shape), COT_SEED, "trans3d_model.cot"))
    (out * cot).sum().backward()
    params = dict(m.named_parameters())
    assert params["placeholder"].grad is None
    arr = {"out": out.detach().numpy(), "cot": cot.numpy(), "in.x": x.detach().numpy(),
           "in.fx": fx.detach().numpy(), "gin.x": x.grad.numpy(), "gin.fx": fx.grad.numpy(),
           "mesh": np.asarray(MESH), "recipe_seed": np.asarray(RECIPE_SEED),
           "w_rowmax_mean": np.asarray(rowmax), "uniform_move_out": np.asarray(move),
           "rescale_json": np.asarray(json.dumps(RESCALE)),
           "layout_json": np.asarray(json.dumps([[k, list(s)] for k, s in shapes]))}
    for k in GRAD_KEYS:
        arr["g." + k] = params[k].grad.numpy()
    arr.update(init)
    arr["init_seed"] = np.asarray(INIT_SEED)

    # the fp32 reference against the float64 restatement on the same parameters
    p = {k: torch.from_numpy(v).double().requires_grad_(True) for k, v in st.items()}
    inp = torch.cat((x.detach(), fx.detach()), -1).transpose(1, 2).double().requires_grad_(True)
    rec = []
    y = t3.transolver3d(p, inp, MESH, record=rec)
    (y * cot.transpose(1, 2).double()).sum().backward()
    e = rel(arr["out"], y.detach().transpose(1, 2).numpy())
    print(f"  fp32 reference vs float64: out {e:.2e}")
    assert e <= OUT_TOL, e
    gin = inp.grad.transpose(1, 2).numpy()
    errs = {"gin.x": rel(arr["gin.x"], gin[..., :3]), "gin.fx": rel(arr["gin.fx"], gin[..., 3:])}
    errs.update({"g." + k: rel(arr["g." + k], p[k].grad.numpy()) for k in GRAD_KEYS})
    worst = max(errs, key=errs.get)
    print(f"  max gradient error {errs[worst]:.2e} ({worst}, {len(errs)} gradients)")
    assert errs[worst] <= G_TOL, (worst, errs[worst])
    r64 = float(np.mean([float(w.max(2).values.mean()) for w in rec]))
    assert abs(r64 - rowmax) <= 1e-4, (r64, rowmax)
    path = os.path.join(HERE, "trans3d_model.npz")
    np.savez_compressed(path, **arr)
    print(f"  wrote trans3d_model.npz ({os.path.getsize(path) / 1024:.1f} KiB, {len(arr)} arrays)")


def build_composite():
    """The composition, on the reference's Model and FNO3d."""
    import torch
    import torch.nn as nn
    import FNOModules as FM
    from model.Transolver_Structured_Mesh_3D import Model

    fno_layers, width, modes, output_dim = NIO_CTOR
    H, W, D = NIO_X_SHAPE[2:]

    class RefNIOFP3D_Trans(nn.Module):
        def __init__(self):
            super().__init__()
            self.trans_input = Model(H=H, W=W, D=D, **MODEL_KW)
            self.fc0 = nn.Linear(4, width)
            self.fno = FM.FNO3d(modes=modes, width=width, n_layers=fno_layers, input_dim=width,
                                output_dim=output_dim)

        def forward(self, x, grid, idx):
            x = x[:, idx]
            L = x.shape[1]
            batchsize = x.shape[0]
            x_input = x.reshape(x.shape[0] * x.shape[1], -1, 1)
            nx, ny, nz = grid.shape[:3]
            grid_r = grid.unsqueeze(0).repeat(x_input.shape[0], 1, 1, 1, 1).reshape(x_input.shape[0], -1, 3)
            x = self.trans_input(x_input, grid_r)
            x = x.view(batchsize, L, nx, ny, nz)
            grid = grid.unsqueeze(0).repeat(x.shape[0], 1, 1, 1, 1).permute(0, 4, 1, 2, 3)
            x = torch.cat((grid, x), 1)
            weight_trans_mat = self.fc0.weight.data
            bias_trans_mat = self.fc0.bias.data
            weight_trans_mat = torch.cat(
                [weight_trans_mat[:, :3], weight_trans_mat[:, 3].view(-1, 1).repeat(1, L) / L], dim=1)
            x = x.permute(0, 2, 3, 4, 1)
            x = torch.matmul(x, weight_trans_mat.T) + bias_trans_mat
            return self.fno(x)

    return RefNIOFP3D_Trans()


def nio_state(shapes, cnames, seed):
    """The composite's parameters: the recipe's draw (complex FNO3d weights as in
    nio3d_ref.make_state3d), the Transolver's part rescaled as in make_golden_trans.py."""
    import numpy as np
    import nio3d_ref
    st = nio3d_ref.make_state3d(shapes, seed, cnames)
    for name in st:
        if name.startswith("trans_input."):
            for suffix, f in RESCALE.items():
                if name.endswith(suffix):
                    st[name] = (st[name] * np.float32(f)).astype(st[name].dtype)
    return st


def capture_nio():
    import numpy as np
    import torch
    from recipe import make_array
    import nio3d_ref
    import transolver3d_ref as t3

    torch.manual_seed(0)
    m = build_composite()
    shapes = [(k, tuple(v.shape)) for k, v in m.state_dict().items()]
    cnames = [k for k, v in m.state_dict().items() if v.is_complex()]
    st = nio_state(shapes, cnames, NIO_RECIPE_SEED)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in st.items()})
    m.train()
    x = torch.from_numpy(make_array(NIO_X_SHAPE, NIO_RECIPE_SEED, "nio3d_trans.x"))
    grid = torch.from_numpy(grid_of(NIO_X_SHAPE[2:]))
    idx = list(BAG_IDX)
    assert len(set(idx)) < len(idx) and max(idx) < NIO_X_SHAPE[1]
    n_points = int(np.prod(NIO_X_SHAPE[2:]))
    _attention_matters(m.trans_input.blocks, n_points, lambda: m(x, grid, idx))
    out = m(x, grid, idx)
    with torch.no_grad():
        move = rel(m(x, grid, sorted(set(idx))).numpy(), out.detach().numpy())
    print(f"  the distinct snapshots alone move the reference's output by {move:.2e}")
    if move < 2 * OUT_TOL:             # a model that ignored multiplicity would miss the output bar twice over
        raise SystemExit("multiplicity does not matter in this bag: take another")
    target = torch.from_numpy(make_array(tuple(out.shape), NIO_COT_SEED, "nio3d_trans_train.target"))
    loss = torch.nn.functional.mse_loss(out, target)
    loss.backward()
    arr = {"out": out.detach().numpy(), "target": target.numpy(), "loss": np.asarray(loss.item()),
           "in.grid": grid.numpy(), "idx": np.asarray(idx), "ctor": np.asarray(NIO_CTOR),
           "x_shape": np.asarray(NIO_X_SHAPE), "recipe_seed": np.asarray(NIO_RECIPE_SEED),
           "rescale_json": np.asarray(json.dumps(RESCALE)),
           "layout_json": np.asarray(json.dumps([[k, list(s)] for k, s in shapes])),
           "complex_json": np.asarray(json.dumps(cnames))}
    for k, p in m.named_parameters():
        if k.startswith("fc0.") or k == "trans_input.placeholder":
            assert p.grad is None, k
            continue
        g = p.grad
        arr["g." + k] = (torch.view_as_real(g) if g.is_complex() else g).numpy()

    p = nio3d_ref.leaves(st)
    y = t3.niofp3d_trans(p, x.double(), grid.double(), idx=idx)
    l64 = torch.nn.functional.mse_loss(y, target.double())
    l64.backward()
    e = rel(arr["out"], y.detach().numpy())
    print(f"  fp32 reference vs float64: out {e:.2e}, loss {abs(float(arr['loss']) - l64.item()) / l64.item():.2e}")
    assert e <= OUT_TOL, e
    worst = (0.0, "")
    for k, v in arr.items():
        if k.startswith("g."):
            g = p[k[2:]].grad
            g = (torch.view_as_real(g) if g.is_complex() else g).numpy()
            worst = max(worst, (rel(v, g), k))
    print(f"  max g.* {worst[0]:.2e} ({worst[1]})")
    assert worst[0] <= G_TOL, worst
    # every temperature of block 2 lies outside the clamp at this seed: the reference's gradient is 0
    zero = [k for k, v in arr.items() if k.startswith("g.") and not np.any(v)]
    assert zero == ["g.trans_input.blocks.2.Attn.temperature"], zero
    path = os.path.join(HERE, "nio3d_trans_train.npz")
    np.savez_compressed(path, **arr)
    print(f"  wrote nio3d_trans_train.npz ({os.path.getsize(path) / 1024:.1f} KiB, {len(arr)} arrays)")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", required=True, help="checkout of the reference repository")
    ap.add_argument("--capture", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.capture:
        import torch
        sys.path.insert(0, os.path.join(a.ref, "2d_FPE"))
        _install_timm_stub()
        torch.set_num_threads(8)
        capture_model()
        capture_nio()
        return
    env = dict(os.environ, PYTHONDONTWRITEBYTECODE="1")
    subprocess.run([sys.executable, __file__, "--ref", a.ref, "--capture"], check=True, env=env)


if __name__ == "__main__":
    main()
