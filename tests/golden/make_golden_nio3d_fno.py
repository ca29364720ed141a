#!/usr/bin/env python3
"""Capture the golden vectors of the 3D FNO-NIO model NIOFP3D_FNO from the reference's own code
(CPU, a few seconds; run where the reference checkout is available -- it never travels with the
tests).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_nio3d_fno.py --ref <reference checkout>

The reference has no 3D FNO-NIO class.  The golden model composes what it does have, in its fp32:
its ``FNO3d`` class (2d_FPE/FNOModules.py:290-366) as the snapshot encoder ``FNO_input`` =
FNO3d(2, 4, 2, 4, 1) and as the head ``fno`` = FNO3d(2, 4, 2, 4, 2), joined by its bag-mean
expression (2d_FPE/NIOModules.py:565-575) with one more grid channel, ``fc0`` = Linear(4, 4)
read through ``.data``.  That is NIOFP3D_FNO(2, 4, 2, 2, "cpu").

``nio3d_fno_train.npz``: the model in train mode on x (2, 52, 7, 6, 5) with a linspace(-1, 1)
grid and np.random.seed(23) for the bag draw (the draw of 2d_FPE/NIOModules.py:548-551).  As in
make_golden_nio3d.py the parameters come from the numpy recipe and are not stored
(``layout_json`` / ``complex_json`` / ``recipe_seed`` regenerate them through
tests/nio3d_ref.make_state3d), and x is the recipe array ``nio3d_fno.x``.  Stored: ``out``,
``cot``, ``in.grid``, ``L``, ``idx`` and every trained parameter's gradient ``g.*``.  A case past
SPLIT_BYTES is split as in make_golden_fno3d.py.

After the capture the float64 restatement (tests/nio3d_fno_ref.py) runs on the same recipe
parameters and the fp32 reference must sit inside every bar tests/test_nio3d_fno_golden.py
applies: if it does not, change RECIPE_SEED, never the bars.
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

CTOR = (2, 4, 2, 2)            # fno_layers, width, modes, output_dim
X_SHAPE = (2, 52, 7, 6, 5)
RECIPE_SEED = 611
COT_SEED = 61
BAG_SEED = 23
SPLIT_BYTES = 512 * 1024

# the bars of tests/test_nio3d_fno_golden.py (those of tests/test_nio3d_golden.py)
OUT_TOL, G_TOL = 1e-4, 1e-3


def grid_of(shape):
    import numpy as np
    axes = [np.linspace(-1, 1, n, dtype=np.float32) for n in shape]
    return np.stack(np.meshgrid(*axes, indexing="ij"), axis=-1)


def _save(name, arr):
    import numpy as np

    def write(n, a):
        path = os.path.join(HERE, f"{n}.npz")
        np.savez_compressed(path, **a)
        print(f"  wrote {n}.npz ({os.path.getsize(path) / 1024:.1f} KiB, {len(a)} arrays)")

    if sum(v.nbytes for v in arr.values()) <= SPLIT_BYTES:
        write(name, arr)
        return
    bwd = {k: v for k, v in arr.items() if k == "cot" or k.startswith(("g.", "gin."))}
    write(name, {k: v for k, v in arr.items() if k not in bwd})
    write(name + "_bwd", bwd)


def build_model(FM):
    """The composition, on the reference's FNO3d."""
    import numpy as np
    import torch
    import torch.nn as nn

    fno_layers, width, modes, output_dim = CTOR

    class RefNIOFP3D_FNO(nn.Module):
        def __init__(self):
            super().__init__()
            self.FNO_input = FM.FNO3d(modes=modes, width=4, n_layers=2, input_dim=4, output_dim=1)
            self.fc0 = nn.Linear(4, width)
            self.fno = FM.FNO3d(modes=modes, width=width, n_layers=fno_layers, input_dim=width,
                                output_dim=output_dim)

        def forward(self, x, grid):
            if self.training:
                L = np.random.randint(50, x.shape[1])
                idx = np.random.choice(x.shape[1], L)
                x = x[:, idx]
            else:
                L = x.shape[1]
            batchsize = x.shape[0]
            x_input = x.reshape(x.shape[0] * x.shape[1], 1, *x.shape[2:])
            nx, ny, nz = grid.shape[:3]
            grid_r = grid.permute(3, 0, 1, 2).unsqueeze(0).repeat(x_input.shape[0], 1, 1, 1, 1)
            inp = torch.cat((x_input, grid_r), dim=1).permute(0, 2, 3, 4, 1)
            x = self.FNO_input(inp)
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

    return RefNIOFP3D_FNO()


def capture():
    import numpy as np
    import torch
    import FNOModules as FM
    from recipe import make_array
    import nio3d_fno_ref

    torch.set_num_threads(8)
    m = build_model(FM)
    shapes = [(k, tuple(v.shape)) for k, v in m.state_dict().items()]
    cnames = [k for k, v in m.state_dict().items() if v.is_complex()]
    st = nio3d_fno_ref.make_state3d(shapes, RECIPE_SEED, cnames)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in st.items()})
    x = torch.from_numpy(make_array(X_SHAPE, RECIPE_SEED, "nio3d_fno.x"))
    grid = torch.from_numpy(grid_of(X_SHAPE[2:]))
    np.random.seed(BAG_SEED)
    L = np.random.randint(50, x.shape[1])
    idx = np.random.choice(x.shape[1], L)
    np.random.seed(BAG_SEED)
    m.train()
    out = m(x, grid)
    cot = torch.from_numpy(make_array(tuple(out.shape), COT_SEED, "nio3d_fno_train.cot"))
    (out * cot).sum().backward()
    assert len(set(idx.tolist())) < L, "the golden bag should hold repeated draws"
    arr = {"out": out.detach().numpy(), "cot": cot.numpy(), "in.grid": grid.numpy(),
           "L": np.asarray(L), "idx": idx, "bag_seed": np.asarray(BAG_SEED),
           "ctor": np.asarray(CTOR), "x_shape": np.asarray(X_SHAPE),
           "recipe_seed": np.asarray(RECIPE_SEED),
           "layout_json": np.asarray(json.dumps([[k, list(s)] for k, s in shapes])),
           "complex_json": np.asarray(json.dumps(cnames))}
    for k, p in m.named_parameters():
        if k.startswith("fc0."):
            assert p.grad is None, k
            continue
        g = p.grad
        arr["g." + k] = (torch.view_as_real(g) if g.is_complex() else g).numpy()
    check_against_fp64(arr, st, x)
    _save("nio3d_fno_train", arr)


def check_against_fp64(arr, st, x):
    """The fp32 reference against the float64 restatement on the same parameters: every bar of
    tests/test_nio3d_fno_golden.py, printed and asserted."""
    import numpy as np
    import torch
    import nio3d_fno_ref

    p = nio3d_fno_ref.leaves(st)
    grid = torch.from_numpy(arr["in.grid"]).double()
    y = nio3d_fno_ref.niofp3d_fno(p, x.double(), grid, idx=arr["idx"].tolist())
    (y * torch.from_numpy(arr["cot"]).double()).sum().backward()

    def rel(a, b):
        return float(np.linalg.norm((a - b).ravel()) / np.linalg.norm(b.ravel()))

    e = rel(arr["out"], y.detach().numpy())
    print(f"  fp32 reference vs float64: out {e:.2e}")
    assert e <= OUT_TOL, e
    worst = (0.0, "")
    for k, v in arr.items():
        if k.startswith("g."):
            g = p[k[2:]].grad
            g = (torch.view_as_real(g) if g.is_complex() else g).numpy()
            worst = max(worst, (rel(v, g), k))
    print(f"  max g.* {worst[0]:.2e} ({worst[1]})")
    assert worst[0] <= G_TOL, worst


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", required=True, help="checkout of the reference repository")
    ap.add_argument("--capture", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.capture:
        sys.path.insert(0, os.path.join(a.ref, "2d_FPE"))
        capture()
        return
    env = dict(os.environ, PYTHONDONTWRITEBYTECODE="1")
    subprocess.run([sys.executable, __file__, "--ref", a.ref, "--capture"], check=True, env=env)


if __name__ == "__main__":
    main()
