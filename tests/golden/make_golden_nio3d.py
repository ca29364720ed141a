#!/usr/bin/env python3
"""Capture the golden vectors of the reference's NIOFP3D and the state_dict layouts of its 3D
encoder classes (CPU, about 1.2 s of model time; run where the reference checkout is available --
it never travels with the tests).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_nio3d.py --ref <reference checkout>

``nio3d_train.npz``: NIOFP3D(3, 3, 100, 25, 2, 6, 4, 1, "cpu") in train mode on x (1, 52, 33, 9,
10) with a linspace(-1, 1) grid and np.random.seed(17) for the bag draw.  The model has 28.7 M
parameters, so (as nio2d_nc_train in make_golden.py) the parameters come from the numpy recipe and
are not stored (``layout_json`` / ``complex_json`` / ``recipe_seed`` regenerate them through
tests/nio3d_ref.make_state3d), x is the recipe array ``nio3d.x`` and is not stored either, and the
branch's gradients are stored as norms (``gnorm.*``).  A case past SPLIT_BYTES is split as in
make_golden_fno3d.py.

``layouts3d.json``: names / shapes / dtypes of the reference's NIOFP3D (both encoders), Encoder3D,
Encoder3D_down and ConvBlock3D.

After the capture the float64 restatement (tests/nio3d_ref.py) runs on the same recipe parameters
and the fp32 reference must sit inside every bar tests/test_nio3d_golden.py applies (the
LeakyReLU branch flips of an fp32 run can move the first blocks' gradients by a few 1e-3): if it
does not, change RECIPE_SEED, never the bars.
"""
from __future__ import annotations

import argparse
import json
import os
import subprocess
import sys
import types

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
for _p in (HERE, TESTS, os.path.dirname(TESTS)):
    if _p not in sys.path:
        sys.path.insert(0, _p)

CTOR = (3, 3, 100, 25, 2, 6, 4, 1, "cpu")
X_SHAPE = (1, 52, 33, 9, 10)
RECIPE_SEED = 501
COT_SEED = 51
BAG_SEED = 17
SPLIT_BYTES = 512 * 1024

# the bars of tests/test_nio3d_golden.py (those of nio2d_nc_train)
OUT_TOL, G_TOL, GN_REL, GN_ABS = 1e-4, 1e-3, 1e-3, 1e-5


def _install_timm_stub():
    # 2d_FPE/NIOModules.py imports the vendored Transolver, which needs one name of timm
    import torch
    timm = types.ModuleType("timm")
    models = types.ModuleType("timm.models")
    layers = types.ModuleType("timm.models.layers")
    layers.trunc_normal_ = torch.nn.init.trunc_normal_
    timm.models = models
    models.layers = layers
    sys.modules.update({"timm": timm, "timm.models": models, "timm.models.layers": layers})


def _layout(module):
    return [[k, list(v.shape), str(v.dtype).replace("torch.", "")] for k, v in module.state_dict().items()]


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


def capture():
    import numpy as np
    import torch
    _install_timm_stub()
    import Baselines as BL
    import NIOModules as NM
    from recipe import make_array
    import nio3d_ref

    torch.set_num_threads(8)
    m = NM.NIOFP3D(*CTOR)
    shapes = [(k, tuple(v.shape)) for k, v in m.state_dict().items()]
    cnames = [k for k, v in m.state_dict().items() if v.is_complex()]
    st = nio3d_ref.make_state3d(shapes, RECIPE_SEED, cnames)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in st.items()})
    x = torch.from_numpy(make_array(X_SHAPE, RECIPE_SEED, "nio3d.x"))
    grid = torch.from_numpy(grid_of(X_SHAPE[2:])).requires_grad_(True)
    np.random.seed(BAG_SEED)
    L = np.random.randint(50, x.shape[1])
    idx = np.random.choice(x.shape[1], L)
    np.random.seed(BAG_SEED)
    m.train()
    out = m(x, grid)
    cot = torch.from_numpy(make_array(tuple(out.shape), COT_SEED, "nio3d_train.cot"))
    (out * cot).sum().backward()
    arr = {"out": out.detach().numpy(), "cot": cot.numpy(), "in.grid": grid.detach().numpy(),
           "gin.grid": grid.grad.numpy(), "L": np.asarray(L), "idx": idx,
           "x_shape": np.asarray(X_SHAPE), "recipe_seed": np.asarray(RECIPE_SEED),
           "layout_json": np.asarray(json.dumps([[k, list(s)] for k, s in shapes])),
           "complex_json": np.asarray(json.dumps(cnames))}
    for k, p in m.named_parameters():
        if p.grad is None:
            continue
        if k.startswith(("branch.", "deeponet.branch.")):
            arr["gnorm." + k] = np.array(float(p.grad.double().norm()))
        else:
            g = p.grad
            arr["g." + k] = (torch.view_as_real(g) if g.is_complex() else g).numpy()
    # running statistics of the branch after this one step, as norms (fp32 reference)
    for k, v in m.state_dict().items():
        if k.startswith("branch.") and k.endswith(("running_mean", "running_var")):
            arr["rnorm." + k] = np.array(float(v.double().norm()))
    check_against_fp64(arr, st, x)
    _save("nio3d_train", arr)

    layouts = {
        "NIOFP3D(3,3,100,25,2,6,4,1)": _layout(m),
        "NIOFP3D(3,3,100,25,2,6,4,1,down)": _layout(NM.NIOFP3D(*CTOR, down=True)),
        "Encoder3D(25)": _layout(BL.Encoder3D(25)),
        "Encoder3D_down(25)": _layout(BL.Encoder3D_down(25)),
        "ConvBlock3D(4,6,(1,7,7),(1,2,2),(0,3,3))":
            _layout(BL.ConvBlock3D(4, 6, kernel_size=(1, 7, 7), stride=(1, 2, 2), padding=(0, 3, 3))),
    }
    with open(os.path.join(HERE, "layouts3d.json"), "w") as f:
        json.dump(layouts, f, indent=0)
    print("  wrote layouts3d.json")


def check_against_fp64(arr, st, x):
    """The fp32 reference against the float64 restatement on the same parameters: every bar of
    tests/test_nio3d_golden.py, printed and asserted."""
    import numpy as np
    import torch
    import nio3d_ref

    p = nio3d_ref.leaves(st)
    grid = torch.from_numpy(arr["in.grid"]).double().requires_grad_(True)
    y = nio3d_ref.niofp3d(p, x.double(), grid, idx=arr["idx"].tolist())
    (y * torch.from_numpy(arr["cot"]).double()).sum().backward()

    def rel(a, b):
        return float(np.linalg.norm((a - b).ravel()) / np.linalg.norm(b.ravel()))

    e = rel(arr["out"], y.detach().numpy())
    print(f"  fp32 reference vs float64: out {e:.2e}")
    assert e <= OUT_TOL, e
    worst = 0.0
    for k, v in arr.items():
        if k.startswith("g."):
            g = p[k[2:]].grad
            g = (torch.view_as_real(g) if g.is_complex() else g).numpy()
            worst = max(worst, rel(v, g))
    e = rel(arr["gin.grid"], grid.grad.numpy())
    print(f"  max g.* {worst:.2e}, gin.grid {e:.2e}")
    assert worst <= G_TOL and e <= G_TOL, (worst, e)
    gmax = max(float(v) for k, v in arr.items() if k.startswith("gnorm."))
    for k, v in arr.items():
        if k.startswith("gnorm."):
            got = float(p[k[6:]].grad.norm())
            d = abs(got - float(v))
            bar = GN_REL * abs(float(v)) + GN_ABS * gmax
            print(f"  {k}: fp32 {float(v):.6e} fp64 {got:.6e} diff/bar {d / bar:.2f}")
            assert d <= bar, (k, got, float(v))


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
