#!/usr/bin/env python3
"""Capture the golden vectors of the reference's NIOFP2D_attn and its state_dict layout (CPU; run
where the reference checkout is available -- it never travels with the tests).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_nio2d_attn.py --ref <reference checkout>

``nio2d_attn_train.npz``: the non-conservative experiment's NIOFP2D_attn(2, 3, 100, 25, 2, 6, 8, 2)
(2d_Non_conservative_FPE/NIOModules.py:406-, heads fno_Fx / fno_Fy, Encoder2D (3, 2)) in train mode
on x (1, 52, 80, 80) with a linspace(-1, 1) grid and np.random.seed(17) for the bag draw: L =
randint(50, 52) = 51 draws with replacement (35 distinct snapshots, so the recorded draw holds
duplicates).  As nio2d_nc_train in make_golden.py and
nio3d_train in make_golden_nio3d.py, the parameters come from the numpy recipe (``layout_json`` /
``recipe_seed`` regenerate them through recipe.make_state) and the branch's gradients are stored
as norms (``gnorm.*``); x is AMP times the recipe array ``nio2d_attn.x`` and is not stored.

The attention must matter in the fixture (a restatement that replaced A by the uniform matrix must
not pass): the REFERENCE's own fp32 fused field AND model output must both move by at least 10 x
OUT_TOL (relative) when its attention matrix is replaced by the uniform one; the mean row maximum of
A is recorded (``A_rowmax_mean``).  AMP, the input amplitude, is the smallest of AMPS at which that
holds -- but the amplitude turns out not to act at all: the branch's first BatchNorm divides it out,
so every AMP gives the same tokens.  What decides the condition is the parameter draw.  With
RECIPE_SEED = 411 the fused field moves by 24 % and the output by only 9.9e-4 (the heads of that
draw barely read their input); 412 is the first seed after it that meets the condition (fused field
35 %, output 1.0e-2; seeds 412-422 all do, 2.3e-3 .. 3.7e-2).

``layouts_nio2d_attn.json``: names / shapes / dtypes of NIOFP2D_attn(2,3,100,25,3,12,32,2) in both
2D experiments.

After the capture the float64 restatement (tests/nio2d_attn_ref.niofp2d_attn) runs on the same
recipe parameters and the fp32 reference must sit inside every bar tests/test_nio2d_attn.py applies:
if it does not, change RECIPE_SEED, never the bars.
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

CTOR = (2, 3, 100, 25, 2, 6, 8, 2)
LAYOUT_CTOR = (2, 3, 100, 25, 3, 12, 32, 2)
X_SHAPE = (1, 52, 80, 80)
RECIPE_SEED = 412
COT_SEED = 43
BAG_SEED = 17
AMPS = (1.0, 2.0, 4.0)

# the bars of tests/test_nio2d_attn.py (those of test_oracle_golden.py::test_niofp2d_nio_branch_trunk)
OUT_TOL, G_TOL, GN_REL, GN_ABS = 1e-4, 1e-3, 1e-3, 1e-5


def _install_timm_stub():
    # NIOModules.py imports the vendored Transolver, which needs one name of timm
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


def grid_of(n):
    import numpy as np
    ax = np.linspace(-1, 1, n, dtype=np.float32)
    gx, gy = np.meshgrid(ax, ax, indexing="ij")
    return np.stack([gx, gy], axis=2)


def _attention_of(m, x, grid, idx):
    """(A, fused field, fused field under uniform attention) of the reference's own fp32 forward,
    recomputed from its submodules exactly as NIOFP2D_attn.forward composes them."""
    import math
    import torch
    with torch.no_grad():
        xs = x[:, idx]
        B, L = xs.shape[:2]
        nx, ny = grid.shape[:2]
        u = m.deeponet(xs.unsqueeze(2), grid.view(-1, 2)).view(B, L, nx * ny)
        xt = torch.cat((grid.view(-1, 2).t().unsqueeze(0).repeat(B, 1, 1), u), 1)
        A = torch.softmax(xt @ xt.transpose(1, 2) / math.sqrt(nx * ny), -1)
        w0, b = m.fc0.weight.data[:, 0], m.fc0.bias.data
        fused = (A @ xt).mean(1).unsqueeze(-1) * w0 + b
        uniform = xt.mean(1).unsqueeze(-1) * w0 + b
        heads = lambda h: torch.cat((m.fno_Fx(h.view(B, nx, ny, -1)), m.fno_Fy(h.view(B, nx, ny, -1))), -1)  # noqa: E731
        out, out_uniform = heads(fused), heads(uniform)
    return A, fused, uniform, out, out_uniform


def capture(exp):
    import numpy as np
    import torch
    _install_timm_stub()
    import NIOModules as NM
    from recipe import make_array, make_state

    torch.set_num_threads(8)
    if exp == "layout":
        return _layout(NM.NIOFP2D_attn(*LAYOUT_CTOR))
    m = NM.NIOFP2D_attn(*CTOR)
    shapes = [(k, tuple(v.shape)) for k, v in m.state_dict().items()]
    st = make_state(shapes, seed=RECIPE_SEED)
    x1 = torch.from_numpy(make_array(X_SHAPE, RECIPE_SEED, "nio2d_attn.x"))
    grid = torch.from_numpy(grid_of(X_SHAPE[2]))
    np.random.seed(BAG_SEED)
    L = np.random.randint(50, X_SHAPE[1])
    idx = np.random.choice(X_SHAPE[1], L)
    assert L == 51, "the fixture records 51 draws"
    assert len(set(idx.tolist())) < L, "the recorded draw must hold a duplicate"
    for amp in AMPS:
        m.load_state_dict({k: torch.from_numpy(v) for k, v in st.items()})
        m.train()
        x = amp * x1
        A, fused, uniform, out_a, out_u = _attention_of(m, x, grid, idx)
        move = float((fused - uniform).norm() / fused.norm())
        move_out = float((out_a - out_u).norm() / out_a.norm())
        rowmax = float(A.max(-1).values.mean())
        print(f"  amp {amp}: mean row max of A {rowmax:.3f}, uniform attention moves the fused field by {move:.2e} "
              f"and the output by {move_out:.2e}")
        if min(move, move_out) >= 10 * OUT_TOL:
            break
    else:
        raise SystemExit("the attention does not matter at this RECIPE_SEED (no amplitude changes that): take the next")
    m.load_state_dict({k: torch.from_numpy(v) for k, v in st.items()})    # fresh running statistics
    m.train()
    np.random.seed(BAG_SEED)
    out = m(x, grid)
    cot = torch.from_numpy(make_array(tuple(out.shape), COT_SEED, "nio2d_attn_train.cot"))
    (out * cot).sum().backward()
    arr = {"out": out.detach().numpy(), "cot": cot.numpy(), "in.grid": grid.numpy(), "L": np.asarray(L),
           "idx": idx, "amp": np.asarray(amp, np.float32), "x_shape": np.asarray(X_SHAPE),
           "recipe_seed": np.asarray(RECIPE_SEED), "A_rowmax_mean": np.asarray(rowmax),
           "uniform_move": np.asarray(move), "uniform_move_out": np.asarray(move_out),
           "layout_json": np.asarray(json.dumps([[k, list(s)] for k, s in shapes]))}
    for k, p in m.named_parameters():
        if p.grad is None:
            continue
        if k.startswith(("branch.", "deeponet.branch.")):
            arr["gnorm." + k] = np.array(float(p.grad.double().norm()))
        else:
            arr["g." + k] = p.grad.numpy()
    check_against_fp64(arr, st, x)
    path = os.path.join(HERE, "nio2d_attn_train.npz")
    np.savez_compressed(path, **arr)
    print(f"  wrote nio2d_attn_train.npz ({os.path.getsize(path) / 1024:.1f} KiB, {len(arr)} arrays)")
    assert os.path.getsize(path) < os.path.getsize(os.path.join(HERE, "nio2d_nc_train.npz"))
    return None


def check_against_fp64(arr, st, x):
    """The fp32 reference against the float64 restatement on the same parameters: every bar of
    tests/test_nio2d_attn.py, printed and asserted."""
    import numpy as np
    import torch
    import nio2d_attn_ref

    p = {k: torch.from_numpy(v).double().requires_grad_(v.dtype.kind == "f") for k, v in st.items()}
    grid = torch.from_numpy(arr["in.grid"]).double()
    rec = {}
    y = nio2d_attn_ref.niofp2d_attn(p, x.double(), grid, idx=arr["idx"].tolist(), heads=("fno_Fx", "fno_Fy"),
                                    record=rec)
    (y * torch.from_numpy(arr["cot"]).double()).sum().backward()

    def rel(a, b):
        return float(np.linalg.norm((a - b).ravel()) / np.linalg.norm(b.ravel()))

    e = rel(arr["out"], y.detach().numpy())
    move = rel(rec["h_uniform"].numpy(), rec["h"].numpy())
    move_out = rel(rec["y_uniform"].numpy(), y.detach().numpy())
    print(f"  fp32 reference vs float64: out {e:.2e}; float64 uniform-attention move: fused field {move:.2e}, "
          f"output {move_out:.2e}; mean row max {float(rec['A'].max(-1).values.mean()):.3f}")
    assert e <= OUT_TOL, e
    assert move >= 10 * OUT_TOL and move_out >= 10 * OUT_TOL, (move, move_out)
    worst = max(rel(v, p[k[2:]].grad.numpy()) for k, v in arr.items() if k.startswith("g."))
    print(f"  max g.* {worst:.2e}")
    assert worst <= G_TOL, worst
    gmax = max(float(v) for k, v in arr.items() if k.startswith("gnorm."))
    for k, v in arr.items():
        if k.startswith("gnorm."):
            got = float(p[k[6:]].grad.norm())
            d = abs(got - float(v))
            bar = GN_REL * abs(float(v)) + GN_ABS * gmax
            assert d <= bar, (k, got, float(v))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", required=True, help="checkout of the reference repository")
    ap.add_argument("--capture", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.capture:
        exp, what = a.capture.split(":")
        sys.path.insert(0, os.path.join(a.ref, exp))
        lay = capture(what)
        if lay is not None:
            print("LAYOUT " + json.dumps(lay))
        return
    env = dict(os.environ, PYTHONDONTWRITEBYTECODE="1")
    layouts = {}
    for exp, key in (("2d_FPE", "2d_FPE"), ("2d_Non_conservative_FPE", "2d_NC")):
        r = subprocess.run([sys.executable, __file__, "--ref", a.ref, "--capture", exp + ":layout"],
                           check=True, env=env, capture_output=True, text=True)
        line = [ln for ln in r.stdout.splitlines() if ln.startswith("LAYOUT ")][-1]
        layouts[f"{key}.NIOFP2D_attn({','.join(map(str, LAYOUT_CTOR))})"] = json.loads(line[7:])
    with open(os.path.join(HERE, "layouts_nio2d_attn.json"), "w") as f:
        json.dump(layouts, f, indent=0)
    print("  wrote layouts_nio2d_attn.json")
    subprocess.run([sys.executable, __file__, "--ref", a.ref, "--capture", "2d_Non_conservative_FPE:train"],
                   check=True, env=env)


if __name__ == "__main__":
    main()
