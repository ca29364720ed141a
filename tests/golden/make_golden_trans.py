#!/usr/bin/env python3
"""Capture the golden vectors of the reference's NIOFP2D_Trans and its state_dict layout (CPU; run
where the reference checkout is available -- it never travels with the tests).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_trans.py --ref <reference checkout>

``nio2d_trans_train.npz``: 2d_FPE's NIOFP2D_Trans(2, 3, 100, 25, 2, 6, 8, 2)
(2d_FPE/NIOModules.py:85-166) in train mode on x (1, 52, 61, 61) with a linspace(-1, 1) grid and
np.random.seed(17) for the bag draw: L = randint(50, 52) = 51 draws with replacement, so the
recorded draw holds duplicates (asserted).  The parameters come from the numpy recipe
(``layout_json`` / ``recipe_seed`` regenerate them through recipe.make_state); x is the recipe array
``nio2d_trans.x`` and is not stored.  Stored: the output, the cotangent, idx, L and every gradient
that is not None (``branch.*``, ``fc0.*`` and the Transolver's ``placeholder`` get none).

The recipe's parameter draw is not the reference's initialisation, and at the recipe's own scales
(LayerNorm gains within +-0.1, fan-in bounded weights) the attention branch is negligible at every
seed.  The generator therefore multiplies the recipe's draw of some parameters by the factors of
RESCALE (keyed by name suffix: the LayerNorm gains x 10, in_project_fx and to_out x 4, in_project_x
x 2), through transolver_ref.rescaled_state, and stores them as ``rescale_json`` so the tests
rebuild the same parameters.  The attention must then be shown to matter in the fixture: with the slice weights w of every block replaced by the uniform 1/16 the
REFERENCE's own fp32 output must move by at least 10 x OUT_TOL (relative), and the slices must not
be near-uniform (the mean row maximum of w, recorded as ``w_rowmax_mean``, must exceed 2/16).  If a
seed fails, take the next seed, never another bar.

``layouts_trans.json``: names / shapes / dtypes of NIOFP2D_Trans(2,3,100,25,3,12,32,2) in both 2D
experiments.

After the capture the float64 restatement (tests/transolver_ref.niofp2d_trans) runs on the same
recipe parameters and the fp32 reference must sit inside every bar tests/test_transolver_ref.py
applies (those of tests/test_nio2d_attn.py).
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
X_SHAPE = (1, 52, 61, 61)
RECIPE_SEED = 511
COT_SEED = 44
BAG_SEED = 17
HEADS = ("fno_drift", "fno_diffusion")
RESCALE = {"Attn.to_out.0.weight": 4, "Attn.in_project_x.weight": 2, "Attn.in_project_fx.weight": 4,
           "ln_1.weight": 10, "ln_2.weight": 10, "ln_3.weight": 10}

# the bars of tests/test_transolver_ref.py (those of tests/test_nio2d_attn.py)
OUT_TOL, G_TOL = 1e-4, 1e-3
ROWMAX_MIN = 2.0 / 16


def _install_timm_stub():
    # the vendored Transolver needs one name of timm
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


def _slice_probe(n_points, uniform, seen):
    """Stands in for an attention module's ``softmax``: records the slice weights' row maxima and,
    with ``uniform``, replaces the slice weights (the (.., N, 16) call) by 1/16; the 16 x 16 token
    softmax passes through."""
    import torch

    class Probe(torch.nn.Module):
        def forward(self, z):
            w = torch.softmax(z, dim=-1)
            if z.shape[-2] == n_points:
                seen.append(float(w.max(-1).values.mean()))
                if uniform:
                    return torch.full_like(w, 1.0 / w.shape[-1])
            return w
    return Probe()


def _probe(m, x, grid, uniform):
    import numpy as np
    import torch
    seen = []
    saved = [(b.Attn, b.Attn.softmax) for b in m.trans_input.blocks]
    for attn, _ in saved:
        attn.softmax = _slice_probe(X_SHAPE[2] * X_SHAPE[3], uniform, seen)
    try:
        np.random.seed(BAG_SEED)
        with torch.no_grad():
            out = m(x, grid)
    finally:
        for attn, sm in saved:
            attn.softmax = sm
    return out, float(np.mean(seen))


def capture(what):
    import numpy as np
    import torch
    _install_timm_stub()
    import NIOModules as NM
    from recipe import make_array
    import transolver_ref

    torch.set_num_threads(8)
    if what == "layout":
        return _layout(NM.NIOFP2D_Trans(*LAYOUT_CTOR))
    m = NM.NIOFP2D_Trans(*CTOR)
    shapes = [(k, tuple(v.shape)) for k, v in m.state_dict().items()]
    st = transolver_ref.rescaled_state(shapes, RECIPE_SEED, RESCALE)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in st.items()})
    m.train()
    x = torch.from_numpy(make_array(X_SHAPE, RECIPE_SEED, "nio2d_trans.x"))
    grid = torch.from_numpy(grid_of(X_SHAPE[2]))
    np.random.seed(BAG_SEED)
    L = np.random.randint(50, X_SHAPE[1])
    idx = np.random.choice(X_SHAPE[1], L)
    assert L == 51, "the fixture records 51 draws"
    assert len(set(idx.tolist())) < L, "the recorded draw must hold a duplicate"
    out_a, rowmax = _probe(m, x, grid, uniform=False)
    out_u, _ = _probe(m, x, grid, uniform=True)
    move = float((out_a - out_u).norm() / out_a.norm())
    print(f"  mean row max of w {rowmax:.3f}; uniform slice weights move the reference's output by {move:.2e}")
    if move < 10 * OUT_TOL or rowmax <= ROWMAX_MIN:
        raise SystemExit("the attention does not matter at this RECIPE_SEED: take the next")
    np.random.seed(BAG_SEED)
    out = m(x, grid)
    assert torch.equal(out.detach(), out_a), "the probed forward is the model's own"
    cot = torch.from_numpy(make_array(tuple(out.shape), COT_SEED, "nio2d_trans_train.cot"))
    (out * cot).sum().backward()
    arr = {"out": out.detach().numpy(), "cot": cot.numpy(), "in.grid": grid.numpy(), "L": np.asarray(L),
           "idx": idx, "x_shape": np.asarray(X_SHAPE), "recipe_seed": np.asarray(RECIPE_SEED),
           "w_rowmax_mean": np.asarray(rowmax),
           "rescale_json": np.asarray(json.dumps(RESCALE)), "uniform_move_out": np.asarray(move),
           "layout_json": np.asarray(json.dumps([[k, list(s)] for k, s in shapes]))}
    for k, p in m.named_parameters():
        if p.grad is not None:
            arr["g." + k] = p.grad.numpy()
    assert not any(k.startswith(("g.branch.", "g.fc0.")) or k == "g.trans_input.placeholder" for k in arr)
    check_against_fp64(arr, st, x)
    path = os.path.join(HERE, "nio2d_trans_train.npz")
    np.savez_compressed(path, **arr)
    print(f"  wrote nio2d_trans_train.npz ({os.path.getsize(path) / 1024:.1f} KiB, {len(arr)} arrays)")
    assert os.path.getsize(path) <= os.path.getsize(os.path.join(HERE, "nio2d_fno_attn_train.npz"))
    return None


def check_against_fp64(arr, st, x):
    """The fp32 reference against the float64 restatement on the same parameters: every bar of
    tests/test_transolver_ref.py, printed and asserted."""
    import numpy as np
    import torch
    import transolver_ref

    p = {k: torch.from_numpy(v).double().requires_grad_(v.dtype.kind == "f") for k, v in st.items()}
    grid = torch.from_numpy(arr["in.grid"]).double()
    idx = arr["idx"].tolist()
    rec = []
    y = transolver_ref.niofp2d_trans(p, x.double(), grid, idx=idx, heads=HEADS, record=rec)
    (y * torch.from_numpy(arr["cot"]).double()).sum().backward()
    with torch.no_grad():
        yu = transolver_ref.niofp2d_trans(p, x.double(), grid, idx=idx, heads=HEADS, uniform=True)

    def rel(a, b):
        return float(np.linalg.norm((a - b).ravel()) / np.linalg.norm(b.ravel()))

    e = rel(arr["out"], y.detach().numpy())
    move = rel(yu.numpy(), y.detach().numpy())
    rowmax = float(np.mean([float(w.max(2).values.mean()) for w in rec]))
    print(f"  fp32 reference vs float64: out {e:.2e}; float64 uniform-slice move of the output {move:.2e}; "
          f"mean row max {rowmax:.3f}")
    assert e <= OUT_TOL, e
    assert move >= 10 * OUT_TOL, move
    assert abs(rowmax - float(arr["w_rowmax_mean"])) <= 1e-4
    errs = {k: rel(v, p[k[2:]].grad.numpy()) for k, v in arr.items() if k.startswith("g.")}
    worst = max(errs, key=errs.get)
    print(f"  max g.* {errs[worst]:.2e} ({worst}, {len(errs)} gradients)")
    assert errs[worst] <= G_TOL, (worst, errs[worst])


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
        layouts[f"{key}.NIOFP2D_Trans({','.join(map(str, LAYOUT_CTOR))})"] = json.loads(line[7:])
    with open(os.path.join(HERE, "layouts_trans.json"), "w") as f:
        json.dump(layouts, f, indent=0)
    print("  wrote layouts_trans.json")
    subprocess.run([sys.executable, __file__, "--ref", a.ref, "--capture", "2d_FPE:train"], check=True, env=env)


if __name__ == "__main__":
    main()
