#!/usr/bin/env python3
"""Capture the golden vectors of the reference's NIOFP2D_Trans_attn and its state_dict layout (CPU;
run where the reference checkout is available -- it never travels with the tests).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_trans_attn.py --ref <reference checkout>

``nio2d_trans_attn_train.npz``: 2d_FPE's NIOFP2D_Trans_attn(2, 3, 100, 25, 2, 6, 8, 2, 61, 61)
(2d_FPE/NIOModules.py:169-296) in train mode on x (1, 52, 61, 61) with a linspace(-1, 1) grid and
np.random.seed(17) for the bag draw: L = randint(50, 52) = 51 draws with replacement, so the
recorded draw holds duplicates (asserted).  The parameters come from the numpy recipe
(``layout_json`` / ``recipe_seed`` regenerate them through recipe.make_state) with the factors of
make_golden_trans.RESCALE (stored as ``rescale_json``); x is the recipe array ``nio2d_trans_attn.x``
and is not stored.  Stored: the output, the cotangent, idx, L and every gradient that is not None
(``branch.*``, ``fc0.*`` and the Transolver's ``placeholder`` get none).

The token attention must be shown to matter in the fixture: with the attention matrix replaced by
the identity, and by the uniform 1 / (L + 2), the REFERENCE's own fp32 output must move by at least
10 x OUT_TOL (relative) each.  If a recipe seed fails either one, take the next seed, never another
bar (make_golden_trans's seed 511 and 512 leave the attention too close to the identity; 513 is
the first that passes both).

``layouts_trans_attn.json``: names / shapes / dtypes of NIOFP2D_Trans_attn(2,3,100,25,3,12,32,2,61,61)
in both 2D experiments.

After the capture the float64 restatement (tests/trans_attn_ref.niofp2d_trans_attn) runs on the same
recipe parameters and the fp32 reference must sit inside every bar tests/test_trans_attn_ref.py
applies (those of tests/test_transolver_ref.py).
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

from make_golden_trans import RESCALE, _install_timm_stub, _layout, grid_of  # noqa: E402

CTOR = (2, 3, 100, 25, 2, 6, 8, 2, 61, 61)
LAYOUT_CTOR = (2, 3, 100, 25, 3, 12, 32, 2, 61, 61)
X_SHAPE = (1, 52, 61, 61)
RECIPE_SEED = 513      # 511 and 512 fail the identity bar (3.0e-5, 1.1e-5)
COT_SEED = 45
BAG_SEED = 17
HEADS = ("fno_drift", "fno_diffusion")

# the bars of tests/test_trans_attn_ref.py (those of tests/test_transolver_ref.py)
OUT_TOL, G_TOL = 1e-4, 1e-3


class _Functional:
    """Stands in for ``torch.nn.functional`` inside NIOModules: ``softmax`` of the (B, T, T) token
    scores returns the identity or the uniform matrix; everything else passes through."""

    def __init__(self, mode):
        self.mode = mode

    def __getattr__(self, name):
        import torch.nn.functional as F
        return getattr(F, name)

    def softmax(self, z, dim=-1):
        import torch
        assert z.dim() == 3 and z.shape[1] == z.shape[2]
        T = z.shape[-1]
        if self.mode == "identity":
            return torch.eye(T, dtype=z.dtype).expand_as(z)
        return torch.full_like(z, 1.0 / T)


def _probe(NM, m, x, grid, mode):
    import numpy as np
    import torch
    saved = NM.F
    NM.F = _Functional(mode)
    try:
        np.random.seed(BAG_SEED)
        with torch.no_grad():
            return m(x, grid)
    finally:
        NM.F = saved


def capture(what):
    import numpy as np
    import torch
    _install_timm_stub()
    import NIOModules as NM
    from recipe import make_array
    import transolver_ref

    torch.set_num_threads(8)
    if what == "layout":
        return _layout(NM.NIOFP2D_Trans_attn(*LAYOUT_CTOR))
    m = NM.NIOFP2D_Trans_attn(*CTOR)
    shapes = [(k, tuple(v.shape)) for k, v in m.state_dict().items()]
    st = transolver_ref.rescaled_state(shapes, RECIPE_SEED, RESCALE)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in st.items()})
    m.train()
    x = torch.from_numpy(make_array(X_SHAPE, RECIPE_SEED, "nio2d_trans_attn.x"))
    grid = torch.from_numpy(grid_of(X_SHAPE[2]))
    np.random.seed(BAG_SEED)
    L = np.random.randint(50, X_SHAPE[1])
    idx = np.random.choice(X_SHAPE[1], L)
    assert L == 51, "the fixture records 51 draws"
    assert len(set(idx.tolist())) < L, "the recorded draw must hold a duplicate"
    np.random.seed(BAG_SEED)
    out = m(x, grid)
    moves = {}
    for mode in ("identity", "uniform"):
        o = _probe(NM, m, x, grid, mode)
        moves[mode] = float((o - out.detach()).norm() / out.detach().norm())
    print(f"  the reference's output moves by {moves['identity']:.2e} with the identity for the attention "
          f"matrix, by {moves['uniform']:.2e} with the uniform matrix")
    if min(moves.values()) < 10 * OUT_TOL:
        raise SystemExit("the token attention does not matter at this RECIPE_SEED: take the next")
    cot = torch.from_numpy(make_array(tuple(out.shape), COT_SEED, "nio2d_trans_attn_train.cot"))
    (out * cot).sum().backward()
    arr = {"out": out.detach().numpy(), "cot": cot.numpy(), "in.grid": grid.numpy(), "L": np.asarray(L),
           "idx": idx, "x_shape": np.asarray(X_SHAPE), "recipe_seed": np.asarray(RECIPE_SEED),
           "bag_seed": np.asarray(BAG_SEED),
           "rescale_json": np.asarray(json.dumps(RESCALE)),
           "identity_move_out": np.asarray(moves["identity"]),
           "uniform_move_out": np.asarray(moves["uniform"]),
           "layout_json": np.asarray(json.dumps([[k, list(s)] for k, s in shapes]))}
    for k, p in m.named_parameters():
        if p.grad is not None:
            arr["g." + k] = p.grad.numpy()
    assert not any(k.startswith(("g.branch.", "g.fc0.")) or k == "g.trans_input.placeholder" for k in arr)
    check_against_fp64(arr, st, x)
    path = os.path.join(HERE, "nio2d_trans_attn_train.npz")
    np.savez_compressed(path, **arr)
    print(f"  wrote nio2d_trans_attn_train.npz ({os.path.getsize(path) / 1024:.1f} KiB, {len(arr)} arrays)")
    assert os.path.getsize(path) <= os.path.getsize(os.path.join(HERE, "nio2d_fno_attn_train.npz"))
    return None


def check_against_fp64(arr, st, x):
    """The fp32 reference against the float64 restatement on the same parameters: every bar of
    tests/test_trans_attn_ref.py, printed and asserted."""
    import numpy as np
    import torch
    import trans_attn_ref

    p = {k: torch.from_numpy(v).double().requires_grad_(v.dtype.kind == "f") for k, v in st.items()}
    grid = torch.from_numpy(arr["in.grid"]).double()
    idx = arr["idx"].tolist()
    y = trans_attn_ref.niofp2d_trans_attn(p, x.double(), grid, idx=idx, heads=HEADS)
    (y * torch.from_numpy(arr["cot"]).double()).sum().backward()

    def rel(a, b):
        return float(np.linalg.norm((a - b).ravel()) / np.linalg.norm(b.ravel()))

    e = rel(arr["out"], y.detach().numpy())
    moves = {}
    with torch.no_grad():
        for mode in ("identity", "uniform"):
            ym = trans_attn_ref.niofp2d_trans_attn(p, x.double(), grid, idx=idx, heads=HEADS, attn=mode)
            moves[mode] = rel(ym.numpy(), y.detach().numpy())
    print(f"  fp32 reference vs float64: out {e:.2e}; float64 moves of the output: identity "
          f"{moves['identity']:.2e}, uniform {moves['uniform']:.2e}")
    assert e <= OUT_TOL, e
    assert min(moves.values()) >= 10 * OUT_TOL, moves
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
        layouts[f"{key}.NIOFP2D_Trans_attn({','.join(map(str, LAYOUT_CTOR))})"] = json.loads(line[7:])
    with open(os.path.join(HERE, "layouts_trans_attn.json"), "w") as f:
        json.dump(layouts, f, indent=0)
    print("  wrote layouts_trans_attn.json")
    subprocess.run([sys.executable, __file__, "--ref", a.ref, "--capture", "2d_FPE:train"], check=True, env=env)


if __name__ == "__main__":
    main()
