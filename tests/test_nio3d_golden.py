"""NIOFP3D and the 3D snapshot encoders without a GPU: the drop-in classes' state_dict layouts
against the reference's (tests/golden/layouts3d.json), the float64 restatement
(tests/nio3d_ref.py) pinned to the reference's golden run (tests/golden/nio3d_train*.npz), the new
host-only queries, and the shapes that must be rejected.

Bars, as for nio2d_nc_train (BatchNorm over ~50 volumes in the reference's fp32): out rel-L2 <=
1e-4, g.* rel-L2 <= 1e-3, gnorm.* within 1e-3 |v| + 1e-5 gmax.  At capture time the fp32 reference
sat at 3e-7 (out) and inside every gradient bar against this restatement
(make_golden_nio3d.check_against_fp64).
"""
import json
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN, ROOT, load_golden, rel_l2
from recipe import make_array

import nio3d_ref

CTOR = (3, 3, 100, 25, 2, 6, 4, 1, "cpu")


def load_nio3d():
    g = load_golden("nio3d_train")
    if os.path.exists(os.path.join(GOLDEN, "nio3d_train_bwd.npz")):
        g.update(load_golden("nio3d_train_bwd"))
    return g


def golden_state(g):
    """(numpy state from the recipe, x) of the golden case."""
    shapes = [(k, tuple(s)) for k, s in json.loads(str(g["layout_json"]))]
    st = nio3d_ref.make_state3d(shapes, int(g["recipe_seed"]), json.loads(str(g["complex_json"])))
    x = make_array(tuple(int(v) for v in g["x_shape"]), int(g["recipe_seed"]), "nio3d.x")
    return st, x


def check_grads(g, grad_of, grid_grad):
    """The golden's gradient bars on a {name: gradient tensor} lookup."""
    gmax = max(float(v) for k, v in g.items() if k.startswith("gnorm."))
    n = 0
    for k, v in g.items():
        if k.startswith("g."):
            got = grad_of(k[2:])
            got = (torch.view_as_real(got) if got.is_complex() else got).detach().cpu().numpy()
            e = rel_l2(got, v)
            assert e <= 1e-3, (k, e)
            n += 1
        elif k.startswith("gnorm."):
            # conv biases ahead of a train-mode BatchNorm have exactly zero gradient; the fp32
            # reference leaves ~1e-10 noise there, hence the absolute term
            got = float(grad_of(k[6:]).double().norm())
            assert abs(got - float(v)) <= 1e-3 * abs(float(v)) + 1e-5 * gmax, (k, got, float(v))
            n += 1
    assert n > 40
    if grid_grad is not None:
        assert rel_l2(grid_grad.detach().cpu().numpy(), g["gin.grid"]) <= 1e-3


def test_ref_matches_reference_golden():
    g = load_nio3d()
    st, x = golden_state(g)
    assert len(g["idx"]) == int(g["L"])
    p = nio3d_ref.leaves(st)
    grid = torch.from_numpy(g["in.grid"]).double().requires_grad_(True)
    y = nio3d_ref.niofp3d(p, torch.from_numpy(x).double(), grid, idx=g["idx"].tolist())
    e = rel_l2(y.detach().numpy(), g["out"])
    print(f"nio3d_train: fwd {e:.2e}")
    assert e <= 1e-4, e
    (y * torch.from_numpy(g["cot"]).double()).sum().backward()
    check_grads(g, lambda k: p[k].grad, grid.grad)


def _layout(m):
    return [[k, list(v.shape), str(v.dtype).replace("torch.", "")] for k, v in m.state_dict().items()]


def test_layouts_match_reference():
    import blindno
    lay = json.load(open(os.path.join(GOLDEN, "layouts3d.json")))
    assert _layout(blindno.NIOFP3D(*CTOR)) == lay["NIOFP3D(3,3,100,25,2,6,4,1)"]
    assert _layout(blindno.NIOFP3D(*CTOR, down=True)) == lay["NIOFP3D(3,3,100,25,2,6,4,1,down)"]
    assert _layout(blindno.Encoder3D(25)) == lay["Encoder3D(25)"]
    assert _layout(blindno.Encoder3D_down(25)) == lay["Encoder3D_down(25)"]
    blk = blindno.ConvBlock3D(4, 6, kernel_size=(1, 7, 7), stride=(1, 2, 2), padding=(0, 3, 3))
    assert _layout(blk) == lay["ConvBlock3D(4,6,(1,7,7),(1,2,2),(0,3,3))"]
    # the two encoders differ in the last kernel only
    a, b = blindno.Encoder3D(25).state_dict(), blindno.Encoder3D_down(25).state_dict()
    assert tuple(a["convblock7_3.layers.0.weight"].shape) == (512, 512, 2, 1, 1)
    assert tuple(b["convblock7_3.layers.0.weight"].shape) == (512, 512, 1, 1, 1)


def test_golden_layout_is_the_drop_in_layout():
    """The recipe layout stored with the golden (names and shapes the reference's NIOFP3D had at
    capture time) is the drop-in model's: its parameters load with strict=True."""
    import blindno
    g = load_golden("nio3d_train")
    st, _ = golden_state(g)
    m = blindno.NIOFP3D(*CTOR)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in st.items()}, strict=True)
    assert sum(p.numel() for p in m.parameters()) > 28_000_000


def test_dropin_namespaces():
    from blindno import dropin
    import blindno
    for exp in ("2d_FPE", "2d_Non_conservative_FPE"):
        assert dropin.module(exp, "NIOModules").NIOFP3D is blindno.NIOFP3D
    for exp in ("1d_FPE", "1d_GPE"):      # their NIOModules.py never defines the class
        assert not hasattr(dropin.module(exp, "NIOModules"), "NIOFP3D")
    for exp in dropin.EXPERIMENTS:
        b = dropin.module(exp, "Baselines")
        assert (b.ConvBlock3D, b.Encoder3D, b.Encoder3D_down) == \
            (blindno.ConvBlock3D, blindno.Encoder3D, blindno.Encoder3D_down)


def test_non_bn_blocks_take_the_torch_path():
    """norm='in', no norm and dropout run as plain torch modules (as ConvBlock does), on the CPU too."""
    import blindno
    torch.manual_seed(0)
    x = torch.randn(2, 3, 4, 5, 6)
    for kw in ({"norm": "in"}, {"norm": None}, {"dropout": 0.5}):
        blk = blindno.ConvBlock3D(3, 4, **kw).eval()
        assert torch.equal(blk(x), blk.layers(x))
        assert blk(x).shape == (2, 4, 4, 5, 6)


@pytest.mark.parametrize("cls,shape", [("Encoder3D", (32, 9, 10)), ("Encoder3D", (65, 9, 10)),
                                       ("Encoder3D", (40, 65, 10)), ("Encoder3D", (40, 10, 65)),
                                       ("Encoder3D_down", (33, 9, 10)), ("Encoder3D_down", (16, 65, 8))])
def test_unsupported_grids_raise(cls, shape):
    import blindno
    enc = getattr(blindno, cls)(25)
    with pytest.raises(ValueError, match="does not reduce to one voxel"):
        enc(torch.zeros(1, 2, 1, *shape))


def test_cpu_tensors_are_rejected():
    import blindno
    m = blindno.NIOFP3D(3, 2, 16, 25, 2, 4, 2, 1, "cpu")
    with pytest.raises(blindno.BlindnoError):
        m(torch.zeros(1, 60, 33, 4, 4), torch.zeros(33, 4, 4, 3))
    with pytest.raises(blindno.BlindnoError):
        blindno.Encoder3D(25)(torch.zeros(1, 2, 1, 33, 4, 4))


def test_conv3d_split_queries_without_a_device():
    """Host-only size queries work without a device; an output extent of 0 is refused."""
    from blindno import _lib
    g = (7, 512, 3, 1, 1, 512, 3, 3, 3, 2, 2, 2, 1, 1, 1)
    assert _lib.query("blindno_conv3d_fwd_nsplit", *g) > 1
    assert _lib.query("blindno_conv3d_bwd_data_nsplit", *g) > 1
    assert _lib.query("blindno_conv3d_wgrad_nsplit", *g) >= 1
    assert _lib.query("blindno_conv3d_fwd_nsplit", 7, 512, 1, 1, 1, 512, 3, 3, 3, 2, 2, 2, 0, 0, 0) == -1
    src = open(os.path.join(ROOT, "reconstruction-of-pde-without-time-label_amd", "csrc", "conv3d.hip")).read()
    assert "atomic" not in src.lower()
