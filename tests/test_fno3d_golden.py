"""The 3D Fourier layer without a GPU: the float64 restatement (tests/fno3d_ref.py) pinned to the
reference's golden vectors, the drop-in modules' layout, the host-only queries and the shapes that
must be rejected.

Bars: forward rel-L2 <= 1e-5, gradients rel-L2 <= 1e-4.  The reference's own fp32
forward sits 1.3e-7 .. 1.7e-7 from the float64 restatement at these cases.
"""
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN, load_golden, rel_l2

import fno3d_ref

FWD_TOL = 1e-5
GRAD_TOL = 1e-4

# case -> (kind, constructor arguments)
CASES = {
    "sc3d_a": ("sc3d", (3, 4, 2, 3, 2)),
    "sc3d_overlap": ("sc3d", (2, 3, 3, 3, 3)),
    "sc3d_nyq": ("sc3d", (2, 2, 2, 2, 3)),
    "sc3d_tiles": ("sc3d", (4, 4, 4, 4, 4)),
    "fno3d_a": ("fno3d", (3, 5, 4, 4, 2)),
    "fno3d_b": ("fno3d", (4, 8, 4, 3, 1)),
}


def load3d(name):
    """A golden case; the large ones keep their backward arrays in <name>_bwd.npz."""
    g = load_golden(name)
    if os.path.exists(os.path.join(GOLDEN, name + "_bwd.npz")):
        g.update(load_golden(name + "_bwd"))
    return g


@pytest.mark.parametrize("case", list(CASES))
def test_ref_matches_reference_golden(case):
    g = load3d(case)
    p = {k[2:]: v for k, v in g.items() if k.startswith("p.")}
    out, grads, gin = fno3d_ref.run(CASES[case][0], p, g["in.x"], g["cot"])
    e = rel_l2(out.numpy(), g["out"])
    print(f"{case}: fwd {e:.2e}")
    assert e <= FWD_TOL, e
    e = rel_l2(gin.numpy(), g["gin.x"])
    assert e <= GRAD_TOL, ("gin.x", e)
    n = 0
    for k, v in g.items():
        if k.startswith("g."):
            e = rel_l2(grads[k[2:]].numpy(), v)
            assert e <= GRAD_TOL, (k, e)
            n += 1
    assert n == len(p)


def test_overlap_losers_get_zero_gradient():
    """sc3d_overlap: 2 m > P on axes 1 and 2 -- the entries of weights1..3 that a later corner
    overwrites have exactly zero gradient in the reference, and ref.winners names them."""
    g = load3d("sc3d_overlap")
    masks = fno3d_ref.winners(3, 3, 5, 5)
    assert not all(bool(m.all()) for m in masks[:3])
    assert bool(masks[3].all())
    for q, m in enumerate(masks):
        gw = torch.from_numpy(g[f"g.weights{q + 1}"])
        assert float(gw[:, :, ~m].abs().max() if (~m).any() else 0.0) == 0.0
        assert float(gw[:, :, m].abs().min()) > 0.0


def test_mixed_spectrum_restates_the_layer():
    """ref.mixed_spectrum_planes (the checker of blindno_colpass3d alone) composed with the
    last-axis transforms is the layer, and its direction 1 is its adjoint."""
    g = load3d("sc3d_overlap")
    x = fno3d_ref.to64(g["in.x"])
    ws = [fno3d_ref.to64(g[f"p.weights{q}"]) for q in range(1, 5)]
    P = tuple(x.shape[2:])
    m3 = ws[0].shape[4]
    At = torch.fft.rfft(x, dim=-1)[..., :m3].permute(0, 4, 1, 2, 3)
    Z = fno3d_ref.mixed_spectrum_planes(At, ws, P, 0)               # (B, P1, P2, m3, Co)
    k = torch.arange(m3, dtype=torch.float64)
    z = torch.arange(P[2], dtype=torch.float64)
    E = torch.exp(2j * torch.pi * k[:, None] * z[None, :] / P[2])
    y = torch.einsum("bxykc,kz->bcxyz", Z, E).real
    assert rel_l2(y.numpy(), fno3d_ref.spectral_conv3d(x, ws).numpy()) <= 1e-12
    gen = torch.Generator().manual_seed(5)
    b = torch.randn(Z.shape, dtype=torch.float64, generator=gen) + 1j * torch.randn(
        Z.shape, dtype=torch.float64, generator=gen)
    # <L a, b> = <a, L^H b> with a = At, b over Z's index set (adjoint input laid out like At)
    bt = b.permute(0, 3, 4, 1, 2)
    Lb = fno3d_ref.mixed_spectrum_planes(bt, ws, P, 1)              # (B, P1, P2, m3, Ci)
    lhs = torch.sum(Z.conj() * b).real
    rhs = torch.sum(At.permute(0, 3, 4, 1, 2).conj() * Lb).real
    assert abs(float(lhs - rhs)) <= 1e-10 * abs(float(lhs))


def test_fno3d_state_dict_layout():
    import blindno
    g = load3d("fno3d_a")
    sd = blindno.FNO3d(3, 5, 4, 4, 2).state_dict()
    want = {k[2:]: v for k, v in g.items() if k.startswith("p.")}
    assert list(sd) == list(want)
    for k, v in sd.items():
        assert tuple(v.shape) == want[k].shape, k
        assert str(v.dtype).replace("torch.", "") == str(want[k].dtype), k


def test_3d_queries_without_a_device():
    """Host-only queries work without a device."""
    from blindno import _lib
    assert _lib.query("blindno_spectral3d_ok", 4, 20, 20, 42, 42, 42, 8, 8, 8) == 1
    assert _lib.query("blindno_spectral3d_ok", 1, 33, 33, 8, 8, 8, 2, 2, 2) == 0      # C > 32
    assert _lib.query("blindno_lift3d_bwd_nchunk", 4, 40, 40, 40) >= 1
    assert _lib.query("blindno_project3d_bwd_nchunk", 4, 40, 40, 40) >= 1


def test_cpu_tensors_raise():
    import blindno
    from blindno._lib import BlindnoError
    with pytest.raises(BlindnoError, match="no CPU path"):
        blindno.FNO3d(3, 5, 4, 4, 2)(torch.randn(2, 6, 5, 7, 4))
    with pytest.raises(BlindnoError, match="no CPU path"):
        blindno.SpectralConv3d(3, 4, 2, 3, 2)(torch.randn(2, 3, 8, 7, 9))


@pytest.mark.parametrize("ctor,shape,msg", [
    ((2, 2, 7, 2, 2), (1, 2, 6, 6, 6), "exceed the grid"),          # m1 > P1
    ((2, 2, 2, 7, 2), (1, 2, 6, 6, 6), "exceed the grid"),          # m2 > P2
    ((2, 2, 2, 2, 5), (1, 2, 6, 6, 6), "exceed P3//2"),             # m3 > P3/2 + 1
    ((33, 33, 2, 2, 2), (1, 33, 6, 6, 6), "kernels' limits"),       # C > 32
    ((2, 2, 2, 2, 49), (1, 2, 4, 4, 100), "kernels' limits"),       # m3 > 48
])
def test_rejected_shapes_raise(ctor, shape, msg):
    """Shapes the reference rejects (a corner slice longer than its axis) and shapes past the
    kernels' limits raise before anything is launched (the check needs no device)."""
    import blindno
    from blindno._lib import BlindnoError
    with pytest.raises(BlindnoError, match=msg):
        blindno.SpectralConv3d(*ctor)(torch.randn(*shape))


def test_fno3d_rejects_modes_past_the_padded_grid():
    import blindno
    from blindno._lib import BlindnoError
    with pytest.raises(BlindnoError, match="exceed"):
        blindno.FNO3d(6, 4, 4, 3, 1)(torch.randn(1, 3, 3, 3, 3))    # padded 5^3: m3 = 6 > 3
