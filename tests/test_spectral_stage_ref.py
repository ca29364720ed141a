"""The float64 stage references of tests/spectral_stage_ref.py checked on the host, without a GPU:

* chained (row DFT -> column pass with pack_w2d-layout weights -> bare row inverse) they equal
  oracle.fno_ref.spectral_conv2d, and the 1D chain spectral_conv1d, to 1e-12 rel-L2;
* the adjoint stages are the true adjoints, <A x, y> = <x, A^H y> to 1e-12, and the chained
  adjoint equals the oracle's autograd gradient;
* the A-tile decode inverts the encode, which is a permutation of the plain Z.
"""
import numpy as np
import pytest
import torch

import spectral_stage_ref as sr
from conftest import rel_l2

import oracle.fno_ref as oref

# (Bn, Ci, Co, P1, P2, m1, m2)
SHAPES_2D = [
    pytest.param((2, 3, 4, 20, 18, 4, 5), id="no_overlap"),
    pytest.param((2, 2, 3, 6, 10, 4, 6), id="overlap_2m1_gt_P1_nyquist"),
    pytest.param((2, 3, 3, 12, 16, 3, 9), id="even_P2_nyquist"),
    pytest.param((2, 4, 2, 9, 15, 2, 8), id="odd_P2"),
]


def _crandn(rng, *shape):
    return rng.standard_normal(shape) + 1j * rng.standard_normal(shape)


def _inner(a, b):
    """The real inner product of two (real or complex) tensors."""
    return float(np.real(np.vdot(a, b)))


def _close(a, b, tol=1e-12):
    return abs(a - b) <= tol * max(abs(a), abs(b), 1e-300)


@pytest.mark.parametrize("geom", SHAPES_2D)
def test_chain_equals_oracle_2d(geom):
    Bn, Ci, Co, P1, P2, m1, m2 = geom
    rng = np.random.default_rng(sum(geom))
    x = rng.standard_normal((Bn, Ci, P1, P2))
    w1, w2 = _crandn(rng, Ci, Co, m1, m2), _crandn(rng, Ci, Co, m1, m2)
    At = sr.row_dft(x, m2)
    _, Z = sr.col_pass(At, sr.pack_w2d(w1, w2, P1), P1, P2, m1, 0)
    y = sr.row_inv(Z, P2)
    xt, w1t, w2t = (torch.from_numpy(a).requires_grad_(True) for a in (x, w1, w2))
    yo = oref.spectral_conv2d(xt, w1t, w2t)
    assert rel_l2(y, yo.detach().numpy()) <= 1e-12
    # the chained adjoint is the oracle's gradient w.r.t. the input
    dy = rng.standard_normal(y.shape)
    _, GZ = sr.col_pass(sr.row_dft(dy, m2), sr.pack_w2d(w1, w2, P1), P1, P2, m1, 1)
    dx = sr.row_inv_adj(GZ, P2)
    (dxo,) = torch.autograd.grad(yo, (xt,), torch.from_numpy(dy))
    assert rel_l2(dx, dxo.numpy()) <= 1e-12


@pytest.mark.parametrize("geom", [(3, 4, 5, 11, 20), (2, 3, 2, 8, 15), (5, 1, 1, 1, 8), (2, 5, 3, 6, 10)])
def test_chain_equals_oracle_1d(geom):
    Bn, Ci, Co, m, P2 = geom
    rng = np.random.default_rng(sum(geom))
    x = rng.standard_normal((Bn, Ci, P2))
    w = _crandn(rng, Ci, Co, m)
    At = sr.row_dft(x[:, :, None, :], m)[..., 0]                       # (Bn, m, Ci)
    _, Z = sr.mix1d(At, sr.pack_w1d(w), P2, 0)
    y = sr.row_inv(Z[:, None], P2)[:, :, 0]
    xt, wt = torch.from_numpy(x).requires_grad_(True), torch.from_numpy(w).requires_grad_(True)
    yo = oref.spectral_conv1d(xt, wt)
    assert rel_l2(y, yo.detach().numpy()) <= 1e-12
    dy = rng.standard_normal(y.shape)
    _, GZ = sr.mix1d(sr.row_dft(dy[:, :, None, :], m)[..., 0], sr.pack_w1d(w), P2, 1)
    dx = sr.row_inv_adj(GZ[:, None], P2)[:, :, 0]
    (dxo,) = torch.autograd.grad(yo, (xt,), torch.from_numpy(dy))
    assert rel_l2(dx, dxo.numpy()) <= 1e-12


@pytest.mark.parametrize("valid", [None, (5, 7)])
def test_row_inverse_is_the_adjoint_of_the_row_dft(valid):
    rng = np.random.default_rng(3)
    Bn, C, P1, P2, m2 = 2, 3, 6, 10, 6
    x = rng.standard_normal((Bn, C, P1, P2))
    A = _crandn(rng, Bn, m2, C, P1)
    lhs = _inner(sr.row_dft(x, m2, 0, valid), A)
    back = sr.row_inv_adj(np.ascontiguousarray(A.transpose(0, 3, 1, 2)), P2)   # At order -> Z order
    xv = x.copy()
    if valid is not None:
        back[:, :, valid[0]:, :] = 0
        back[:, :, :, valid[1]:] = 0
    assert _close(lhs, _inner(xv, back))


@pytest.mark.parametrize("geom", SHAPES_2D)
def test_col_pass_dir1_is_the_adjoint_of_dir0(geom):
    Bn, Ci, Co, P1, P2, m1, m2 = geom
    rng = np.random.default_rng(7 + sum(geom))
    Wt = _crandn(rng, m2, min(2 * m1, P1), Ci, Co)
    A = _crandn(rng, Bn, m2, Ci, P1)
    B = _crandn(rng, Bn, m2, Co, P1)
    _, Z0 = sr.col_pass(A, Wt, P1, P2, m1, 0)                      # (Bn, P1, m2, Co)
    _, Z1 = sr.col_pass(B, Wt, P1, P2, m1, 1)                      # (Bn, P1, m2, Ci)
    assert _close(_inner(Z0.transpose(0, 2, 3, 1), B), _inner(A, Z1.transpose(0, 2, 3, 1)))
    # the saved spectra: dir 1's is c_k/(P1 P2) times the column DFT that dir 0 saves
    X0, _ = sr.col_pass(B, np.conj(Wt.transpose(0, 1, 3, 2)), P1, P2, m1, 0)
    X1, _ = sr.col_pass(B, Wt, P1, P2, m1, 1)
    assert rel_l2(X1, X0 * (sr.c2r(m2, P2) / (P1 * P2))[None, :, None, None]) <= 1e-14


@pytest.mark.parametrize("geom", [(3, 4, 5, 11, 20), (2, 3, 2, 8, 15), (5, 1, 1, 1, 8)])
def test_mix1d_dir1_is_the_adjoint_of_dir0(geom):
    Bn, Ci, Co, m, P2 = geom
    rng = np.random.default_rng(11 + sum(geom))
    Wt = _crandn(rng, m, Ci, Co)
    A, B = _crandn(rng, Bn, m, Ci), _crandn(rng, Bn, m, Co)
    _, Z0 = sr.mix1d(A, Wt, P2, 0)
    _, Z1 = sr.mix1d(B, Wt, P2, 1)
    assert _close(_inner(Z0, B), _inner(A, Z1))


@pytest.mark.parametrize("act", [0, 1])
@pytest.mark.parametrize("crop", [None, (4, 7)])
def test_row_inverse_epilogue_adjoint(act, crop):
    """z(x) = rowinv(Z) + Wc f(x) + bc: its Jacobian w.r.t. x applied to v, paired with dz, equals
    <v, row_inv_adj(G = 0, dz)>; act 0 exactly (linear), act 1 by a central difference; the crop
    zeroes dz.  The weight-gradient sums are the derivatives of <z, dz> w.r.t. Wc and bc."""
    rng = np.random.default_rng(5 + act)
    Bn, C, P1, P2, m2 = 2, 3, 5, 9, 4
    Z = _crandn(rng, Bn, P1, m2, C)
    x, v, dz = (rng.standard_normal((Bn, C, P1, P2)) for _ in range(3))
    wc, bc = rng.standard_normal((C, C)), rng.standard_normal(C)
    dzc = sr._crop(dz, crop)
    dx = sr.row_inv_adj(np.zeros_like(Z), P2, dz, wc, x, act, crop)
    if act == 0:
        jv = sr.row_inv(Z, P2, x + v, wc, bc, 0) - sr.row_inv(Z, P2, x, wc, bc, 0)
        assert _close(_inner(jv, dzc), _inner(v, dx), 1e-12)
    else:
        e = 1e-5
        jv = (sr.row_inv(Z, P2, x + e * v, wc, bc, 1) - sr.row_inv(Z, P2, x - e * v, wc, bc, 1)) / (2 * e)
        assert _close(_inner(jv, dzc), _inner(v, dx), 1e-8)
    # the spectrum part: G enters like Z in the forward
    G = _crandn(rng, Bn, P1, m2, C)
    assert rel_l2(sr.row_inv_adj(G, P2), sr.row_inv(G, P2)) == 0.0
    g = sr.conv_wgrad(dz, x, act, crop)
    f = sr.gelu(x) if act else x
    assert rel_l2(g[:C * C].reshape(C, C), np.einsum("nohw,nihw->oi", dzc, f)) <= 1e-14
    assert rel_l2(g[C * C:], dzc.sum((0, 2, 3))) <= 1e-14


def test_gelu_matches_torch():
    x = np.linspace(-12, 12, 4001)
    xt = torch.from_numpy(x).requires_grad_(True)
    y = torch.nn.functional.gelu(xt)
    (g,) = torch.autograd.grad(y.sum(), (xt,))
    assert np.abs(sr.gelu(x) - y.detach().numpy()).max() <= 1e-14
    assert np.abs(sr.gelu_grad(x) - g.numpy()).max() <= 1e-14


@pytest.mark.parametrize("C", [8, 12, 16])
def test_tile_layout_round_trip(C):
    Bn, P1, m2 = 2, 20, 6
    n = Bn * P1 * m2 * C * 2
    Zr = np.arange(n, dtype=np.float64).reshape(Bn, P1, m2, C, 2)    # every element distinct
    Zt = sr.tile_encode(Zr)
    assert Zt.shape == (n,)
    assert np.array_equal(np.sort(Zt), Zr.ravel())                    # a permutation of the plain Z
    assert not np.array_equal(Zt, Zr.ravel())
    assert np.array_equal(sr.tile_decode(Zt, Bn, P1, m2, C), Zr)
    # the formula at one hand-computed element: q = 3, g = 1, s = 2, l = 37 -> row 13, kk = 10
    # (k = 5, Re), channel 5
    l, q, g, s = 37, 3, 1, 2
    assert Zt[((q * (C // 4) + g) * (m2 // 2) + s) * 64 + l] == Zr.reshape(Bn * P1, m2, C, 2)[13, 5, 5, 0]


def test_tile_layout_rule():
    assert sr.tile_layout(2, 12, 32, 32, 8) == 1
    assert sr.tile_layout(2, 8, 16, 100, 48) == 1
    assert sr.tile_layout(2, 12, 16, 100, 34) == 0       # m2/2 > 16 for C = 12
    assert sr.tile_layout(2, 8, 16, 32, 9) == 0          # odd m2
    assert sr.tile_layout(2, 12, 18, 40, 20) == 0        # P1 % 4
    assert sr.tile_layout(2, 4, 16, 32, 8) == 0
    assert sr.tile_layout(2, 16, 12, 32, 8) == 0         # P1 < 16


def test_abs_twins_dominate():
    """|stage(x)| <= stage_abs(x) elementwise (the triangle inequality): the S_abs of the bound."""
    rng = np.random.default_rng(9)
    Bn, Ci, Co, P1, P2, m1, m2 = 2, 3, 4, 8, 10, 3, 5
    x = rng.standard_normal((Bn, Ci, P1, P2))
    At = sr.row_dft(x, m2, 1, (6, 7))
    S, cnt = sr.row_dft_abs(x, m2, 1, (6, 7))
    assert np.all(np.abs(At) <= S + 1e-15) and cnt.max() == 7 and cnt.min() == 0
    Wt = _crandn(rng, m2, 6, Ci, Co)
    for d in (0, 1):
        A = _crandn(rng, Bn, m2, Ci if d == 0 else Co, P1)
        X, Z = sr.col_pass(A, Wt, P1, P2, m1, d)
        Xa, Za = sr.col_pass_abs(A, Wt, P1, P2, m1, d)
        assert np.all(np.abs(X) <= Xa * (1 + 1e-14)) and np.all(np.abs(Z) <= Za * (1 + 1e-14))
    Zc = _crandn(rng, Bn, P1, m2, Ci)
    wc, bc = rng.standard_normal((Ci, Ci)), rng.standard_normal(Ci)
    dz = rng.standard_normal(x.shape)
    for act in (0, 1):
        S, _ = sr.row_inv_abs(Zc, P2, x, wc, bc, act)
        assert np.all(np.abs(sr.row_inv(Zc, P2, x, wc, bc, act)) <= S * (1 + 1e-14))
        S, _ = sr.row_inv_adj_abs(Zc, P2, dz, wc, x, act, (5, 9))
        assert np.all(np.abs(sr.row_inv_adj(Zc, P2, dz, wc, x, act, (5, 9))) <= S * (1 + 1e-14))
        S, _ = sr.conv_wgrad_abs(dz, x, act, (5, 9))
        assert np.all(np.abs(sr.conv_wgrad(dz, x, act, (5, 9))) <= S * (1 + 1e-14))
